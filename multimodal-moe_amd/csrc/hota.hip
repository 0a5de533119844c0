// HOTA on the GPU (hota.py: hota_pass_a / hota_gas / hota_pass_b, which
// moteval.evaluate(..., hota=True) runs on the host with MOE_TRACK_EVAL=0).
//
// HOTA's per-frame assignment depends on a score table that is global to the
// sequence and on nothing of the frame before, so -- unlike moteval.hip, whose
// frames are serial by the rule -- every frame gets a 64-lane workgroup of its
// own: the grid is the launch's F frames, whatever sequences they belong to
// (frame_slot[f] names the state slot).  Everything the frames share is added
// with INTEGER atomics (exact and commutative: the result is the reference's
// bits in any order); the one floating-point sum, the localisation sum, leaves
// the kernel as a plain [F][19] buffer of per-frame partials that the host adds
// in frame order.  No floating-point atomic anywhere.
//
//   hota_pass_a_kernel  rows into LDS as moteval.hip's step 1; in a frame with a
//       flag-0 row the ignore-region solve (moteval.hip's step 2, the same cost)
//       and the keep-mask of its tracker rows into a [F][K] workspace, so that
//       pass B does not solve the removal again; the truths and the remaining
//       rows listed; a lane per row walks the truths and a lane per truth walks
//       the rows for the fp64 sums (sequential adds in row order, the rule's),
//       kept in LDS where the solver's arrays were; a lane per pair adds
//       rint(sim_iou * 2^32) to pot_q (64-bit atomic), a lane per truth / row
//       counts gt_count / trk_count (32-bit atomics).
//   hota_gas_kernel     one thread per cell: gas = fp32(pot_q / (2^32 (gc + tc) -
//       pot_q)), the denominator in int64, one correctly rounded fp64 division.
//   hota_pass_b_kernel  rows and keep-mask into LDS; ONE lsap_solve with cost
//       -(gas[g][t] * iou), gas read from global memory (L2), iou from the boxes;
//       per threshold the pairs with (double)iou >= alpha[a] are counted with
//       ballots and mc gets a 32-bit atomic per counted pair; lane 0 adds TP / FN
//       / FP (64-bit atomics); lane a < 19 adds the frame's loc partial of
//       threshold a in ground-truth row order and stores it.
//
// IoU is moteval.hip's mot_iou restated (fp32, each operation rounded on its
// own); no FMA contraction (pragma below) and no fast-math flag reaches this
// file (build_ext.py: -O3 only), so the fp64 divisions are IEEE.
//
// LDS (dynamic), Q = max(K, M), N = min(K, M): the solver 29 Q + 13 N bytes
// (lsap.h; pass A reuses its first 8 K + 8 M bytes for the sums), the truths 20
// M, the rows 20 K, the assignment 4 N, the two lists 2 K + 2 M; pass B adds 8 M
// (a truth's pair: iou and table cell).  At the limits K = 1024, M = 256: pass A
// 62,208 bytes, pass B 64,256, 32 more static (lsap_solve's shared scalars).
//
// Limits: 1 <= M <= 256, 1 <= K <= 1024 (rtdetr_mot_eval's), F <= 65,536, S <=
// 1024 and S * NG * NT <= 2^21 cells: mc is 19 int32 a cell, 152 MiB at the
// bound (pot_q 16 MiB, gas 8 MiB); the caller processes its sequences in groups
// under that budget and scores a single sequence over it on the host.
#include "lsap.h"
#include "moe_common.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace moe {

constexpr int kHotaMaxK = 1024, kHotaMaxM = 256, kHotaMaxF = 65536, kHotaMaxS = 1024, kHotaAlphas = 19;
constexpr long long kHotaMaxCells = 1ll << 21;
constexpr size_t kHotaStaticLds = 32;  // lsap_solve's shared scalars

__host__ __device__ constexpr size_t hota_up16(size_t n) { return (n + 15) & ~(size_t)15; }

struct HotaLds {
  size_t solver, gbox, gidx, tbox, tidx, out, tlist, glist, giou, gcell, total_a, total_b;
  __host__ __device__ HotaLds(int K, int M) {
    const size_t Q = K > M ? K : M, N = K > M ? M : K;
    solver = 0;                                                      // pass A's sums: double [K] + double [M]
    gbox = hota_up16(N * 8 + 2 * Q * 8 + 3 * Q * 4 + N * 4 + N + Q);  // float4 [M]
    gidx = gbox + (size_t)M * 16;                                    // int32 [M]: g, or -1 - g of a flag-0 row
    tbox = gidx + hota_up16((size_t)M * 4);                          // float4 [K]
    tidx = tbox + (size_t)K * 16;                                    // int32 [K]: t, or -1 - t once removed
    out = tidx + hota_up16((size_t)K * 4);                           // int32 [N]: the solver's assignment
    tlist = out + hota_up16(N * 4);                                  // uint16 [K]: the remaining rows
    glist = tlist + hota_up16((size_t)K * 2);                        // uint16 [M]: the truths
    total_a = glist + hota_up16((size_t)M * 2);
    giou = total_a;                                                  // float [M]: per truth, its pair's iou or -1
    gcell = giou + hota_up16((size_t)M * 4);                         // int32 [M]: per truth, its pair's g * NT + t
    total_b = gcell + hota_up16((size_t)M * 4);
  }
};

__device__ __forceinline__ float hota_area(float4 b) { return fmaxf(b.z - b.x, 0.f) * fmaxf(b.w - b.y, 0.f); }

// track.py's rule 3 (track._iou), tracker box first: moteval.hip's mot_iou
__device__ __forceinline__ float hota_iou(float4 t, float4 g) {
  const float iw = fmaxf(fminf(t.z, g.z) - fmaxf(t.x, g.x), 0.f);
  const float ih = fmaxf(fminf(t.w, g.w) - fmaxf(t.y, g.y), 0.f);
  const float inter = iw * ih;
  const float den = (hota_area(t) + hota_area(g)) - inter;
  return den > 0.f ? __fdiv_rn(inter, den) : 0.f;
}

// The solver's cost, from the boxes.  gas == nullptr: the ignore-region solve over all rows (cost iou >= thr ?
// -iou : 0); else pass B's over the listed rows: -(gas[g][t] * iou).  One functor, one lsap_solve per kernel.
struct HotaCost {
  const float4* gbox;
  const float4* tbox;
  const int32_t* gidx;
  const int32_t* tidx;
  const uint16_t* glist;
  const uint16_t* tlist;
  const float* gas;  // the slot's [NG][NT]
  int NT;
  float thr;
  bool trk_q;
  __device__ __forceinline__ float operator()(int q, int m) const {
    int t = trk_q ? q : m, g = trk_q ? m : q;
    if (gas == nullptr) {
      const float iou = hota_iou(tbox[t], gbox[g]);
      return iou >= thr ? -iou : 0.f;
    }
    t = tlist[t];
    g = glist[g];
    const float score = gas[(size_t)gidx[g] * NT + tidx[t]] * hota_iou(tbox[t], gbox[g]);
    return -score;
  }
};

struct HotaRows {
  float4* gbox;
  int32_t* gidx;
  float4* tbox;
  int32_t* tidx;
  uint16_t* tlist;
  uint16_t* glist;
};

// Step 1: the frame's rows into LDS.  -> false (block-uniform) if an index is outside its range; any_ign: the
// frame has a flag-0 row.  Ends with a barrier.
__device__ __forceinline__ bool hota_load(const HotaRows& r, const float* gt_boxes, const int32_t* gt_idx,
                                          const int32_t* gt_flag, const float* trk_boxes, const int32_t* trk_idx,
                                          const uint8_t* keep, int f, int M, int K, int ng, int nt, int NG, int NT,
                                          bool* any_ign) {
  const int lane = threadIdx.x;
  const float4* gb = reinterpret_cast<const float4*>(gt_boxes) + (size_t)f * M;
  const float4* tb = reinterpret_cast<const float4*>(trk_boxes) + (size_t)f * K;
  bool bad = false, ign = false;
  for (int i = lane; i < ng; i += 64) {
    const int gi = gt_idx[(size_t)f * M + i];
    const bool scored = gt_flag[(size_t)f * M + i] != 0, ok = gi >= 0 && gi < NG;
    bad |= !ok;
    ign |= !scored;
    r.gbox[i] = gb[i];
    r.gidx[i] = !ok ? 0 : (scored ? gi : -1 - gi);
  }
  for (int i = lane; i < nt; i += 64) {
    const int ti = trk_idx[(size_t)f * K + i];
    const bool ok = ti >= 0 && ti < NT;
    bad |= !ok;
    r.tbox[i] = tb[i];
    r.tidx[i] = !ok ? 0 : (keep == nullptr || keep[(size_t)f * K + i] != 0 ? ti : -1 - ti);
  }
  const bool any_bad = __ballot(bad) != 0ull;
  *any_ign = __ballot(ign) != 0ull;
  __syncthreads();
  return !any_bad;
}

// The truths and the remaining rows, listed in row order.  Ends with a barrier.
__device__ __forceinline__ void hota_lists(const HotaRows& r, int ng, int nt, int* ngs_out, int* nts_out) {
  const int lane = threadIdx.x;
  int ngs = 0, nts = 0;
  for (int base = 0; base < ng; base += 64) {
    const int i = base + lane;
    const bool keep = i < ng && r.gidx[i] >= 0;
    const unsigned long long bal = __ballot(keep);
    if (keep) r.glist[ngs + mbcnt(bal)] = (uint16_t)i;
    ngs += __popcll(bal);
  }
  for (int base = 0; base < nt; base += 64) {
    const int i = base + lane;
    const bool keep = i < nt && r.tidx[i] >= 0;
    const unsigned long long bal = __ballot(keep);
    if (keep) r.tlist[nts + mbcnt(bal)] = (uint16_t)i;
    nts += __popcll(bal);
  }
  __syncthreads();
  *ngs_out = ngs;
  *nts_out = nts;
}

__global__ __launch_bounds__(64) void hota_pass_a_kernel(
    const float* __restrict__ gt_boxes, const int32_t* __restrict__ gt_idx, const int32_t* __restrict__ gt_flag,
    const int32_t* __restrict__ n_gt, const float* __restrict__ trk_boxes, const int32_t* __restrict__ trk_idx,
    const int32_t* __restrict__ n_trk, const int32_t* __restrict__ frame_slot, int F, int M, int K, int S, int NG,
    int NT, float thr, unsigned long long* __restrict__ pot_q, int32_t* __restrict__ gt_count,
    int32_t* __restrict__ trk_count, uint8_t* __restrict__ keep, int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const HotaLds o(K, M);
  char* solver = smem + o.solver;
  const HotaRows r{reinterpret_cast<float4*>(smem + o.gbox),    reinterpret_cast<int32_t*>(smem + o.gidx),
                   reinterpret_cast<float4*>(smem + o.tbox),    reinterpret_cast<int32_t*>(smem + o.tidx),
                   reinterpret_cast<uint16_t*>(smem + o.tlist), reinterpret_cast<uint16_t*>(smem + o.glist)};
  int32_t* out = reinterpret_cast<int32_t*>(smem + o.out);

  const int f = blockIdx.x, lane = threadIdx.x;
  const int s = frame_slot[f];
  if (s < 0 || s >= S) return;  // block-uniform: the frame is skipped
  const int ng = min(max(n_gt[f], 0), M), nt = min(max(n_trk[f], 0), K);
  bool any_ign;
  if (!hota_load(r, gt_boxes, gt_idx, gt_flag, trk_boxes, trk_idx, nullptr, f, M, K, ng, nt, NG, NT, &any_ign)) {
    if (lane == 0) atomicExch(status, 4);  // an index outside the state: the frame is left out, the call fails
    return;
  }
  // ignore regions (moteval.hip's step 2)
  if (any_ign && nt > 0) {
    const bool tq = nt >= ng;
    const int n = tq ? ng : nt;
    lsap_solve(HotaCost{r.gbox, r.tbox, r.gidx, r.tidx, r.glist, r.tlist, nullptr, NT, thr, tq}, n, tq ? nt : ng, n,
               out, status, solver);
    __syncthreads();
    for (int m = lane; m < n; m += 64) {
      const int q = out[m];
      if (q < 0) continue;
      const int t = tq ? q : m, g = tq ? m : q;
      if (r.gidx[g] < 0 && hota_iou(r.tbox[t], r.gbox[g]) >= thr) r.tidx[t] = -1 - r.tidx[t];
    }
    __syncthreads();
  }
  for (int i = lane; i < nt; i += 64) keep[(size_t)f * K + i] = r.tidx[i] >= 0 ? 1 : 0;
  int ngs, nts;
  hota_lists(r, ng, nt, &ngs, &nts);  // its barrier also ends the solver's use of its arrays

  // the sums, in the rule's order: a lane owns a row (a truth) and walks the truths (the rows)
  double* rowsum = reinterpret_cast<double*>(solver);  // [nts]
  double* colsum = rowsum + K;                         // [ngs]
  for (int q = lane; q < nts; q += 64) {
    const float4 tb = r.tbox[r.tlist[q]];
    double acc = 0.0;
    for (int j = 0; j < ngs; ++j) acc = acc + (double)hota_iou(tb, r.gbox[r.glist[j]]);
    rowsum[q] = acc;
  }
  for (int j = lane; j < ngs; j += 64) {
    const float4 gb = r.gbox[r.glist[j]];
    double acc = 0.0;
    for (int q = 0; q < nts; ++q) acc = acc + (double)hota_iou(r.tbox[r.tlist[q]], gb);
    colsum[j] = acc;
    atomicAdd(gt_count + (size_t)s * NG + r.gidx[r.glist[j]], 1);
  }
  for (int q = lane; q < nts; q += 64) atomicAdd(trk_count + (size_t)s * NT + r.tidx[r.tlist[q]], 1);
  __syncthreads();
  unsigned long long* pot = pot_q + (size_t)s * NG * NT;
  const int pairs = ngs * nts;
  for (int p = lane; p < pairs; p += 64) {
    const int j = p / nts, q = p - j * nts;
    const int g = r.glist[j], t = r.tlist[q];
    const double sim = (double)hota_iou(r.tbox[t], r.gbox[g]);
    const double den = (rowsum[q] + colsum[j]) - sim;
    if (!(den > 2.220446049250313e-16)) continue;  // np.finfo(float).eps
    const long long term = __double2ll_rn(__ddiv_rn(sim, den) * 4294967296.0);
    if (term != 0) atomicAdd(pot + (size_t)r.gidx[g] * NT + r.tidx[t], (unsigned long long)term);
  }
}

__global__ __launch_bounds__(256) void hota_gas_kernel(const long long* __restrict__ pot_q,
                                                       const int32_t* __restrict__ gt_count,
                                                       const int32_t* __restrict__ trk_count, long long cells, int NG,
                                                       int NT, float* __restrict__ gas) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  const long long per = (long long)NG * NT;
  const long long s = i / per, c = i - s * per;
  const int g = (int)(c / NT), t = (int)(c - (long long)g * NT);
  const long long p = pot_q[i];
  const long long n = (long long)gt_count[s * NG + g] + (long long)trk_count[s * NT + t];
  const long long den = n * 4294967296ll - p;
  gas[i] = p != 0 ? __double2float_rn(__ddiv_rn(__ll2double_rn(p), __ll2double_rn(den))) : 0.f;
}

__global__ __launch_bounds__(64) void hota_pass_b_kernel(
    const float* __restrict__ gt_boxes, const int32_t* __restrict__ gt_idx, const int32_t* __restrict__ gt_flag,
    const int32_t* __restrict__ n_gt, const float* __restrict__ trk_boxes, const int32_t* __restrict__ trk_idx,
    const int32_t* __restrict__ n_trk, const int32_t* __restrict__ frame_slot, const uint8_t* __restrict__ keep, int F,
    int M, int K, int S, int NG, int NT, const float* __restrict__ gas, const double* __restrict__ alpha,
    unsigned long long* __restrict__ counts, int32_t* __restrict__ mc, double* __restrict__ loc_part,
    int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const HotaLds o(K, M);
  char* solver = smem + o.solver;
  const HotaRows r{reinterpret_cast<float4*>(smem + o.gbox),    reinterpret_cast<int32_t*>(smem + o.gidx),
                   reinterpret_cast<float4*>(smem + o.tbox),    reinterpret_cast<int32_t*>(smem + o.tidx),
                   reinterpret_cast<uint16_t*>(smem + o.tlist), reinterpret_cast<uint16_t*>(smem + o.glist)};
  int32_t* out = reinterpret_cast<int32_t*>(smem + o.out);
  float* giou = reinterpret_cast<float*>(smem + o.giou);
  int32_t* gcell = reinterpret_cast<int32_t*>(smem + o.gcell);

  const int f = blockIdx.x, lane = threadIdx.x;
  if (lane < kHotaAlphas) loc_part[(size_t)f * kHotaAlphas + lane] = 0.0;  // every element is written
  const int s = frame_slot[f];
  if (s < 0 || s >= S) return;
  const int ng = min(max(n_gt[f], 0), M), nt = min(max(n_trk[f], 0), K);
  bool any_ign;
  if (!hota_load(r, gt_boxes, gt_idx, gt_flag, trk_boxes, trk_idx, keep, f, M, K, ng, nt, NG, NT, &any_ign)) {
    if (lane == 0) atomicExch(status, 4);
    return;
  }
  int ngs, nts;
  hota_lists(r, ng, nt, &ngs, &nts);
  for (int j = lane; j < ngs; j += 64) {
    giou[j] = -1.f;
    gcell[j] = 0;
  }
  __syncthreads();
  if (ngs > 0 && nts > 0) {
    const bool tq = nts >= ngs;
    const int n = tq ? ngs : nts;
    lsap_solve(HotaCost{r.gbox, r.tbox, r.gidx, r.tidx, r.glist, r.tlist, gas + (size_t)s * NG * NT, NT, 0.f, tq}, n,
               tq ? nts : ngs, n, out, status, solver);
    __syncthreads();
    for (int m = lane; m < n; m += 64) {
      const int q = out[m];
      if (q < 0) continue;
      const int tp = tq ? q : m, gp = tq ? m : q;
      const int t = r.tlist[tp], g = r.glist[gp];
      giou[gp] = hota_iou(r.tbox[t], r.gbox[g]);
      gcell[gp] = r.gidx[g] * NT + r.tidx[t];
    }
    __syncthreads();
  }
  // per threshold: the counted pairs by ballot, mc per counted pair
  int32_t* mcs = mc + (size_t)s * kHotaAlphas * NG * NT;
  unsigned long long* cs = counts + (size_t)s * 3 * kHotaAlphas;
  for (int a = 0; a < kHotaAlphas; ++a) {
    const double al = alpha[a];
    int tp = 0;
    for (int base = 0; base < ngs; base += 64) {
      const int j = base + lane;
      const bool hit = j < ngs && (double)giou[j] >= al;
      tp += __popcll(__ballot(hit));
      if (hit) atomicAdd(mcs + (size_t)a * NG * NT + gcell[j], 1);
    }
    if (lane == 0) {
      if (tp) atomicAdd(cs + a, (unsigned long long)tp);
      if (ngs - tp) atomicAdd(cs + kHotaAlphas + a, (unsigned long long)(ngs - tp));
      if (nts - tp) atomicAdd(cs + 2 * kHotaAlphas + a, (unsigned long long)(nts - tp));
    }
  }
  // the loc partials: lane a walks the truths in row order
  if (lane < kHotaAlphas) {
    const double al = alpha[lane];
    double acc = 0.0;
    for (int j = 0; j < ngs; ++j) {
      const double io = (double)giou[j];
      if (io >= al) acc = acc + io;
    }
    loc_part[(size_t)f * kHotaAlphas + lane] = acc;
  }
}

static int hota_check_common(const std::string& what, int F, int M, int K, int S, int NG, int NT) {
  if (F < 0 || F > kHotaMaxF || M < 1 || M > kHotaMaxM || K < 1 || K > kHotaMaxK || S < 0 || S > kHotaMaxS || NG < 1 ||
      NT < 1)
    return fail(what + ": need 0 <= F <= 65536, 1 <= M <= 256, 1 <= K <= 1024, 0 <= S <= 1024, NG >= 1, NT >= 1");
  if ((long long)(S > 0 ? S : 1) * NG * NT > kHotaMaxCells)
    return fail(what + ": the tables exceed the budget: need S * NG * NT <= 2097152 cells");
  return 0;
}

}  // namespace moe

using namespace moe;

extern "C" int rtdetr_hota_pass_a(const float* gt_boxes, const int32_t* gt_idx, const int32_t* gt_flag,
                                  const int32_t* n_gt, const float* trk_boxes, const int32_t* trk_idx,
                                  const int32_t* n_trk, const int32_t* frame_slot, int F, int M, int K, int S, int NG,
                                  int NT, float thr, int64_t* pot_q, int32_t* gt_count, int32_t* trk_count,
                                  uint8_t* keep, int32_t* status, hipStream_t stream) {
  const std::string what = "rtdetr_hota_pass_a";
  if (int rc = hota_check_common(what, F, M, K, S, NG, NT)) return rc;
  if (!(thr > 0.f && thr <= 1.f)) return fail(what + ": thr must be in (0, 1]");
  if (F == 0) return 0;
  if (S < 1) return fail(what + ": need S >= 1 state slots with F > 0");
  if (!gt_boxes || !gt_idx || !gt_flag || !n_gt || !trk_boxes || !trk_idx || !n_trk || !frame_slot)
    return fail(what + ": NULL input pointer");
  if (!pot_q || !gt_count || !trk_count || !keep || !status) return fail(what + ": NULL state pointer");
  if ((reinterpret_cast<uintptr_t>(gt_boxes) | reinterpret_cast<uintptr_t>(trk_boxes)) & 15)
    return fail(what + ": gt_boxes and trk_boxes must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(pot_q) & 7) return fail(what + ": pot_q must be 8-byte aligned");
  const size_t shmem = HotaLds(K, M).total_a;
  if (shmem + kHotaStaticLds > 64 * 1024) return fail(what + ": K / M too large for LDS");
  ProfScope prof(stream, PROF_EVAL, (double)F * (M * 24.0 + K * 21.0 + 12.0));
  MOE_LAUNCH(prof, hota_pass_a_kernel, dim3(F), dim3(64), shmem, stream, gt_boxes, gt_idx, gt_flag, n_gt, trk_boxes,
             trk_idx, n_trk, frame_slot, F, M, K, S, NG, NT, thr, reinterpret_cast<unsigned long long*>(pot_q),
             gt_count, trk_count, keep, status);
  return check_launch(what.c_str());
}

extern "C" int rtdetr_hota_gas(const int64_t* pot_q, const int32_t* gt_count, const int32_t* trk_count, int S, int NG,
                               int NT, float* gas, hipStream_t stream) {
  const std::string what = "rtdetr_hota_gas";
  if (int rc = hota_check_common(what, 0, 1, 1, S, NG, NT)) return rc;
  if (S == 0) return 0;
  if (!pot_q || !gt_count || !trk_count || !gas) return fail(what + ": NULL pointer");
  if (reinterpret_cast<uintptr_t>(pot_q) & 7) return fail(what + ": pot_q must be 8-byte aligned");
  const long long cells = (long long)S * NG * NT;
  ProfScope prof(stream, PROF_EVAL, (double)cells * 12.0 + (double)S * (NG + NT) * 4.0);
  MOE_LAUNCH(prof, hota_gas_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream,
             reinterpret_cast<const long long*>(pot_q), gt_count, trk_count, cells, NG, NT, gas);
  return check_launch(what.c_str());
}

extern "C" int rtdetr_hota_pass_b(const float* gt_boxes, const int32_t* gt_idx, const int32_t* gt_flag,
                                  const int32_t* n_gt, const float* trk_boxes, const int32_t* trk_idx,
                                  const int32_t* n_trk, const int32_t* frame_slot, const uint8_t* keep, int F, int M,
                                  int K, int S, int NG, int NT, const float* gas, const double* alpha,
                                  int64_t* counts, int32_t* mc, double* loc_part, int32_t* status,
                                  hipStream_t stream) {
  const std::string what = "rtdetr_hota_pass_b";
  if (int rc = hota_check_common(what, F, M, K, S, NG, NT)) return rc;
  if (F == 0) return 0;
  if (S < 1) return fail(what + ": need S >= 1 state slots with F > 0");
  if (!gt_boxes || !gt_idx || !gt_flag || !n_gt || !trk_boxes || !trk_idx || !n_trk || !frame_slot || !keep)
    return fail(what + ": NULL input pointer");
  if (!gas || !alpha || !counts || !mc || !loc_part || !status) return fail(what + ": NULL state pointer");
  if ((reinterpret_cast<uintptr_t>(gt_boxes) | reinterpret_cast<uintptr_t>(trk_boxes)) & 15)
    return fail(what + ": gt_boxes and trk_boxes must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(alpha) | reinterpret_cast<uintptr_t>(counts) |
       reinterpret_cast<uintptr_t>(loc_part)) & 7)
    return fail(what + ": alpha, counts and loc_part must be 8-byte aligned");
  const size_t shmem = HotaLds(K, M).total_b;
  if (shmem + kHotaStaticLds > 64 * 1024) return fail(what + ": K / M too large for LDS");
  ProfScope prof(stream, PROF_EVAL, (double)F * (M * 24.0 + K * 21.0 + 12.0 + 8.0 * kHotaAlphas));
  MOE_LAUNCH(prof, hota_pass_b_kernel, dim3(F), dim3(64), shmem, stream, gt_boxes, gt_idx, gt_flag, n_gt, trk_boxes,
             trk_idx, n_trk, frame_slot, keep, F, M, K, S, NG, NT, gas, alpha,
             reinterpret_cast<unsigned long long*>(counts), mc, loc_part, status);
  return check_launch(what.c_str());
}
