// Tracking evaluation on the GPU (moteval.py: mot_reference, which
// moteval.evaluate runs on the host with MOE_TRACK_EVAL=0): the CLEAR-MOT
// counts and the identity table of a tracker's rows against ground truth.
//
// One 64-lane workgroup per state slot (a sequence).  The workgroup reads
// frame_slot[] front to back and handles its own frames in frame order -- the
// matching of a frame prefers the pairs of the frame before, so the frames of
// a sequence are serial by the rule; the parallelism is across sequences and,
// inside a frame, across the solver's column scans.  This kernel is latency
// bound by construction.  Per frame:
//   1. The rows go into LDS: boxes, dense indices (a flag-0 row's index g kept
//      as -1 - g) and every scored row's prev_step entry.
//   2. In a frame with a flag-0 row: lsap_solve of all tracker rows against all
//      ground-truth rows, cost iou >= thr ? -iou : 0 evaluated from the boxes
//      on the fly; a tracker row assigned to a flag-0 row at iou >= thr is
//      marked removed (its index t kept as -1 - t).
//   3. The scored rows and the remaining tracker rows are listed in row order
//      (ballots) and lsap_solve runs on them, cost -(iou, or 1000 + iou where
//      prev_step[g] == t, or 0 below thr), again from the boxes.  Both solves
//      put the side with more rows first, tracker rows on a tie.
//   4. prev_step is cleared (-1, or -2: absent since a matched frame); then a
//      lane per scored row updates per_gt, gt_count, last_ever and prev_step
//      and the wave counts matches and switches with ballots; every lane adds
//      the matched pairs' iou to the fp64 sum in row order (the same adds in
//      every lane; lane 0 stores it); a lane per remaining tracker row counts
//      trk_count, a lane per pair of rows with iou >= thr counts pmc -- plain
//      loads and stores: the workgroup owns its slot and an index is unique in
//      a frame.  No atomics on the state, no workspace.
// The state stays in HBM (L2) between frames, ordered by the barriers; the six
// counts and the sum live in registers from a slot's first frame to its last.
//
// IoU and scores are mot_reference's bit for bit: fp32, each operation rounded
// on its own, no FMA contraction (pragma below), one correctly rounded division.
//
// LDS (dynamic, every array's offset a multiple of 16), Q = max(K, M), N =
// min(K, M): the solver 29 Q + 13 N bytes (lsap.h), the ground-truth rows 32 M,
// the tracker rows 20 K, the assignment 4 N, the two lists 2 K + 2 M;
// lsap_solve's shared scalars add 32 static bytes.
// At the limits K = 1024, M = 256: 33,024 + 8,192 + 20,480 + 1,024 + 2,560 =
// 65,280 bytes, 65,312 with the static ones: 63.8 KiB of the 64.
#include "lsap.h"
#include "moe_common.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace moe {

constexpr int kMotMaxK = 1024, kMotMaxM = 256, kMotMaxNG = 1024, kMotMaxNT = 4096, kMotMaxF = 1024, kMotMaxS = 1024;
constexpr size_t kMotStaticLds = 32;  // lsap_solve's shared scalars

__host__ __device__ constexpr size_t mot_up16(size_t n) { return (n + 15) & ~(size_t)15; }

struct MotLds {
  size_t solver, gbox, gidx, gprev, giou, gmt, tbox, tidx, out, tlist, glist, total;
  __host__ __device__ MotLds(int K, int M) {
    const size_t Q = K > M ? K : M, N = K > M ? M : K;
    solver = 0;
    gbox = mot_up16(N * 8 + 2 * Q * 8 + 3 * Q * 4 + N * 4 + N + Q);  // float4 [M]
    gidx = gbox + (size_t)M * 16;                                    // int32 [M]: g, or -1 - g of a flag-0 row
    gprev = gidx + mot_up16((size_t)M * 4);                          // int32 [M]: prev_step[g] as the frame found it
    giou = gprev + mot_up16((size_t)M * 4);                          // float [M]: per scored row, its match's iou or 0
    gmt = giou + mot_up16((size_t)M * 4);                            // int32 [M]: per scored row, its match's t
    tbox = gmt + mot_up16((size_t)M * 4);                            // float4 [K]
    tidx = tbox + (size_t)K * 16;                                    // int32 [K]: t, or -1 - t once removed
    out = tidx + mot_up16((size_t)K * 4);                            // int32 [N]: the solver's assignment
    tlist = out + mot_up16(N * 4);                                   // uint16 [K]: the remaining tracker rows
    glist = tlist + mot_up16((size_t)K * 2);                         // uint16 [M]: the scored rows
    total = glist + mot_up16((size_t)M * 2);
  }
};

__device__ __forceinline__ float mot_area(float4 b) { return fmaxf(b.z - b.x, 0.f) * fmaxf(b.w - b.y, 0.f); }

// track.py's rule 3 (track._iou), tracker box first
__device__ __forceinline__ float mot_iou(float4 t, float4 g) {
  const float iw = fmaxf(fminf(t.z, g.z) - fmaxf(t.x, g.x), 0.f);
  const float ih = fmaxf(fminf(t.w, g.w) - fmaxf(t.y, g.y), 0.f);
  const float inter = iw * ih;
  const float den = (mot_area(t) + mot_area(g)) - inter;
  return den > 0.f ? __fdiv_rn(inter, den) : 0.f;
}

// The solver's cost, from the boxes.  clear false: step 2 over all rows; true: step 3 over the listed rows.
// trk_q: the tracker rows are the solver's queries.  One functor, so that lsap_solve is instantiated once.
struct MotCost {
  const float4* gbox;
  const float4* tbox;
  const int32_t* gprev;
  const int32_t* tidx;
  const uint16_t* glist;
  const uint16_t* tlist;
  float thr;
  bool trk_q, clear;
  __device__ __forceinline__ float operator()(int q, int m) const {
    int t = trk_q ? q : m, g = trk_q ? m : q;
    if (!clear) {
      const float iou = mot_iou(tbox[t], gbox[g]);
      return iou >= thr ? -iou : 0.f;
    }
    t = tlist[t];
    g = glist[g];
    const float iou = mot_iou(tbox[t], gbox[g]);
    if (!(iou >= thr)) return -0.f;
    return -(gprev[g] == tidx[t] ? 1000.f + iou : iou);
  }
};

struct MotState {
  int32_t* prev_step;  // [S][NG]
  int32_t* last_ever;  // [S][NG]
  int32_t* per_gt;     // [S][NG][3]
  long long* counts;   // [S][8]
  double* motp_sum;    // [S]
  int32_t* pmc;        // [S][NG][NT]
  int32_t* gt_count;   // [S][NG]
  int32_t* trk_count;  // [S][NT]
};

__global__ __launch_bounds__(64) void mot_eval_kernel(
    const float* __restrict__ gt_boxes, const int32_t* __restrict__ gt_idx, const int32_t* __restrict__ gt_flag,
    const int32_t* __restrict__ n_gt, const float* __restrict__ trk_boxes, const int32_t* __restrict__ trk_idx,
    const int32_t* __restrict__ n_trk, const int32_t* __restrict__ frame_slot,
    const int32_t* __restrict__ frame_reset, int F, int M, int K, int S, int NG, int NT, float thr, MotState st,
    int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const MotLds o(K, M);
  char* solver = smem + o.solver;
  float4* gbox = reinterpret_cast<float4*>(smem + o.gbox);
  int32_t* gidx = reinterpret_cast<int32_t*>(smem + o.gidx);
  int32_t* gprev = reinterpret_cast<int32_t*>(smem + o.gprev);
  float* giou = reinterpret_cast<float*>(smem + o.giou);
  int32_t* gmt = reinterpret_cast<int32_t*>(smem + o.gmt);
  float4* tbox = reinterpret_cast<float4*>(smem + o.tbox);
  int32_t* tidx = reinterpret_cast<int32_t*>(smem + o.tidx);
  int32_t* out = reinterpret_cast<int32_t*>(smem + o.out);
  uint16_t* tlist = reinterpret_cast<uint16_t*>(smem + o.tlist);
  uint16_t* glist = reinterpret_cast<uint16_t*>(smem + o.glist);

  const int s = blockIdx.x, lane = threadIdx.x;
  int32_t* prev = st.prev_step + (size_t)s * NG;
  int32_t* last = st.last_ever + (size_t)s * NG;
  int32_t* per = st.per_gt + (size_t)s * NG * 3;
  int32_t* pmc = st.pmc + (size_t)s * NG * NT;
  int32_t* gcount = st.gt_count + (size_t)s * NG;
  int32_t* tcount = st.trk_count + (size_t)s * NT;
  long long c_tp = 0, c_fn = 0, c_fp = 0, c_sw = 0, c_rm = 0, c_fr = 0;  // wave-uniform
  double msum = 0.0;                                                    // the same in every lane
  bool loaded = false;

  for (int f = 0; f < F; ++f) {
    if (frame_slot[f] != s) continue;  // block-uniform
    if (frame_reset[f] != 0) {
      for (int g = lane; g < NG; g += 64) {
        prev[g] = -1;
        last[g] = -1;
        per[3 * g] = 0;
        per[3 * g + 1] = 0;
        per[3 * g + 2] = 0;
        gcount[g] = 0;
      }
      for (int t = lane; t < NT; t += 64) tcount[t] = 0;
      for (size_t i = lane; i < (size_t)NG * NT; i += 64) pmc[i] = 0;
      if (lane < 2) st.counts[(size_t)s * 8 + 6 + lane] = 0;
      c_tp = c_fn = c_fp = c_sw = c_rm = c_fr = 0;
      msum = 0.0;
      loaded = true;
      __syncthreads();
    } else if (!loaded) {
      const long long* c = st.counts + (size_t)s * 8;
      c_tp = c[0], c_fn = c[1], c_fp = c[2], c_sw = c[3], c_rm = c[4], c_fr = c[5];
      msum = st.motp_sum[s];
      loaded = true;
    }

    // 1. the rows
    const int ng = min(max(n_gt[f], 0), M), nt = min(max(n_trk[f], 0), K);
    const float4* gb = reinterpret_cast<const float4*>(gt_boxes) + (size_t)f * M;
    const float4* tb = reinterpret_cast<const float4*>(trk_boxes) + (size_t)f * K;
    bool bad = false, ign = false;
    for (int r = lane; r < ng; r += 64) {
      const int gi = gt_idx[(size_t)f * M + r];
      const bool scored = gt_flag[(size_t)f * M + r] != 0, ok = gi >= 0 && gi < NG;
      bad |= !ok;
      ign |= !scored;
      gbox[r] = gb[r];
      gidx[r] = !ok ? 0 : (scored ? gi : -1 - gi);
      gprev[r] = ok && scored ? prev[gi] : -1;
    }
    for (int r = lane; r < nt; r += 64) {
      const int ti = trk_idx[(size_t)f * K + r];
      const bool ok = ti >= 0 && ti < NT;
      bad |= !ok;
      tbox[r] = tb[r];
      tidx[r] = ok ? ti : 0;
    }
    const bool any_bad = __ballot(bad) != 0ull, any_ign = __ballot(ign) != 0ull;
    __syncthreads();
    if (any_bad) {  // an index outside the state: the frame is left out and the call fails
      if (lane == 0) atomicExch(status, 4);
      continue;
    }

    // 2. ignore regions
    if (any_ign && nt > 0) {
      const bool tq = nt >= ng;
      const int n = tq ? ng : nt;
      lsap_solve(MotCost{gbox, tbox, gprev, tidx, glist, tlist, thr, tq, false}, n, tq ? nt : ng, n, out, status,
                 solver);
      __syncthreads();
      for (int m = lane; m < n; m += 64) {
        const int q = out[m];
        if (q < 0) continue;
        const int t = tq ? q : m, g = tq ? m : q;
        if (gidx[g] < 0 && mot_iou(tbox[t], gbox[g]) >= thr) tidx[t] = -1 - tidx[t];
      }
      __syncthreads();
    }

    // 3. the scored rows, the remaining tracker rows, the CLEAR matching
    int ngs = 0, nts = 0;
    for (int base = 0; base < ng; base += 64) {
      const int r = base + lane;
      const bool keep = r < ng && gidx[r] >= 0;
      const unsigned long long bal = __ballot(keep);
      if (keep) glist[ngs + mbcnt(bal)] = (uint16_t)r;
      ngs += __popcll(bal);
    }
    for (int base = 0; base < nt; base += 64) {
      const int r = base + lane;
      const bool keep = r < nt && tidx[r] >= 0;
      const unsigned long long bal = __ballot(keep);
      if (keep) tlist[nts + mbcnt(bal)] = (uint16_t)r;
      nts += __popcll(bal);
    }
    for (int j = lane; j < ngs; j += 64) {
      giou[j] = 0.f;
      gmt[j] = -1;
    }
    __syncthreads();
    if (ngs > 0 && nts > 0) {
      const bool tq = nts >= ngs;
      const int n = tq ? ngs : nts;
      lsap_solve(MotCost{gbox, tbox, gprev, tidx, glist, tlist, thr, tq, true}, n, tq ? nts : ngs, n, out, status,
                 solver);
      __syncthreads();
      for (int m = lane; m < n; m += 64) {
        const int q = out[m];
        if (q < 0) continue;
        const int tp = tq ? q : m, gp = tq ? m : q;
        const int t = tlist[tp];
        const float iou = mot_iou(tbox[t], gbox[glist[gp]]);
        if (iou >= thr) {  // score > 0
          giou[gp] = iou;
          gmt[gp] = tidx[t];
        }
      }
    }
    // 4. the state.  prev_step: everything is cleared, then the scored rows write theirs
    for (int g = lane; g < NG; g += 64) {
      const int p = prev[g];
      if (p >= 0) prev[g] = -2;
    }
    __syncthreads();
    int nm = 0, nsw = 0;
    for (int base = 0; base < ngs; base += 64) {
      const int j = base + lane;
      bool mt = false, sw = false;
      if (j < ngs) {
        const int g = glist[j];
        const int gi = gidx[g];
        mt = giou[j] > 0.f;
        per[3 * gi] += 1;
        gcount[gi] += 1;
        if (mt) {
          const int t = gmt[j], le = last[gi];
          per[3 * gi + 1] += 1;
          if (gprev[g] == -1) per[3 * gi + 2] += 1;  // not matched in its previous present frame
          sw = le >= 0 && le != t;
          last[gi] = t;
          prev[gi] = t;
        } else {
          prev[gi] = -1;
        }
      }
      nm += __popcll(__ballot(mt));
      nsw += __popcll(__ballot(sw));
    }
    for (int j = 0; j < ngs; ++j) {  // the rule's order: ground-truth row order, one add per pair
      const float io = giou[j];
      if (io > 0.f) msum = msum + (double)io;
    }
    for (int q = lane; q < nts; q += 64) tcount[tidx[tlist[q]]] += 1;
    const int pairs = ngs * nts;
    for (int p = lane; p < pairs; p += 64) {
      const int j = p / nts, q = p - j * nts;
      const int g = glist[j], t = tlist[q];
      if (mot_iou(tbox[t], gbox[g]) >= thr) pmc[(size_t)gidx[g] * NT + tidx[t]] += 1;
    }
    c_tp += nm;
    c_fn += ngs - nm;
    c_fp += nts - nm;
    c_sw += nsw;
    c_rm += nt - nts;
    c_fr += 1;
    __syncthreads();  // the state's stores and the rows in LDS, before the next frame
  }

  if (loaded && lane == 0) {
    long long* c = st.counts + (size_t)s * 8;
    c[0] = c_tp, c[1] = c_fn, c[2] = c_fp, c[3] = c_sw, c[4] = c_rm, c[5] = c_fr;
    st.motp_sum[s] = msum;
  }
}

}  // namespace moe

using namespace moe;

extern "C" int rtdetr_mot_eval(const float* gt_boxes, const int32_t* gt_idx, const int32_t* gt_flag,
                               const int32_t* n_gt, const float* trk_boxes, const int32_t* trk_idx,
                               const int32_t* n_trk, const int32_t* frame_slot, const int32_t* frame_reset, int F,
                               int M, int K, int S, int NG, int NT, float thr, int32_t* prev_step,
                               int32_t* last_ever, int32_t* per_gt, int64_t* counts, double* motp_sum, int32_t* pmc,
                               int32_t* gt_count, int32_t* trk_count, int32_t* status, hipStream_t stream) {
  const std::string what = "rtdetr_mot_eval";
  if (F < 0 || F > kMotMaxF || M < 1 || M > kMotMaxM || K < 1 || K > kMotMaxK || S < 0 || S > kMotMaxS || NG < 1 ||
      NG > kMotMaxNG || NT < 1 || NT > kMotMaxNT)
    return fail(what + ": need 0 <= F <= 1024, 1 <= M <= 256, 1 <= K <= 1024, 0 <= S <= 1024, 1 <= NG <= 1024, "
                       "1 <= NT <= 4096");
  if (!(thr > 0.f && thr <= 1.f)) return fail(what + ": thr must be in (0, 1]");
  if (F == 0) return 0;
  if (S < 1) return fail(what + ": need S >= 1 state slots with F > 0");
  if (!gt_boxes || !gt_idx || !gt_flag || !n_gt || !trk_boxes || !trk_idx || !n_trk)
    return fail(what + ": NULL input pointer");
  if (!frame_slot || !frame_reset) return fail(what + ": NULL frame table");
  if (!prev_step || !last_ever || !per_gt || !counts || !motp_sum || !pmc || !gt_count || !trk_count || !status)
    return fail(what + ": NULL state pointer");
  if ((reinterpret_cast<uintptr_t>(gt_boxes) | reinterpret_cast<uintptr_t>(trk_boxes)) & 15)
    return fail(what + ": gt_boxes and trk_boxes must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(motp_sum)) & 7)
    return fail(what + ": counts and motp_sum must be 8-byte aligned");
  const size_t shmem = MotLds(K, M).total;
  if (shmem + kMotStaticLds > 64 * 1024) return fail(what + ": K / M too large for LDS");
  MotState st{prev_step, last_ever, per_gt, reinterpret_cast<long long*>(counts), motp_sum, pmc, gt_count, trk_count};
  ProfScope prof(stream, PROF_EVAL,
                 (double)F * (M * 24.0 + K * 20.0 + 16.0) + (double)S * (NG * 28.0 + NT * 4.0 + 72.0));
  MOE_LAUNCH(prof, mot_eval_kernel, dim3(S), dim3(64), shmem, stream, gt_boxes, gt_idx, gt_flag, n_gt, trk_boxes,
             trk_idx, n_trk, frame_slot, frame_reset, F, M, K, S, NG, NT, thr, st, status);
  return check_launch(what.c_str());
}
