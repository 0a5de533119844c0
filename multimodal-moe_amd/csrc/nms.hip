// The merge of tiled prediction on the GPU (merge.py: merge_reference, which
// engine.predict runs on the host with MOE_PREDICT_MERGE=0): the detections of
// a frame's passes -- the full frame and its tiles -- hold every object several
// times; a greedy, score-ordered suppression keeps one of each.
//
// One workgroup per image.
//   1. Filter: candidate i takes part if i < n_valid and score >= conf (NaN
//      never does).  The participants are compacted into LDS as 64-bit keys
//      (order-preserving score bits << 32 | ~i): the key carries the index, so
//      the compaction order does not matter (wave ballots + one LDS counter).
//   2. Bitonic sort of the keys in LDS, descending: descending score, equal
//      scores by lower index -- np.argsort(-scores, kind="stable").  -0.0 is
//      keyed as +0.0, which that argsort treats as equal.
//   3. Walk the sorted candidates 64 at a time (one candidate per lane, box,
//      area and label in registers).  Every wave of the workgroup tests the
//      chunk against its share of the kept list (kept j with j % waves == wave:
//      box, area, label in LDS, a broadcast read) and publishes its ballot of
//      suppressed lanes; wave 0 ORs the ballots and resolves the 64 candidates
//      among themselves in order: the first live lane is kept, appended to the
//      kept list and broadcast to the later lanes, which test themselves
//      against it; and so on, at most one round per kept candidate.  The walk
//      stops after max_det kept.  At most N * max_det box tests per image.
//   4. Every output element is written: kept rows, then zeros (-1 in out_src).
//
// The decisions are merge_reference's bit for bit: fp32, each operation rounded
// on its own, no division, no FMA contraction (pragma below): a fused
// (area_i + area_j) - inter flips decisions at the threshold.
//
// LDS (dynamic, every offset a multiple of 16): keys 8 P bytes (P = N rounded
// up to a power of two, <= 32 KiB), kept boxes 16 max_det, areas, labels and
// sources 4 max_det each (<= 28 KiB), 160 bytes of ballots and counters:
// 60.2 KiB at the limits N = 4096, max_det = 1024.
//
// rtdetr_box_fuse (merge.py: fuse_reference; predict(merge="fuse")) is the same
// kernel instantiated with FUSE: the walk and its outputs are the ones above,
// and every kept box (a leader) is then averaged with the copies it suppressed
// that agree with it.
//   3'. In the walk every wave records, per lane, the lowest kept rank of its
//      share that suppresses the lane's candidate (16 bits per (wave, lane) in
//      LDS instead of the ballot); wave 0 takes the minimum over the waves and
//      resolves the chunk as above, handing a lane suppressed inside the chunk
//      the rank of the lane that suppresses it: the first leader in kept order.
//      The lane of a suppressed candidate runs the fuse test against its
//      leader's box (LDS) -- both boxes clamped into the intersection of their
//      passes' windows, then IoU > fuse_thr -- and stores (rank << 1 | verdict)
//      in the high half of its own sort key: the score bits there are not
//      needed once the position is settled.  A kept lane stores its own rank
//      with verdict 1.  ctl[2] counts the visited positions: those up to the
//      max_det-th kept one.
//   4'. One thread per kept row scans the visited positions in order and
//      accumulates its members side by side -- num += score * coord, den +=
//      score, a side cut by a tile window left out -- so the order of the fp32
//      sums is the reference's; then one correctly rounded division per side,
//      the clamp to the frame and the fallback of an unordered axis.
// LDS: 2 KiB of ranks and 1 KiB of windows (P <= 64) more: 63.2 KiB at the limits.
#include "moe_common.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace moe {

constexpr int kNmsMaxN = 4096, kNmsMaxDet = 1024, kNmsMaxB = 1024, kNmsMaxWaves = 16;
constexpr int kFuseMaxP = 64;      // rtdetr_box_fuse's most passes (windows in LDS)
constexpr int kNoLead = 0xFFFF;    // "no kept candidate suppresses this one": above every kept rank (< 1024)

__host__ __device__ constexpr size_t nms_up16(size_t n) { return (n + 15) & ~(size_t)15; }

struct NmsLds {
  size_t keys, kbox, karea, klabel, ksrc, mask, ctl, wrank, win, total;
  __host__ __device__ NmsLds(int P, int max_det, bool fuse = false) {
    keys = 0;                                            // uint64 [P]
    kbox = keys + (size_t)P * 8;                         // float4 [max_det]
    karea = kbox + (size_t)max_det * 16;                 // float [max_det]
    klabel = karea + nms_up16((size_t)max_det * 4);      // int32 [max_det]
    ksrc = klabel + nms_up16((size_t)max_det * 4);       // int32 [max_det]
    mask = ksrc + nms_up16((size_t)max_det * 4);         // uint64 [kNmsMaxWaves]
    ctl = mask + (size_t)kNmsMaxWaves * 8;               // int32 [4]: participants, kept, visited (fuse)
    wrank = ctl + 32;                                    // fuse only: uint16 [kNmsMaxWaves][64]
    win = wrank + (fuse ? (size_t)kNmsMaxWaves * 64 * 2 : 0);  // fuse only: float4 [kFuseMaxP]
    total = win + (fuse ? (size_t)kFuseMaxP * 16 : 0);
  }
};

// what rtdetr_box_fuse's instantiation takes on top of the walk's arguments; empty for the plain kernel
template <bool FUSE>
struct FuseArgs {};
template <>
struct FuseArgs<true> {
  float fuse_thr;
  const float* windows;  // [B][n_pass][4] or nullptr with n_pass == 0
  int n_pass, per_pass;  // candidate i belongs to pass i / per_pass
  int32_t* out_members;  // [B][max_det]
};

__device__ __forceinline__ uint32_t nms_score_key(float f) {
  if (f == 0.f) f = 0.f;  // -0.0 sorts with +0.0
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending uint order = ascending float order
}

__device__ __forceinline__ float nms_area(float4 b) { return fmaxf(b.z - b.x, 0.f) * fmaxf(b.w - b.y, 0.f); }

// whether kept (kb, karea) suppresses candidate (cb, carea): inter > thr * den
__device__ __forceinline__ bool nms_hit(float4 cb, float carea, float4 kb, float karea, float thr, int metric) {
  const float iw = fmaxf(fminf(cb.z, kb.z) - fmaxf(cb.x, kb.x), 0.f);
  const float ih = fmaxf(fminf(cb.w, kb.w) - fmaxf(cb.y, kb.y), 0.f);
  const float inter = iw * ih;
  const float den = metric == 0 ? (carea + karea) - inter : fminf(carea, karea);
  return inter > thr * den;
}

__device__ __forceinline__ float4 nms_clamp(float4 b, float4 lo_hi) {  // into (x0, y0, x1, y1), per coordinate
  return make_float4(fminf(fmaxf(b.x, lo_hi.x), lo_hi.z), fminf(fmaxf(b.y, lo_hi.y), lo_hi.w),
                     fminf(fmaxf(b.z, lo_hi.x), lo_hi.z), fminf(fmaxf(b.w, lo_hi.y), lo_hi.w));
}

// fuse_reference's step 2: candidate box cb of pass window wc against its leader's box kb of pass window wk
__device__ __forceinline__ bool nms_fuses(float4 cb, float4 kb, bool windows, float4 wc, float4 wk, float fuse_thr) {
  if (windows) {
    const float4 v = make_float4(fmaxf(wc.x, wk.x), fmaxf(wc.y, wk.y), fminf(wc.z, wk.z), fminf(wc.w, wk.w));
    cb = nms_clamp(cb, v);
    kb = nms_clamp(kb, v);
  }
  return nms_hit(cb, nms_area(cb), kb, nms_area(kb), fuse_thr, 0);
}

template <bool FUSE>
__global__ __launch_bounds__(1024) void nms_merge_kernel(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ n_valid, int N, int P, float conf, float thr, int metric, int class_agnostic,
    int max_det, float* __restrict__ out_boxes, float* __restrict__ out_scores, int32_t* __restrict__ out_labels,
    int32_t* __restrict__ out_src, int32_t* __restrict__ count, FuseArgs<FUSE> fa) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const NmsLds o(P, max_det, FUSE);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem + o.keys);
  float4* kbox = reinterpret_cast<float4*>(smem + o.kbox);
  float* karea = reinterpret_cast<float*>(smem + o.karea);
  int32_t* klabel = reinterpret_cast<int32_t*>(smem + o.klabel);
  int32_t* ksrc = reinterpret_cast<int32_t*>(smem + o.ksrc);
  unsigned long long* wmask = reinterpret_cast<unsigned long long*>(smem + o.mask);
  int32_t* ctl = reinterpret_cast<int32_t*>(smem + o.ctl);

  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nwaves = nthr >> 6;
  const int n = n_valid != nullptr ? min(max(n_valid[b], 0), N) : N;
  const float* sc = scores + (size_t)b * N;
  const float4* bx = reinterpret_cast<const float4*>(boxes) + (size_t)b * N;
  const int32_t* lb = labels + (size_t)b * N;

  if (tid == 0) {
    ctl[0] = 0;
    ctl[1] = 0;
    ctl[2] = 0;
  }
  [[maybe_unused]] uint16_t* wrank = reinterpret_cast<uint16_t*>(smem + o.wrank);
  [[maybe_unused]] float4* win = reinterpret_cast<float4*>(smem + o.win);
  if constexpr (FUSE) {
    if (tid < fa.n_pass) win[tid] = reinterpret_cast<const float4*>(fa.windows)[(size_t)b * fa.n_pass + tid];
  }
  __syncthreads();

  // 1. filter + compaction (any order: the key holds the index)
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int base = 0; base < n; base += nthr) {  // block-uniform bound: every lane of a wave reaches the ballot
    const int i = base + tid;
    const float s = i < n ? sc[i] : 0.f;
    const bool part = i < n && s >= conf;  // false for NaN
    const unsigned long long bal = __ballot(part);
    int slot0 = 0;
    if (lane == 0 && bal != 0ull) slot0 = atomicAdd(&ctl[0], __popcll(bal));
    slot0 = __shfl(slot0, 0, 64);
    if (part)
      keys[slot0 + __popcll(bal & below)] = ((unsigned long long)nms_score_key(s) << 32) | (uint32_t)~(uint32_t)i;
  }
  __syncthreads();
  const int M = ctl[0];  // participants, <= n <= N <= P

  // 2. bitonic sort of the M keys, descending (padded with 0: below every real key, whose score half is > 0)
  int Ps = 1;
  while (Ps < M) Ps <<= 1;
  for (int s = M + tid; s < Ps; s += nthr) keys[s] = 0ull;
  __syncthreads();
  for (int size = 2; size <= Ps; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < Ps / 2; t += nthr) {
        const int a = 2 * t - (t & (stride - 1)), c = a + stride;
        const bool desc = (a & size) == 0;
        const unsigned long long ka = keys[a], kc = keys[c];
        if ((ka > kc) != desc) {
          keys[a] = kc;
          keys[c] = ka;
        }
      }
      __syncthreads();
    }
  }

  // 3. the walk
  for (int base = 0; base < M; base += 64) {
    const int nk = ctl[1];  // kept so far (written by wave 0 before the last barrier)
    if (nk >= max_det) break;
    const int r = base + lane;
    const bool valid = r < M;
    const int i = valid ? (int)(~(uint32_t)keys[r]) : 0;  // in bounds: N >= 1 whenever M >= 1
    const float4 cb = valid ? bx[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int cl = valid ? lb[i] : 0;
    const float ca = nms_area(cb);
    bool sup = false;
    [[maybe_unused]] int lead = kNoLead;  // fuse: the lowest kept rank that suppresses this lane's candidate
    for (int j = wave; j < nk; j += nwaves) {
      const float4 kb = kbox[j];
      const bool hit = (class_agnostic || klabel[j] == cl) && nms_hit(cb, ca, kb, karea[j], thr, metric);
      if constexpr (FUSE) {
        if (hit && !sup) lead = j;  // j ascends: the first hit is this wave's lowest rank
      }
      sup = sup || hit;
    }
    if constexpr (FUSE) {
      wrank[wave * 64 + lane] = (uint16_t)lead;
    } else {
      const unsigned long long bal = __ballot(sup);
      if (lane == 0) wmask[wave] = bal;
    }
    __syncthreads();
    if (wave == 0) {
      bool alive;
      if constexpr (FUSE) {
        lead = kNoLead;
        for (int w = 0; w < nwaves; ++w) lead = min(lead, (int)wrank[w * 64 + lane]);
        alive = valid && lead == kNoLead;
      } else {
        unsigned long long dead = 0ull;
        for (int w = 0; w < nwaves; ++w) dead |= wmask[w];
        alive = valid && !((dead >> lane) & 1ull);
      }
      int kept = nk;
      [[maybe_unused]] int tlast = 63;  // fuse: the lane of the last candidate kept in this chunk
      unsigned long long rem = __ballot(alive);
      while (rem != 0ull && kept < max_det) {  // wave-uniform
        const int t = __ffsll((long long)rem) - 1;  // the best live candidate of the chunk: kept
        const float4 kb = make_float4(__shfl(cb.x, t, 64), __shfl(cb.y, t, 64), __shfl(cb.z, t, 64),
                                      __shfl(cb.w, t, 64));
        const float ka = __shfl(ca, t, 64);
        const int kl = __shfl(cl, t, 64);
        if (lane == t) {
          kbox[kept] = cb;
          karea[kept] = ca;
          klabel[kept] = cl;
          ksrc[kept] = i;
        }
        if constexpr (FUSE) {
          if (lane == t) lead = kept;  // a leader: its own rank
          tlast = t;
        }
        ++kept;
        if (alive && lane > t && (class_agnostic || kl == cl) && nms_hit(cb, ca, kb, ka, thr, metric)) {
          alive = false;
          if constexpr (FUSE) lead = kept - 1;  // suppressed inside the chunk: no earlier leader did
        }
        const unsigned long long upto = t == 63 ? ~0ull : ((2ull << t) - 1ull);  // lanes <= t are settled
        rem = __ballot(alive) & ~upto;
      }
      if (lane == 0) ctl[1] = kept;
      if constexpr (FUSE) {
        // visited: up to the max_det-th kept candidate (the reference's walk stops there), else the whole chunk
        const bool visited = valid && (kept < max_det || lane <= tlast);
        if (visited) {
          int fuses = 1;
          if (!alive) {  // suppressed by the leader of rank lead, whose box wave 0 wrote (LDS is in order per wave)
            const bool w = fa.n_pass > 0;
            const float4 wc = w ? win[i / fa.per_pass] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 wk = w ? win[ksrc[lead] / fa.per_pass] : make_float4(0.f, 0.f, 0.f, 0.f);
            fuses = nms_fuses(cb, kbox[lead], w, wc, wk, fa.fuse_thr) ? 1 : 0;
          }
          keys[r] = ((unsigned long long)(uint32_t)((lead << 1) | fuses) << 32) | (uint32_t)keys[r];
        }
        const unsigned long long vis = __ballot(visited);  // a prefix of the chunk
        if (lane == 0) ctl[2] = base + __popcll(vis);
      }
    }
    __syncthreads();
  }
  __syncthreads();  // the loop's break leaves before a barrier only where every thread does (ctl[1] is uniform)

  // 4. outputs: every element written
  const int nk = min(ctl[1], max_det);
  float4* ob = reinterpret_cast<float4*>(out_boxes) + (size_t)b * max_det;
  for (int r = tid; r < max_det; r += nthr) {
    const bool k = r < nk;
    const int src = k ? ksrc[r] : -1;
    if constexpr (FUSE) {
      // 4'. this row's members, in visit order (the leader stands first: it precedes all it suppresses)
      float4 fb = make_float4(0.f, 0.f, 0.f, 0.f);
      int members = 0;
      if (k) {
        const float4 lb4 = kbox[r];
        const bool w = fa.n_pass > 0;
        const float4 w0 = w ? win[0] : make_float4(0.f, 0.f, 0.f, 0.f);
        const uint32_t want = ((uint32_t)r << 1) | 1u;
        const int visited = ctl[2];
        float nx1 = 0.f, ny1 = 0.f, nx2 = 0.f, ny2 = 0.f, dx1 = 0.f, dy1 = 0.f, dx2 = 0.f, dy2 = 0.f;
        for (int v = 0; v < visited; ++v) {  // a broadcast read: every thread reads the same word
          const unsigned long long key = keys[v];
          if ((uint32_t)(key >> 32) != want) continue;
          ++members;
          const int i = (int)(~(uint32_t)key);
          const float s = sc[i];
          if (!(s > 0.f && s < INFINITY)) continue;  // contributes nothing: not finite, zero or negative
          const float4 c = bx[i];
          bool u0 = true, u1 = true, u2 = true, u3 = true;  // sides not cut by the candidate's tile window
          const int p = w ? i / fa.per_pass : 0;
          if (p > 0) {
            const float4 wp = win[p];
            u0 = !(c.x <= wp.x && wp.x > w0.x);
            u1 = !(c.y <= wp.y && wp.y > w0.y);
            u2 = !(c.z >= wp.z && wp.z < w0.z);
            u3 = !(c.w >= wp.w && wp.w < w0.w);
          }
          if (u0) { nx1 = nx1 + (s * c.x); dx1 = dx1 + s; }
          if (u1) { ny1 = ny1 + (s * c.y); dy1 = dy1 + s; }
          if (u2) { nx2 = nx2 + (s * c.z); dx2 = dx2 + s; }
          if (u3) { ny2 = ny2 + (s * c.w); dy2 = dy2 + s; }
        }
        fb.x = dx1 > 0.f ? __fdiv_rn(nx1, dx1) : lb4.x;
        fb.y = dy1 > 0.f ? __fdiv_rn(ny1, dy1) : lb4.y;
        fb.z = dx2 > 0.f ? __fdiv_rn(nx2, dx2) : lb4.z;
        fb.w = dy2 > 0.f ? __fdiv_rn(ny2, dy2) : lb4.w;
        if (w) fb = nms_clamp(fb, w0);
        if (fb.x > fb.z) { fb.x = lb4.x; fb.z = lb4.z; }
        if (fb.y > fb.w) { fb.y = lb4.y; fb.w = lb4.w; }
      }
      ob[r] = fb;
      fa.out_members[(size_t)b * max_det + r] = members;
    } else {
      ob[r] = k ? kbox[r] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    out_scores[(size_t)b * max_det + r] = k ? sc[src] : 0.f;
    out_labels[(size_t)b * max_det + r] = k ? klabel[r] : 0;
    out_src[(size_t)b * max_det + r] = src;
  }
  if (tid == 0) count[b] = nk;
}

// the argument checks the two entry points share; 0, or fail() with ``what`` in front
static int nms_check(const std::string& what, int B, int N, float conf, float thr, int metric, int max_det) {
  if (B < 0 || N < 0 || B > kNmsMaxB || N > kNmsMaxN || max_det < 1 || max_det > kNmsMaxDet)
    return fail(what + ": need 0 <= B <= 1024, 0 <= N <= 4096, 1 <= max_det <= 1024");
  if (metric != 0 && metric != 1) return fail(what + ": metric must be 0 (iou) or 1 (ios)");
  if (conf != conf || thr != thr) return fail(what + ": conf and thr must not be NaN");
  return 0;
}

static int nms_check_pointers(const std::string& what, const float* boxes, const float* scores,
                              const int32_t* labels, int N, const float* out_boxes, const float* out_scores,
                              const int32_t* out_labels, const int32_t* out_src, const int32_t* count) {
  if (!out_boxes || !out_scores || !out_labels || !out_src || !count) return fail(what + ": NULL output pointer");
  if (N > 0 && (!boxes || !scores || !labels)) return fail(what + ": NULL input pointer");
  if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(out_boxes)) & 15)
    return fail(what + ": boxes and out_boxes must be 16-byte aligned");
  return 0;
}

}  // namespace moe

using namespace moe;

extern "C" int rtdetr_nms_merge(const float* boxes, const float* scores, const int32_t* labels,
                                const int32_t* n_valid, int B, int N, float conf, float thr, int metric,
                                int class_agnostic, int max_det, float* out_boxes, float* out_scores,
                                int32_t* out_labels, int32_t* out_src, int32_t* count, hipStream_t stream) {
  if (int rc = nms_check("rtdetr_nms_merge", B, N, conf, thr, metric, max_det)) return rc;
  if (B == 0) return 0;
  if (int rc = nms_check_pointers("rtdetr_nms_merge", boxes, scores, labels, N, out_boxes, out_scores, out_labels,
                                  out_src, count))
    return rc;
  int P = 1;
  while (P < N) P <<= 1;
  const size_t shmem = NmsLds(P, max_det).total;
  if (shmem > 64 * 1024) return fail("rtdetr_nms_merge: N / max_det too large for LDS");
  const int threads = N <= 256 ? 256 : 1024;
  ProfScope prof(stream, PROF_MERGE,
                 (double)B * (N * 24.0 + (n_valid ? 4.0 : 0.0) + max_det * 28.0 + 4.0));
  MOE_LAUNCH(prof, (nms_merge_kernel<false>), dim3(B), dim3(threads), shmem, stream, boxes, scores, labels, n_valid,
             N, P, conf, thr, metric, class_agnostic != 0 ? 1 : 0, max_det, out_boxes, out_scores, out_labels,
             out_src, count, FuseArgs<false>{});
  return check_launch("rtdetr_nms_merge");
}

extern "C" int rtdetr_box_fuse(const float* boxes, const float* scores, const int32_t* labels,
                               const int32_t* n_valid, int B, int N, float conf, float thr, int metric,
                               int class_agnostic, int max_det, float fuse_thr, const float* windows, int P,
                               float* out_boxes, float* out_scores, int32_t* out_labels, int32_t* out_src,
                               int32_t* count, int32_t* out_members, hipStream_t stream) {
  if (int rc = nms_check("rtdetr_box_fuse", B, N, conf, thr, metric, max_det)) return rc;
  if (fuse_thr != fuse_thr) return fail("rtdetr_box_fuse: fuse_thr must not be NaN");
  if (P < 0 || P > kFuseMaxP) return fail("rtdetr_box_fuse: need 0 <= P <= 64 passes");
  if (P > 0 && N % P != 0) return fail("rtdetr_box_fuse: N must be a multiple of P (N = P k candidates)");
  if (B == 0) return 0;
  if (P > 0 && !windows) return fail("rtdetr_box_fuse: NULL windows with P > 0");
  if (P > 0 && (reinterpret_cast<uintptr_t>(windows) & 15))
    return fail("rtdetr_box_fuse: windows must be 16-byte aligned");
  if (int rc = nms_check_pointers("rtdetr_box_fuse", boxes, scores, labels, N, out_boxes, out_scores, out_labels,
                                  out_src, count))
    return rc;
  if (!out_members) return fail("rtdetr_box_fuse: NULL output pointer");
  int Pn = 1;
  while (Pn < N) Pn <<= 1;
  const size_t shmem = NmsLds(Pn, max_det, true).total;
  if (shmem > 64 * 1024) return fail("rtdetr_box_fuse: N / max_det too large for LDS");
  const int threads = N <= 256 ? 256 : 1024;
  FuseArgs<true> fa;
  fa.fuse_thr = fuse_thr;
  fa.windows = P > 0 ? windows : nullptr;
  fa.n_pass = P;
  fa.per_pass = P > 0 && N >= P ? N / P : 1;
  fa.out_members = out_members;
  ProfScope prof(stream, PROF_MERGE,
                 (double)B * (N * 24.0 + (n_valid ? 4.0 : 0.0) + P * 16.0 + max_det * 32.0 + 4.0));
  MOE_LAUNCH(prof, (nms_merge_kernel<true>), dim3(B), dim3(threads), shmem, stream, boxes, scores, labels, n_valid,
             N, Pn, conf, thr, metric, class_agnostic != 0 ? 1 : 0, max_det, out_boxes, out_scores, out_labels,
             out_src, count, fa);
  return check_launch("rtdetr_box_fuse");
}

