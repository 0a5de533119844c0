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
#include "moe_common.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace moe {

constexpr int kNmsMaxN = 4096, kNmsMaxDet = 1024, kNmsMaxB = 1024, kNmsMaxWaves = 16;

__host__ __device__ constexpr size_t nms_up16(size_t n) { return (n + 15) & ~(size_t)15; }

struct NmsLds {
  size_t keys, kbox, karea, klabel, ksrc, mask, ctl, total;
  __host__ __device__ NmsLds(int P, int max_det) {
    keys = 0;                                            // uint64 [P]
    kbox = keys + (size_t)P * 8;                         // float4 [max_det]
    karea = kbox + (size_t)max_det * 16;                 // float [max_det]
    klabel = karea + nms_up16((size_t)max_det * 4);      // int32 [max_det]
    ksrc = klabel + nms_up16((size_t)max_det * 4);       // int32 [max_det]
    mask = ksrc + nms_up16((size_t)max_det * 4);         // uint64 [kNmsMaxWaves]
    ctl = mask + (size_t)kNmsMaxWaves * 8;               // int32 [4]: participants, kept, stop
    total = ctl + 32;
  }
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

__global__ __launch_bounds__(1024) void nms_merge_kernel(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ n_valid, int N, int P, float conf, float thr, int metric, int class_agnostic,
    int max_det, float* __restrict__ out_boxes, float* __restrict__ out_scores, int32_t* __restrict__ out_labels,
    int32_t* __restrict__ out_src, int32_t* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const NmsLds o(P, max_det);
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
    for (int j = wave; j < nk; j += nwaves) {
      const float4 kb = kbox[j];
      sup = sup || ((class_agnostic || klabel[j] == cl) && nms_hit(cb, ca, kb, karea[j], thr, metric));
    }
    const unsigned long long bal = __ballot(sup);
    if (lane == 0) wmask[wave] = bal;
    __syncthreads();
    if (wave == 0) {
      unsigned long long dead = 0ull;
      for (int w = 0; w < nwaves; ++w) dead |= wmask[w];
      bool alive = valid && !((dead >> lane) & 1ull);
      int kept = nk;
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
        ++kept;
        if (alive && lane > t && (class_agnostic || kl == cl) && nms_hit(cb, ca, kb, ka, thr, metric)) alive = false;
        const unsigned long long upto = t == 63 ? ~0ull : ((2ull << t) - 1ull);  // lanes <= t are settled
        rem = __ballot(alive) & ~upto;
      }
      if (lane == 0) ctl[1] = kept;
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
    ob[r] = k ? kbox[r] : make_float4(0.f, 0.f, 0.f, 0.f);
    out_scores[(size_t)b * max_det + r] = k ? sc[src] : 0.f;
    out_labels[(size_t)b * max_det + r] = k ? klabel[r] : 0;
    out_src[(size_t)b * max_det + r] = src;
  }
  if (tid == 0) count[b] = nk;
}

}  // namespace moe

using namespace moe;

extern "C" int rtdetr_nms_merge(const float* boxes, const float* scores, const int32_t* labels,
                                const int32_t* n_valid, int B, int N, float conf, float thr, int metric,
                                int class_agnostic, int max_det, float* out_boxes, float* out_scores,
                                int32_t* out_labels, int32_t* out_src, int32_t* count, hipStream_t stream) {
  if (B < 0 || N < 0 || B > kNmsMaxB || N > kNmsMaxN || max_det < 1 || max_det > kNmsMaxDet)
    return fail("rtdetr_nms_merge: need 0 <= B <= 1024, 0 <= N <= 4096, 1 <= max_det <= 1024");
  if (metric != 0 && metric != 1) return fail("rtdetr_nms_merge: metric must be 0 (iou) or 1 (ios)");
  if (conf != conf || thr != thr) return fail("rtdetr_nms_merge: conf and thr must not be NaN");
  if (B == 0) return 0;
  if (!out_boxes || !out_scores || !out_labels || !out_src || !count)
    return fail("rtdetr_nms_merge: NULL output pointer");
  if (N > 0 && (!boxes || !scores || !labels)) return fail("rtdetr_nms_merge: NULL input pointer");
  if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(out_boxes)) & 15)
    return fail("rtdetr_nms_merge: boxes and out_boxes must be 16-byte aligned");
  int P = 1;
  while (P < N) P <<= 1;
  const size_t shmem = NmsLds(P, max_det).total;
  if (shmem > 64 * 1024) return fail("rtdetr_nms_merge: N / max_det too large for LDS");
  const int threads = N <= 256 ? 256 : 1024;
  ProfScope prof(stream, PROF_MERGE,
                 (double)B * (N * 24.0 + (n_valid ? 4.0 : 0.0) + max_det * 28.0 + 4.0));
  MOE_LAUNCH(prof, nms_merge_kernel, dim3(B), dim3(threads), shmem, stream, boxes, scores, labels, n_valid, N, P,
             conf, thr, metric, class_agnostic != 0 ? 1 : 0, max_det, out_boxes, out_scores, out_labels, out_src,
             count);
  return check_launch("rtdetr_nms_merge");
}
