// Detection-to-truth matching of validation on the GPU (metrics.py:
// match_predictions + box_iou_np, which engine._evaluate ran per image on the
// host: 10 IoU thresholds x up to 300 predictions of Python per image).
//
// One workgroup per image, one 64-lane wave per IoU threshold.  The thresholds
// are independent; the predictions of one threshold are a sequential chain
// (a truth taken by a better-scored prediction is gone for the later ones), so
// each wave walks the predictions in np.argsort(-scores, kind="stable") order
// and its lanes stride over the truths: the IoU of (prediction, truth) is
// recomputed per wave -- no [K][M] matrix -- the "taken" set lives in one
// register per lane (lane l owns truths l, l + 64, ...), and the argmax over
// the candidates is a wave butterfly on (iou, lowest j).  Predictions, their
// visit order and the truths are staged once in LDS.  An image with at most 64
// truths -- one per lane, the usual case -- keeps its truth in registers and
// computes the IoUs of four predictions ahead of their four selections: the
// chain is bound by latency, and only the selection depends on its state.
//
// The result is the reference's tp bit for bit, so the arithmetic restates
// numpy's dtypes: intersection, truth area and union in fp64 with the fp32
// prediction coordinates widened exactly; the PREDICTION area in fp32 (the
// reference's np.prod over a float32 array stays float32) and then widened;
// union = (area_a + area_b) - inter; iou = inter / max(union, 1e-9).  No FMA
// contraction anywhere (pragma below): a fused (area_a + area_b) - w h flips
// bits.  The fp64 division is the correctly rounded one.
//
// rtdetr_eval_match_bands is the size-stratified form (the size report of
// validation, metrics.match_predictions_banded): the same workgroup per (image,
// height band), the truths outside the band as ignore regions.  Each lane
// keeps an in-band and an out-of-band best; the in-band set is reduced first
// and the out-of-band one only when the wave found no in-band candidate.  Both
// kernels are one template (eval_match_image), so the staging, the ranks, the
// IoU and the selection are shared.
#include "moe_common.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace moe {

constexpr int kEvalMaxK = 1024, kEvalMaxM = 1024, kEvalMaxT = 16, kEvalMaxR = 8;

__host__ __device__ constexpr size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// LDS carve (every offset a multiple of 16 bytes)
struct EvalLds {
  size_t g, pbox, score, plabel, glabel, order, total;
  __host__ __device__ EvalLds(int K, int M) {
    g = 0;                                    // double [4][Ms]: truth x1 | y1 | x2 | y2
    pbox = g + 4 * up16((size_t)M * 8);       // float4 [K]
    score = pbox + (size_t)K * 16;            // float [K]
    plabel = score + up16((size_t)K * 4);     // int32 [K]
    glabel = plabel + up16((size_t)K * 4);    // int32 [M]
    order = glabel + up16((size_t)M * 4);     // uint16 [K]: order[rank] = prediction
    total = order + up16((size_t)K * 2);
  }
};

// (iou, j) of the better candidate: the larger IoU, the lower j among equals
// (np.argmax over candidates in ascending j); j < 0 = no candidate
__device__ __forceinline__ void better(double& iou, int& j, double o_iou, int o_j) {
  if (o_j >= 0 && (j < 0 || o_iou > iou || (o_iou == iou && o_j < j))) {
    iou = o_iou;
    j = o_j;
  }
}

// box_iou_np of one pair: prediction p (fp32 xyxy), truth (fp64 xyxy)
__device__ __forceinline__ double pair_iou(float4 p, double bx1, double by1, double bx2, double by2) {
  const float area_a32 = fmaxf(p.z - p.x, 0.f) * fmaxf(p.w - p.y, 0.f);  // fp32, as the reference
  const double area_a = (double)area_a32;
  const double ax1 = (double)p.x, ay1 = (double)p.y, ax2 = (double)p.z, ay2 = (double)p.w;
  const double w = fmax(fmin(ax2, bx2) - fmax(ax1, bx1), 0.0);
  const double h = fmax(fmin(ay2, by2) - fmax(ay1, by1), 0.0);
  const double inter = w * h;
  const double area_b = fmax(bx2 - bx1, 0.0) * fmax(by2 - by1, 0.0);
  const double uni = (area_a + area_b) - inter;
  return inter / fmax(uni, 1e-9);
}

// The wave's best candidate out of each lane's (best, best_j); marks it taken
// in its owner lane.  Returns 1 if there was one.  Wave-uniform.
__device__ __forceinline__ int take_best(double best, int best_j, int lane, uint32_t& taken) {
  if (__ballot(best_j >= 0) == 0ull) return 0;  // most predictions have no candidate
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o_iou = __shfl_xor(best, off, 64);
    const int o_j = __shfl_xor(best_j, off, 64);
    better(best, best_j, o_iou, o_j);
  }
  if ((best_j & 63) == lane) taken |= 1u << (best_j >> 6);
  return 1;
}

// lo <= h < hi: membership of a box height in a band (a NaN height is in none)
__device__ __forceinline__ bool in_band(double h, double lo, double hi) { return h >= lo && h < hi; }

// One image of either matcher (blockIdx.x = the image; out = its [K][T] slab).
// kBands = false: metrics.match_predictions, out <- tp (0 / 1).
// kBands = true: metrics.match_predictions_banded for the band [lo, hi) of box
// heights in source pixels (evaluated pixels times scale), out <- 0 false
// positive, 1 true positive, 2 ignored.  Truths outside the band are ignore
// regions: a prediction takes the best in-band candidate (1); only when it has
// none, the best out-of-band candidate (2, and that truth is taken too); with
// no candidate at all it is 0 if its own height is in the band, else 2.  Truth
// heights are fp64, the prediction height is the fp32 difference widened, as
// the reference takes them; each is multiplied by scale in fp64.
template <bool kBands>
__device__ __forceinline__ void eval_match_image(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ labels,
    const double* __restrict__ gt_boxes, const int32_t* __restrict__ gt_labels, const int32_t* __restrict__ n_valid,
    const double* __restrict__ thr, int K, int M, int T, uint8_t* __restrict__ out, double scale, double lo,
    double hi) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const EvalLds o(K, M);
  const int Ms = (int)(up16((size_t)M * 8) / 8);
  double* g = reinterpret_cast<double*>(smem + o.g);
  float* pbox = reinterpret_cast<float*>(smem + o.pbox);
  float* score = reinterpret_cast<float*>(smem + o.score);
  int32_t* plabel = reinterpret_cast<int32_t*>(smem + o.plabel);
  int32_t* glabel = reinterpret_cast<int32_t*>(smem + o.glabel);
  uint16_t* order = reinterpret_cast<uint16_t*>(smem + o.order);

  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int n = min(max(n_valid[b], 0), M);  // padding slots j >= n are never read

  for (int e = tid; e < K * 4; e += nthr) pbox[e] = boxes[(size_t)b * K * 4 + e];
  for (int i = tid; i < K; i += nthr) {
    score[i] = scores[(size_t)b * K + i];
    plabel[i] = labels[(size_t)b * K + i];
  }
  for (int e = tid; e < n * 4; e += nthr) g[(e & 3) * Ms + (e >> 2)] = gt_boxes[(size_t)b * M * 4 + e];
  for (int j = tid; j < n; j += nthr) glabel[j] = gt_labels[(size_t)b * M + j];
  __syncthreads();

  // visit order = np.argsort(-scores, kind="stable"): the rank of prediction i is
  // the count of higher scores plus the count of equal scores at lower indices.
  // NaN scores rank last, as numpy sorts them, so the ranks are a permutation
  // for any input and every order[] slot is written.
  for (int i = tid; i < K; i += nthr) {
    const float s = score[i];
    const bool s_nan = s != s;
    int rank = 0;
    for (int k = 0; k < K; ++k) {
      const float sk = score[k];
      const bool k_nan = sk != sk;
      const bool before = sk > s || (s_nan && !k_nan);
      const bool equal = sk == s || (s_nan && k_nan);
      rank += (before || (equal && k < i)) ? 1 : 0;
    }
    order[rank] = (uint16_t)i;
  }
  __syncthreads();

  const int t = tid >> 6, lane = tid & 63;  // wave t: threshold t
  const double th = thr[t];
  uint32_t taken = 0;  // bit jj: truth lane + 64 jj is taken (M <= 1024: 16 bits)
  uint8_t* tpb = out + t;
  if (n <= 64) {
    // One truth per lane, kept in registers.  The IoU of a pair does not depend
    // on the chain's state (only the selection does), so the IoUs of four
    // consecutive predictions are computed together and their latencies
    // overlap; the four selections then run in order.
    constexpr int U = 4;
    const bool real = lane < n;
    const int jl = real ? lane : 0;  // in bounds; the value is unused when !real
    const double bx1 = g[jl], by1 = g[Ms + jl], bx2 = g[2 * Ms + jl], by2 = g[3 * Ms + jl];
    const int gl = glabel[jl];
    const bool g_in = kBands ? in_band((by2 - by1) * scale, lo, hi) : true;
    for (int r0 = 0; r0 < K; r0 += U) {
      int pi[U];
      bool cand[U], p_in[U];
      double iou[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pi[u] = order[min(r0 + u, K - 1)];
        const float4 p = *reinterpret_cast<const float4*>(pbox + 4 * pi[u]);
        iou[u] = pair_iou(p, bx1, by1, bx2, by2);
        cand[u] = real && plabel[pi[u]] == gl && iou[u] >= th;
        p_in[u] = kBands ? in_band((double)(p.w - p.y) * scale, lo, hi) : true;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (r0 + u >= K) break;
        const bool c = cand[u] && !(taken & 1u);
        int hit = take_best(iou[u], c && g_in ? lane : -1, lane, taken);
        if constexpr (kBands) {
          if (!hit) hit = 2 * take_best(iou[u], c && !g_in ? lane : -1, lane, taken);
          if (!hit) hit = p_in[u] ? 0 : 2;
        }
        if (lane == 0) tpb[(size_t)pi[u] * T] = (uint8_t)hit;
      }
    }
    return;
  }
  uint32_t inb = 0;  // bit jj: truth lane + 64 jj is in the band
  if constexpr (kBands) {
    for (int j = lane, jj = 0; j < n; j += 64, ++jj)
      if (in_band((g[3 * Ms + j] - g[Ms + j]) * scale, lo, hi)) inb |= 1u << jj;
  }
  for (int r = 0; r < K; ++r) {
    const int i = order[r];
    const float4 p = *reinterpret_cast<const float4*>(pbox + 4 * i);
    const int pl = plabel[i];
    double best = 0.0, obest = 0.0;  // the lane's best in-band and out-of-band candidates
    int best_j = -1, obest_j = -1;
    for (int j = lane, jj = 0; j < n; j += 64, ++jj) {
      const double iou = pair_iou(p, g[j], g[Ms + j], g[2 * Ms + j], g[3 * Ms + j]);
      if (glabel[j] == pl && !((taken >> jj) & 1u) && iou >= th) {
        if (!kBands || ((inb >> jj) & 1u))
          better(best, best_j, iou, j);
        else
          better(obest, obest_j, iou, j);
      }
    }
    int hit = take_best(best, best_j, lane, taken);
    if constexpr (kBands) {
      if (!hit) hit = 2 * take_best(obest, obest_j, lane, taken);
      if (!hit) hit = in_band((double)(p.w - p.y) * scale, lo, hi) ? 0 : 2;
    }
    if (lane == 0) tpb[(size_t)i * T] = (uint8_t)hit;
  }
}

__global__ __launch_bounds__(1024) void eval_match_kernel(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ labels,
    const double* __restrict__ gt_boxes, const int32_t* __restrict__ gt_labels, const int32_t* __restrict__ n_valid,
    const double* __restrict__ thr, int K, int M, int T, uint8_t* __restrict__ tp) {
  eval_match_image<false>(boxes, scores, labels, gt_boxes, gt_labels, n_valid, thr, K, M, T,
                          tp + (size_t)blockIdx.x * K * T, 1.0, 0.0, 0.0);
}

// grid (B, R): workgroup (b, r) matches image b for band r; code uint8 [B][R][K][T]
__global__ __launch_bounds__(1024) void eval_match_bands_kernel(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ labels,
    const double* __restrict__ gt_boxes, const int32_t* __restrict__ gt_labels, const int32_t* __restrict__ n_valid,
    const double* __restrict__ thr, const double* __restrict__ scale, const double* __restrict__ bands, int K, int M,
    int T, uint8_t* __restrict__ code) {
  const int b = blockIdx.x, r = blockIdx.y;
  eval_match_image<true>(boxes, scores, labels, gt_boxes, gt_labels, n_valid, thr, K, M, T,
                         code + ((size_t)b * gridDim.y + r) * K * T, scale[b], bands[2 * r], bands[2 * r + 1]);
}

}  // namespace moe

using namespace moe;

extern "C" int rtdetr_eval_match(const float* boxes, const float* scores, const int32_t* labels,
                                 const double* gt_boxes, const int32_t* gt_labels, const int32_t* n_valid,
                                 const double* thr, int B, int K, int M, int T, uint8_t* tp, hipStream_t stream) {
  if (B < 1 || K < 1 || M < 1 || T < 1 || K > kEvalMaxK || M > kEvalMaxM || T > kEvalMaxT)
    return fail("rtdetr_eval_match: need B >= 1, 1 <= K <= 1024, 1 <= M <= 1024, 1 <= T <= 16");
  if (!boxes || !scores || !labels || !gt_boxes || !gt_labels || !n_valid || !thr || !tp)
    return fail("rtdetr_eval_match: NULL pointer");
  const size_t shmem = EvalLds(K, M).total;
  if (shmem > 64 * 1024) return fail("rtdetr_eval_match: K/M too large for LDS");
  ProfScope prof(stream, PROF_EVAL, (double)B * (K * 24.0 + M * 36.0 + 4.0 + (double)K * T) + 8.0 * T);
  MOE_LAUNCH(prof, eval_match_kernel, dim3(B), dim3(64 * T), shmem, stream, boxes, scores, labels, gt_boxes,
             gt_labels, n_valid, thr, K, M, T, tp);
  return check_launch("rtdetr_eval_match");
}

extern "C" int rtdetr_eval_match_bands(const float* boxes, const float* scores, const int32_t* labels,
                                       const double* gt_boxes, const int32_t* gt_labels, const int32_t* n_valid,
                                       const double* thr, const double* scale, const double* bands, int B, int K,
                                       int M, int T, int R, uint8_t* code, hipStream_t stream) {
  if (B < 1 || K < 1 || M < 1 || T < 1 || R < 1 || K > kEvalMaxK || M > kEvalMaxM || T > kEvalMaxT || R > kEvalMaxR)
    return fail(
        "rtdetr_eval_match_bands: need B >= 1, 1 <= K <= 1024, 1 <= M <= 1024, 1 <= T <= 16, 1 <= R <= 8");
  if (!boxes || !scores || !labels || !gt_boxes || !gt_labels || !n_valid || !thr || !scale || !bands || !code)
    return fail("rtdetr_eval_match_bands: NULL pointer");
  const size_t shmem = EvalLds(K, M).total;
  if (shmem > 64 * 1024) return fail("rtdetr_eval_match_bands: K/M too large for LDS");
  ProfScope prof(stream, PROF_EVAL,
                 (double)B * R * (K * 24.0 + M * 36.0 + 12.0 + (double)K * T) + 8.0 * T + 16.0 * R);
  MOE_LAUNCH(prof, eval_match_bands_kernel, dim3(B, R), dim3(64 * T), shmem, stream, boxes, scores, labels, gt_boxes,
             gt_labels, n_valid, thr, scale, bands, K, M, T, code);
  return check_launch("rtdetr_eval_match_bands");
}
