// Multi-scale deformable attention sampling core of the RT-DETR decoder
// ("Deformable attention via grid_sample is the next
// HIP-kernel candidate ... HBM-gather-bound").
//
//   out[b,q,h,c] = sum_{l,p} attn[b,q,h,l,p] * bilinear(value_l[b,:,:,h,c], loc[b,q,h,l,p])
//
// with grid_sample's conventions (align_corners = False, zero padding).
// value is the flattened multi-level bf16 memory [B, S, H, D] (level l occupies
// rows starts[l] .. starts[l] + h_l*w_l); the fused kernels take its row
// stride ldv, so a layer can read its column slice of a wider buffer.
//
// Every sampling kernel: one (b, q, h) per group of LPG = D/2 lanes; each lane
// owns 2 adjacent channels (4-B bf16x2 loads: a group reads a 64-B contiguous
// row segment per corner), 256-thread blocks.  Forward: registers only.
// Backward: per sample, the group reduces <grad_out, value> terms with
// xor-shuffles for the attention-weight and location gradients, and scatters
// the value gradient.
//   msda_fwd / msda_bwd<.., GV16>   loc and attn given (fp32); value gradient by
//       packed bf16 atomics, or (GV16 = false, the tests' reference) fp32 atomics
//   msda_fused_fwd / _bwd           loc and softmax formed in the kernel from the
//       raw linear outputs, any L * P <= 16; packed bf16 atomics
//   msda_fused_fwd_lp / _bwd_lp     the same, level-batched for a fixed L x P
//   msda_fused_bwd_lp<.., REC> + msda_vgrad_sort / _tile   deterministic value
//       gradient: contributions recorded, then summed in a fixed order in fp32
//
// The arithmetic the families share is written once, in the helpers below:
// the bilinear tap and its in-map corners (msda_tap .. msda_load_corner), a
// sample's forward value (msda_bilinear) and backward terms
// (msda_sample_grad), the packed bf16 atomic add (msda_vgrad_add), and the
// fused location rule with its gradient (msda_fused_tap, msda_fused_grad_off;
// tests/test_gpu_msda.py's _vgrad_reference restates that rule).
// Corners are numbered c = 0..3: bit 0 is x + 1, bit 1 is y + 1.
#include <type_traits>

#include "moe_common.h"
#include "prof.h"

namespace moe {

struct MsdaLevels {
  int h[4], w[4], start[4];
};

__device__ __forceinline__ MsdaLevels load_levels(const int32_t* shapes, const int32_t* starts, int L) {
  MsdaLevels lv;
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    lv.h[l] = l < L ? shapes[2 * l] : 0;
    lv.w[l] = l < L ? shapes[2 * l + 1] : 0;
    lv.start[l] = l < L ? starts[l] : 0;
  }
  return lv;
}

// a lane's 2 adjacent bf16 channels (or a sample's x, y offsets) as one 4-B word
__device__ __forceinline__ uint32_t ld_pair(const uint16_t* p) { return *reinterpret_cast<const uint32_t*>(p); }

__device__ __forceinline__ float2 unpack_bf16x2(uint32_t v) {
  return make_float2(__uint_as_float(v << 16), __uint_as_float(v & 0xffff0000u));
}

// A sample's bilinear tap on a level of Hl x Wl pixels: the top-left corner
// and the fractions towards the next column / row.
struct MsdaTap {
  int x0, y0;
  float fx, fy;
};

__device__ __forceinline__ MsdaTap msda_tap(float lx, float ly, int Hl, int Wl) {
  const float x = lx * Wl - 0.5f, y = ly * Hl - 0.5f;
  const float xf = floorf(x), yf = floorf(y);
  return {(int)xf, (int)yf, x - xf, y - yf};
}

// Whether pixel (xi, yi) lies inside a level of Hl x Wl pixels.  A macro, and
// msda_level_geo and the REC path write a corner's (xi, yi) and row out: as
// calls these are simplified on their own before inlining (to bitwise ANDs),
// and the level-batched kernels then compile to other, slower code.
#define MSDA_IN_MAP(xi, yi, Hl, Wl) ((xi) >= 0 && (xi) < (Wl) && (yi) >= 0 && (yi) < (Hl))

__device__ __forceinline__ bool msda_corner_in(const MsdaTap& t, int c, int Hl, int Wl) {
  const int xi = t.x0 + (c & 1), yi = t.y0 + (c >> 1);
  return MSDA_IN_MAP(xi, yi, Hl, Wl);
}

// row of corner c within its level
__device__ __forceinline__ int msda_corner_row(const MsdaTap& t, int c, int Wl) {
  const int xi = t.x0 + (c & 1), yi = t.y0 + (c >> 1);
  return yi * Wl + xi;
}

// The lane's channel pair at corner c (vb: the level's first row at the lane's
// channels, `stride` elements per row) and whether the corner is inside the
// map: zeros and false outside, and for a lane without work (!valid).
__device__ __forceinline__ bool msda_load_corner(const MsdaTap& t, int c, int Hl, int Wl, const uint16_t* vb,
                                                 size_t stride, bool valid, float2& v) {
  const bool in = msda_corner_in(t, c, Hl, Wl) && valid;
  v = in ? unpack_bf16x2(ld_pair(vb + (size_t)msda_corner_row(t, c, Wl) * stride)) : make_float2(0.f, 0.f);
  return in;
}

// A sample's forward value: the weighted sum over the corners inside the map
// (corner weights as w00 .. w11 of msda_sample_grad: the two must agree).
// inside(c) says whether corner c is inside, load(c) returns the lane's channel
// pair there (the generic kernels load it at that point, the level-batched
// ones have it in registers).
template <class Inside, class Load>
__device__ __forceinline__ float2 msda_bilinear(float fx, float fy, Inside&& inside, Load&& load) {
  float2 s = make_float2(0.f, 0.f);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (!inside(c)) continue;
    const float wgt = ((c & 1) ? fx : 1.f - fx) * ((c >> 1) ? fy : 1.f - fy);
    const float2 v = load(c);
    s.x += wgt * v.x;
    s.y += wgt * v.y;
  }
  return s;
}

// A sample's backward terms from the lane's 4 corner values (0 outside the
// map) and its grad_out pair g: the corner weights, and -- summed over the
// group's channels -- ga = d out / d attn and gx, gy = d out / d pixel x, y
// per unit attn.  Every lane of the group must call it (shuffles).
template <int LPG>
__device__ __forceinline__ void msda_sample_grad(const float2 (&v)[2][2], float fx, float fy, float2 g,
                                                 float (&w)[4], float& ga, float& gx, float& gy) {
  const float w00 = (1.f - fx) * (1.f - fy), w01 = fx * (1.f - fy);
  const float w10 = (1.f - fx) * fy, w11 = fx * fy;
  // sampled value and its spatial derivatives (per channel)
  const float sx = w00 * v[0][0].x + w01 * v[0][1].x + w10 * v[1][0].x + w11 * v[1][1].x;
  const float sy = w00 * v[0][0].y + w01 * v[0][1].y + w10 * v[1][0].y + w11 * v[1][1].y;
  const float dxa = (1.f - fy) * (v[0][1].x - v[0][0].x) + fy * (v[1][1].x - v[1][0].x);
  const float dxb = (1.f - fy) * (v[0][1].y - v[0][0].y) + fy * (v[1][1].y - v[1][0].y);
  const float dya = (1.f - fx) * (v[1][0].x - v[0][0].x) + fx * (v[1][1].x - v[0][1].x);
  const float dyb = (1.f - fx) * (v[1][0].y - v[0][0].y) + fx * (v[1][1].y - v[0][1].y);
  ga = g.x * sx + g.y * sy;           // d out / d attn
  gx = g.x * dxa + g.y * dxb;         // d out / d x (per unit attn)
  gy = g.x * dya + g.y * dyb;
  ga = group_sum<LPG>(ga);
  gx = group_sum<LPG>(gx);
  gy = group_sum<LPG>(gy);
  w[0] = w00; w[1] = w01; w[2] = w10; w[3] = w11;
}

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

// One corner's value-gradient contribution into a bf16 grad_value: a lane's 2
// channels (packed bf16, e.g. msda_vgrad_pair(s, g)) in one
// global_atomic_pk_add_bf16 -- half the atomics and half the zero-fill of an
// fp32 buffer, and no fp32 -> bf16 pass afterwards.  Each (token, head) row
// receives < 1 contribution per step on average (230K samples x 4 corners over
// 1.2M rows at C2), so the per-add bf16 rounding stays at the level of the
// final cast it replaces (tests/test_gpu_msda.py).
__device__ __forceinline__ uint32_t msda_vgrad_pair(float s, float2 g) {
  bf16x2_t t;
  t.x = (__bf16)(s * g.x);
  t.y = (__bf16)(s * g.y);
  return __builtin_bit_cast(uint32_t, t);
}

__device__ __forceinline__ void msda_vgrad_add(uint16_t* dst, uint32_t pair) {
  __builtin_amdgcn_global_atomic_fadd_v2bf16((__attribute__((address_space(1))) bf16x2_t*)dst,
                                             __builtin_bit_cast(bf16x2_t, pair));
}

template <int LPG>  // lanes per (b,q,h) group = D / 2
__global__ __launch_bounds__(256) void msda_fwd_kernel(const uint16_t* __restrict__ value,
                                                       const int32_t* __restrict__ shapes,
                                                       const int32_t* __restrict__ starts,
                                                       const float* __restrict__ loc,
                                                       const float* __restrict__ attn, int B, int S, int Q,
                                                       int H, int L, int P, uint16_t* __restrict__ out) {
  constexpr int D = 2 * LPG;
  const MsdaLevels lv = load_levels(shapes, starts, L);
  const int groups = B * Q * H;
  const int sub = threadIdx.x % LPG;
  for (int gidx = (blockIdx.x * blockDim.x + threadIdx.x) / LPG; gidx < groups;
       gidx += gridDim.x * blockDim.x / LPG) {
    const int h = gidx % H;
    const int b = gidx / (Q * H);
    const float* lp = loc + (size_t)gidx * L * P * 2;
    const float* ap = attn + (size_t)gidx * L * P;
    float acc0 = 0.f, acc1 = 0.f;
    for (int l = 0; l < L; ++l) {
      const int Hl = lv.h[l], Wl = lv.w[l];
      const uint16_t* vb = value + ((size_t)b * S + lv.start[l]) * H * D + h * D + 2 * sub;
      for (int p = 0; p < P; ++p) {
        const int sp = l * P + p;
        const MsdaTap t = msda_tap(lp[2 * sp], lp[2 * sp + 1], Hl, Wl);
        const float a = ap[sp];
        const float2 s = msda_bilinear(
            t.fx, t.fy, [&](int c) { return msda_corner_in(t, c, Hl, Wl); },
            [&](int c) { return unpack_bf16x2(ld_pair(vb + (size_t)msda_corner_row(t, c, Wl) * H * D)); });
        acc0 += a * s.x;
        acc1 += a * s.y;
      }
    }
    *reinterpret_cast<uint32_t*>(out + (size_t)gidx * D + 2 * sub) = pack2bf(acc0, acc1);
  }
}

template <int LPG, bool GV16>
__global__ __launch_bounds__(256) void msda_bwd_kernel(
    const uint16_t* __restrict__ value, const int32_t* __restrict__ shapes,
    const int32_t* __restrict__ starts, const float* __restrict__ loc, const float* __restrict__ attn,
    const uint16_t* __restrict__ grad_out, int B, int S, int Q, int H, int L, int P,
    void* __restrict__ grad_value_, float* __restrict__ grad_loc, float* __restrict__ grad_attn) {
  constexpr int D = 2 * LPG;
  const MsdaLevels lv = load_levels(shapes, starts, L);
  const int groups = B * Q * H;
  const int sub = threadIdx.x % LPG;
  // every lane of a group iterates the same trip counts: shuffles stay convergent
  const int ngrp_total = (gridDim.x * blockDim.x) / LPG;
  const int first = (blockIdx.x * blockDim.x + threadIdx.x) / LPG;
  const int iters = (groups + ngrp_total - 1) / ngrp_total;
  for (int it = 0; it < iters; ++it) {
    const int gidx = first + it * ngrp_total;
    const bool valid = gidx < groups;
    const int gi = valid ? gidx : 0;
    const int h = gi % H;
    const int b = gi / (Q * H);
    const float* lp = loc + (size_t)gi * L * P * 2;
    const float* ap = attn + (size_t)gi * L * P;
    const float2 g = valid ? unpack_bf16x2(ld_pair(grad_out + (size_t)gi * D + 2 * sub)) : make_float2(0.f, 0.f);
    for (int l = 0; l < L; ++l) {
      const int Hl = lv.h[l], Wl = lv.w[l];
      const size_t row0 = (size_t)b * S + lv.start[l];
      const uint16_t* vb = value + row0 * H * D + h * D + 2 * sub;
      const size_t gofs = row0 * H * D + h * D + 2 * sub;
      for (int p = 0; p < P; ++p) {
        const int sp = l * P + p;
        const float a = ap[sp];
        const MsdaTap t = msda_tap(lp[2 * sp], lp[2 * sp + 1], Hl, Wl);
        float2 v[2][2];
        bool in[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          in[c] = msda_load_corner(t, c, Hl, Wl, vb, (size_t)H * D, valid, v[c >> 1][c & 1]);
        float wc[4], ga, gx, gy;
        msda_sample_grad<LPG>(v, t.fx, t.fy, g, wc, ga, gx, gy);
        if (valid && sub == 0) {
          grad_attn[(size_t)gi * L * P + sp] = ga;
          grad_loc[((size_t)gi * L * P + sp) * 2] = a * gx * Wl;
          grad_loc[((size_t)gi * L * P + sp) * 2 + 1] = a * gy * Hl;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (!in[c]) continue;
          const float s = a * wc[c];
          const size_t o = gofs + (size_t)msda_corner_row(t, c, Wl) * H * D;
          if constexpr (GV16) {
            msda_vgrad_add(static_cast<uint16_t*>(grad_value_) + o, msda_vgrad_pair(s, g));
          } else {
            float* dst = static_cast<float*>(grad_value_) + o;
            atomicAdd(dst, s * g.x);
            atomicAdd(dst + 1, s * g.y);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Fused variant (decoder cross-attention, TrainStep): the sampling locations
// and attention weights are formed inside the kernel from the raw linear
// outputs -- loc by msda_fused_tap below and attn = softmax over the L*P
// logits of the (b, q, h) group -- and the backward returns the gradients of
// those linear outputs (softmax backward and the location chain rule fused).
// Replaces ~14 element-wise launches per decoder layer.  ref carries no
// gradient (RT-DETR detaches the reference boxes).  L*P <= 16.
// ---------------------------------------------------------------------------
constexpr int MSDA_LP_MAX = 16;

struct MsdaPrep {
  float a[MSDA_LP_MAX];
  float rx, ry, rw, rh;
};

__device__ __forceinline__ void msda_prep(const uint16_t* __restrict__ logits, const float* __restrict__ ref,
                                          int gi, int H, int LP, MsdaPrep& pr) {
  const uint16_t* lg = logits + (size_t)gi * LP;
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < MSDA_LP_MAX; ++i) {
    pr.a[i] = i < LP ? bf2f(lg[i]) : -INFINITY;
    m = fmaxf(m, pr.a[i]);
  }
  float ssum = 0.f;
#pragma unroll
  for (int i = 0; i < MSDA_LP_MAX; ++i) {
    pr.a[i] = i < LP ? expf(pr.a[i] - m) : 0.f;
    ssum += pr.a[i];
  }
  const float inv = 1.f / ssum;
#pragma unroll
  for (int i = 0; i < MSDA_LP_MAX; ++i) pr.a[i] *= inv;
  const float4 r = *reinterpret_cast<const float4*>(ref + (size_t)(gi / H) * 4);
  pr.rx = r.x; pr.ry = r.y; pr.rw = r.z; pr.rh = r.w;
}

__device__ __forceinline__ float msda_pick(const float (&v)[MSDA_LP_MAX], int i) {
  float r = 0.f;
#pragma unroll
  for (int j = 0; j < MSDA_LP_MAX; ++j)
    if (j == i) r = v[j];
  return r;
}

// The fused location rule: a sample's offset (oxy: the bf16 linear outputs for
// x and y, as one 4-B word) is divided by P and rounded to bf16 again -- as the
// unfused decoder's bf16 `off / P` -- and then scales the reference box in fp32:
//   loc = ref.xy + bf16(off / P) * ref.wh * offset_scale        (invP = 1 / P)
// Returns the sample's tap on a level of Hl x Wl pixels.
__device__ __forceinline__ MsdaTap msda_fused_tap(uint32_t oxy, const MsdaPrep& pr, float offset_scale, float invP,
                                                  int Hl, int Wl) {
  const float ox = bf2f(f2bf(bf2f((uint16_t)(oxy & 0xffffu)) * invP));
  const float oy = bf2f(f2bf(bf2f((uint16_t)(oxy >> 16)) * invP));
  const float lx = pr.rx + ox * pr.rw * offset_scale;
  const float ly = pr.ry + oy * pr.rh * offset_scale;
  return msda_tap(lx, ly, Hl, Wl);
}

// ... and its backward, from the location gradient (glx, gly) to the packed
// bf16 offset gradient: d loc / d off = ref.wh * offset_scale / P, straight
// through the bf16 rounding.
__device__ __forceinline__ uint32_t msda_fused_grad_off(float glx, float gly, const MsdaPrep& pr, float offset_scale,
                                                        float invP) {
  return pack2bf(glx * pr.rw * offset_scale * invP, gly * pr.rh * offset_scale * invP);
}

template <int LPG>
__global__ __launch_bounds__(256) void msda_fused_fwd_kernel(
    const uint16_t* __restrict__ value, const int32_t* __restrict__ shapes, const int32_t* __restrict__ starts,
    const uint16_t* __restrict__ off, const float* __restrict__ ref, const uint16_t* __restrict__ logits,
    float offset_scale, int B, int S, int Q, int H, int L, int P, long long ldv, uint16_t* __restrict__ out) {
  constexpr int D = 2 * LPG;
  const MsdaLevels lv = load_levels(shapes, starts, L);
  const int groups = B * Q * H;
  const int sub = threadIdx.x % LPG;
  const int LP = L * P;
  const float invP = 1.f / (float)P;
  for (int gidx = (blockIdx.x * blockDim.x + threadIdx.x) / LPG; gidx < groups;
       gidx += gridDim.x * blockDim.x / LPG) {
    const int h = gidx % H;
    const int b = gidx / (Q * H);
    MsdaPrep pr;
    msda_prep(logits, ref, gidx, H, LP, pr);
    const uint16_t* op = off + (size_t)gidx * LP * 2;
    float acc0 = 0.f, acc1 = 0.f;
    for (int l = 0; l < L; ++l) {
      const int Hl = lv.h[l], Wl = lv.w[l];
      const size_t row0 = (size_t)b * S + lv.start[l];
      const uint16_t* vb = value + row0 * ldv + h * D + 2 * sub;
      for (int p = 0; p < P; ++p) {
        const int sp = l * P + p;
        const MsdaTap t = msda_fused_tap(op[2 * sp] | (uint32_t)op[2 * sp + 1] << 16, pr, offset_scale, invP, Hl, Wl);
        const float a = msda_pick(pr.a, sp);
        const float2 s = msda_bilinear(
            t.fx, t.fy, [&](int c) { return msda_corner_in(t, c, Hl, Wl); },
            [&](int c) { return unpack_bf16x2(ld_pair(vb + (size_t)msda_corner_row(t, c, Wl) * ldv)); });
        acc0 += a * s.x;
        acc1 += a * s.y;
      }
    }
    *reinterpret_cast<uint32_t*>(out + (size_t)gidx * D + 2 * sub) = pack2bf(acc0, acc1);
  }
}

template <int LPG>
__global__ __launch_bounds__(256) void msda_fused_bwd_kernel(
    const uint16_t* __restrict__ value, const int32_t* __restrict__ shapes, const int32_t* __restrict__ starts,
    const uint16_t* __restrict__ off, const float* __restrict__ ref, const uint16_t* __restrict__ logits,
    float offset_scale, const uint16_t* __restrict__ grad_out, int B, int S, int Q, int H, int L, int P,
    long long ldv, uint16_t* __restrict__ grad_value, uint16_t* __restrict__ grad_off,
    uint16_t* __restrict__ grad_logits) {
  constexpr int D = 2 * LPG;
  const MsdaLevels lv = load_levels(shapes, starts, L);
  const int groups = B * Q * H;
  const int sub = threadIdx.x % LPG;
  const int LP = L * P;
  const float invP = 1.f / (float)P;
  const int ngrp_total = (gridDim.x * blockDim.x) / LPG;
  const int first = (blockIdx.x * blockDim.x + threadIdx.x) / LPG;
  const int iters = (groups + ngrp_total - 1) / ngrp_total;
  for (int it = 0; it < iters; ++it) {  // uniform trip count: shuffles stay convergent
    const int gidx = first + it * ngrp_total;
    const bool valid = gidx < groups;
    const int gi = valid ? gidx : 0;
    const int h = gi % H;
    const int b = gi / (Q * H);
    MsdaPrep pr;
    msda_prep(logits, ref, gi, H, LP, pr);
    const uint16_t* op = off + (size_t)gi * LP * 2;
    const float2 g = valid ? unpack_bf16x2(ld_pair(grad_out + (size_t)gi * D + 2 * sub)) : make_float2(0.f, 0.f);
    float gaa[MSDA_LP_MAX];
#pragma unroll
    for (int i = 0; i < MSDA_LP_MAX; ++i) gaa[i] = 0.f;
    float dot = 0.f;  // sum_sp a_sp ga_sp (softmax backward)
    for (int l = 0; l < L; ++l) {
      const int Hl = lv.h[l], Wl = lv.w[l];
      const size_t row0 = (size_t)b * S + lv.start[l];
      const uint16_t* vb = value + row0 * ldv + h * D + 2 * sub;
      const size_t gofs = row0 * ldv + h * D + 2 * sub;
      for (int p = 0; p < P; ++p) {
        const int sp = l * P + p;
        const MsdaTap t = msda_fused_tap(op[2 * sp] | (uint32_t)op[2 * sp + 1] << 16, pr, offset_scale, invP, Hl, Wl);
        const float a = msda_pick(pr.a, sp);
        float2 v[2][2];
        bool in[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) in[c] = msda_load_corner(t, c, Hl, Wl, vb, ldv, valid, v[c >> 1][c & 1]);
        float wc[4], ga, gx, gy;
        msda_sample_grad<LPG>(v, t.fx, t.fy, g, wc, ga, gx, gy);
#pragma unroll
        for (int i = 0; i < MSDA_LP_MAX; ++i)
          if (i == sp) gaa[i] = ga;
        dot += a * ga;
        if (valid && sub == 0)
          *reinterpret_cast<uint32_t*>(grad_off + ((size_t)gi * LP + sp) * 2) =
              msda_fused_grad_off(a * gx * Wl, a * gy * Hl, pr, offset_scale, invP);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (!in[c]) continue;
          const float s = a * wc[c];
          msda_vgrad_add(grad_value + gofs + (size_t)msda_corner_row(t, c, Wl) * ldv, msda_vgrad_pair(s, g));
        }
      }
    }
    // softmax backward: d logit_sp = a_sp (ga_sp - sum_j a_j ga_j); lane `sub` writes sample sub
    if (valid && sub < LP) {
      const float a = msda_pick(pr.a, sub);
      grad_logits[(size_t)gi * LP + sub] = f2bf(a * (msda_pick(gaa, sub) - dot));
    }
  }
}

// ---------------------------------------------------------------------------
// Level-batched fused kernels for the RT-DETR decoder's fixed L = LL, P = PP
// (3 x 4): the loops are unrolled, the group's sampling offsets are loaded
// once, and the 4 PP corner loads of a level are issued together -- the
// generic kernels above issue one sample's offsets and corners per dependent
// round trip (24 per (b, q, h) group).  The backward also issues level l+1's
// corner loads BEFORE level l's value-gradient atomics: on gfx9 `vmcnt` counts
// stores and atomics too, so loads issued after the atomics would wait for
// them.  Same arithmetic, per sample and in the same order, as the generic
// kernels (the location / offset gradients are written by lane `sample`
// instead of lane 0).
// ---------------------------------------------------------------------------
int g_msda_generic = 0;  // moe_set_tuning("msda_generic", bits): 1 generic forward, 2 generic backward (A/B)

template <int PP>
struct MsdaLevelGeo {
  uint32_t raw[PP][4];  // the 4 corners' bf16x2 channel pairs (0 outside the map)
  float fx[PP], fy[PP];
  int x0[PP], y0[PP];
  uint32_t in;          // bit 4 p + c: corner c of sample p inside the map
};

template <int LPG, int LL, int PP>
__device__ __forceinline__ void msda_level_geo(const MsdaLevels& lv, int l, const MsdaPrep& pr,
                                               const uint32_t (&offw)[LL * PP], float offset_scale,
                                               const uint16_t* vb, long long ldv, bool valid, MsdaLevelGeo<PP>& g) {
  constexpr float invP = 1.f / (float)PP;
  const int Hl = lv.h[l], Wl = lv.w[l];
  g.in = 0u;
#pragma unroll
  for (int p = 0; p < PP; ++p) {
    const MsdaTap t = msda_fused_tap(offw[l * PP + p], pr, offset_scale, invP, Hl, Wl);
    g.x0[p] = t.x0;
    g.y0[p] = t.y0;
    g.fx[p] = t.fx;
    g.fy[p] = t.fy;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int xi = t.x0 + (c & 1), yi = t.y0 + (c >> 1);
      const bool in = valid && MSDA_IN_MAP(xi, yi, Hl, Wl);
      g.in |= in ? (1u << (4 * p + c)) : 0u;
      g.raw[p][c] = in ? ld_pair(vb + (size_t)(yi * Wl + xi) * ldv) : 0u;
    }
  }
}

template <int LPG, int LL, int PP>
__global__ __launch_bounds__(256) void msda_fused_fwd_lp_kernel(
    const uint16_t* __restrict__ value, const int32_t* __restrict__ shapes, const int32_t* __restrict__ starts,
    const uint16_t* __restrict__ off, const float* __restrict__ ref, const uint16_t* __restrict__ logits,
    float offset_scale, int B, int S, int Q, int H, long long ldv, uint16_t* __restrict__ out) {
  constexpr int D = 2 * LPG;
  constexpr int LP = LL * PP;
  const MsdaLevels lv = load_levels(shapes, starts, LL);
  const int groups = B * Q * H;
  const int sub = threadIdx.x % LPG;
  for (int gidx = (blockIdx.x * blockDim.x + threadIdx.x) / LPG; gidx < groups;
       gidx += gridDim.x * blockDim.x / LPG) {
    const int h = gidx % H;
    const int b = gidx / (Q * H);
    uint32_t offw[LP];
    const uint32_t* op = reinterpret_cast<const uint32_t*>(off + (size_t)gidx * LP * 2);
#pragma unroll
    for (int i = 0; i < LP; ++i) offw[i] = op[i];
    MsdaPrep pr;
    msda_prep(logits, ref, gidx, H, LP, pr);
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int l = 0; l < LL; ++l) {
      const uint16_t* vb = value + ((size_t)b * S + lv.start[l]) * ldv + h * D + 2 * sub;
      MsdaLevelGeo<PP> g;
      msda_level_geo<LPG, LL, PP>(lv, l, pr, offw, offset_scale, vb, ldv, true, g);
#pragma unroll
      for (int p = 0; p < PP; ++p) {
        const float2 s = msda_bilinear(
            g.fx[p], g.fy[p], [&](int c) { return (g.in & (1u << (4 * p + c))) != 0; },
            [&](int c) { return unpack_bf16x2(g.raw[p][c]); });
        const float a = pr.a[l * PP + p];
        acc0 += a * s.x;
        acc1 += a * s.y;
      }
    }
    *reinterpret_cast<uint32_t*>(out + (size_t)gidx * D + 2 * sub) = pack2bf(acc0, acc1);
  }
}

// REC: instead of the value-gradient atomics, every corner contribution is
// RECORDED as (row within its level or -1, weight a * w_c) at its natural
// position ((b H + h) LL + l) [Q PP 4] + (q PP + p) 4 + c of `rec`; the
// deterministic value gradient (msda_vgrad_sort_kernel + msda_vgrad_tile_kernel
// below) sums them in that order in fp32.
template <int LPG, int LL, int PP, bool REC = false>
__global__ __launch_bounds__(256) void msda_fused_bwd_lp_kernel(
    const uint16_t* __restrict__ value, const int32_t* __restrict__ shapes, const int32_t* __restrict__ starts,
    const uint16_t* __restrict__ off, const float* __restrict__ ref, const uint16_t* __restrict__ logits,
    float offset_scale, const uint16_t* __restrict__ grad_out, int B, int S, int Q, int H, long long ldv,
    uint16_t* __restrict__ grad_value, uint16_t* __restrict__ grad_off, uint16_t* __restrict__ grad_logits,
    int2* __restrict__ rec) {
  constexpr int D = 2 * LPG;
  constexpr int LP = LL * PP;
  constexpr float invP = 1.f / (float)PP;
  const MsdaLevels lv = load_levels(shapes, starts, LL);
  const int groups = B * Q * H;
  const int sub = threadIdx.x % LPG;
  const int ngrp_total = (gridDim.x * blockDim.x) / LPG;
  const int first = (blockIdx.x * blockDim.x + threadIdx.x) / LPG;
  const int iters = (groups + ngrp_total - 1) / ngrp_total;
  for (int it = 0; it < iters; ++it) {  // uniform trip count: shuffles stay convergent
    const int gidx = first + it * ngrp_total;
    const bool valid = gidx < groups;
    const int gi = valid ? gidx : 0;
    const int h = gi % H;
    const int b = gi / (Q * H);
    uint32_t offw[LP];
    const uint32_t* op = reinterpret_cast<const uint32_t*>(off + (size_t)gi * LP * 2);
#pragma unroll
    for (int i = 0; i < LP; ++i) offw[i] = op[i];
    MsdaPrep pr;
    msda_prep(logits, ref, gi, H, LP, pr);
    const float2 g = valid ? unpack_bf16x2(ld_pair(grad_out + (size_t)gi * D + 2 * sub)) : make_float2(0.f, 0.f);
    float my_ga = 0.f;        // ga of sample `sub`
    uint32_t my_goff = 0u;    // packed offset gradient of sample `sub`
    float dot = 0.f;          // sum_sp a_sp ga_sp (softmax backward)
    MsdaLevelGeo<PP> geo[2];
    {
      const uint16_t* vb0 = value + ((size_t)b * S + lv.start[0]) * ldv + h * D + 2 * sub;
      msda_level_geo<LPG, LL, PP>(lv, 0, pr, offw, offset_scale, vb0, ldv, valid, geo[0]);
    }
#pragma unroll
    for (int l = 0; l < LL; ++l) {
      MsdaLevelGeo<PP>& cur = geo[l & 1];
      const int Hl = lv.h[l], Wl = lv.w[l];
      const size_t gofs = ((size_t)b * S + lv.start[l]) * ldv + h * D + 2 * sub;
      uint32_t pv[PP][4];
#pragma unroll
      for (int p = 0; p < PP; ++p) {
        const int sp = l * PP + p;
        const float fx = cur.fx[p], fy = cur.fy[p];  // (read before the unpack: the REC code depends on the order)
        float2 v[2][2];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c >> 1][c & 1] = unpack_bf16x2(cur.raw[p][c]);
        float wc[4], ga, gx, gy;
        msda_sample_grad<LPG>(v, fx, fy, g, wc, ga, gx, gy);
        const float a = pr.a[sp];
        dot += a * ga;
        if (sub == sp) {
          my_ga = ga;
          my_goff = msda_fused_grad_off(a * gx * Wl, a * gy * Hl, pr, offset_scale, invP);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          pv[p][c] = msda_vgrad_pair(a * wc[c], g);
        }
      }
      if (l + 1 < LL) {  // next level's corner loads go out before this level's atomics
        const uint16_t* vbn = value + ((size_t)b * S + lv.start[l + 1]) * ldv + h * D + 2 * sub;
        msda_level_geo<LPG, LL, PP>(lv, l + 1, pr, offw, offset_scale, vbn, ldv, valid, geo[(l + 1) & 1]);
      }
      if constexpr (REC) {
        // lane 4 p + c of the group records corner (p, c) of this level
        if (valid && sub < 4 * PP) {
          const int p = sub >> 2, c = sub & 3;
          float fxp = 0.f, fyp = 0.f, ap = 0.f;
          int x0p = 0, y0p = 0;
#pragma unroll
          for (int pp = 0; pp < PP; ++pp)
            if (pp == p) {
              fxp = cur.fx[pp]; fyp = cur.fy[pp]; x0p = cur.x0[pp]; y0p = cur.y0[pp];
              ap = pr.a[l * PP + pp];
            }
          // (the corner weight of msda_bilinear, for a run-time c)
          const float wcn = ((c & 1) ? fxp : 1.f - fxp) * ((c >> 1) ? fyp : 1.f - fyp);
          const int row = (cur.in & (1u << sub)) ? (y0p + (c >> 1)) * Wl + x0p + (c & 1) : -1;
          const int q = (gi / H) % Q;
          const size_t at = ((size_t)(b * H + h) * LL + l) * ((size_t)Q * PP * 4) + (size_t)q * PP * 4 + sub;
          rec[at] = make_int2(row, __float_as_int(ap * wcn));
        }
        (void)pv;
        (void)gofs;
      } else {
#pragma unroll
        for (int p = 0; p < PP; ++p)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (!(cur.in & (1u << (4 * p + c)))) continue;
            const int xi = cur.x0[p] + (c & 1), yi = cur.y0[p] + (c >> 1);
            msda_vgrad_add(grad_value + gofs + (size_t)(yi * Wl + xi) * ldv, pv[p][c]);
          }
      }
    }
    // softmax backward: d logit_sp = a_sp (ga_sp - sum_j a_j ga_j); lane `sub` writes sample sub
    if (valid && sub < LP) {
      const float a = msda_pick(pr.a, sub);
      grad_logits[(size_t)gi * LP + sub] = f2bf(a * (my_ga - dot));
      *reinterpret_cast<uint32_t*>(grad_off + ((size_t)gi * LP + sub) * 2) = my_goff;
    }
  }
}

// ---------------------------------------------------------------------------
// Deterministic value gradient (REC mode).  The recorded corner contributions
// of every (b, h, level) group -- n = Q PP 4 of them, in (q, p, c) order --
// are bucketed by destination tile of kVgRows value rows (a stable counting
// sort, one workgroup per group, ballot ranks per round of 256 entries).  Each tile's workgroup then takes its entries in chunks
// of kVgChunk (in entry order): sorts the chunk by (row, entry) in LDS
// (ballot peer ranks + a row scan: the order is a pure function of the
// entries), forms every entry's fp32 product w x grad_out[q] in parallel (all loads of
// a thread issued together), and each 32-lane group adds the products of its
// rows (rows r % 8 == group) in sorted order into registers -- row-parallel,
// with no dependent memory access inside a row's sum.  Every element of the
// gradient is written (untouched rows get zeros: no memset), every sum has a
// fixed order (bitwise repeatable), and the accumulation is fp32 -- the
// atomic path added bf16 pairs in arrival order.
// ---------------------------------------------------------------------------
constexpr int kVgTilesMax = 128;  // tiles per level (levels up to kVgRows x 128 = 32,768 rows)
constexpr int kVgRows = 256;      // value rows per tile, at most (levels of < 16 x 256 rows take fewer)
constexpr int kVgChunk = 256;     // entries per sorted chunk

// Per-level tiling, by value (kernel arguments: no memory load to find a
// tile): every level holds the same Q P 4 entries per (b, h), so the small
// levels get smaller tiles (R = 16 .. 256 rows, at least 16 tiles where the
// level allows), spreading their many entries per row over more workgroups.
struct VgLevels {
  int hw[4], R[4], nt[4], start[4];
};

// Stable bucketing of a group's entries by tile: 256 entries per round, one
// per thread; within a wave the lanes of one tile are found from 7 ballots of
// the tile bits (rank = peers below the lane).  Pass 1 records every (round,
// wave, tile) count, a per-tile walk over (round, wave) turns them into
// offsets, a scan over tiles gives the tile bases, and pass 2 recomputes the
// ranks and scatters -- entry order kept within a tile, no serial chain per
// thread (each thread's rec loads are issued four rounds at a time).
__global__ __launch_bounds__(256) void msda_vgrad_sort_kernel(const int2* __restrict__ rec, VgLevels lv, int L,
                                                              int n, int4* __restrict__ sorted,
                                                              int32_t* __restrict__ toff) {
  extern __shared__ __attribute__((aligned(16))) int vsm[];
  const int grp = blockIdx.x, l = grp % L, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int R = lv.R[l], nt = lv.nt[l], NR = (n + 255) / 256;
  int* cnt = vsm;                  // [NR][4][nt]: counts, then offsets within the tile
  int* base = vsm + NR * 4 * nt;   // [nt]
  int* wtot = base + kVgTilesMax;  // [4]
  const int2* src = rec + (size_t)grp * n;
  for (int i = tid; i < NR * 4 * nt; i += 256) cnt[i] = 0;
  __syncthreads();
  // one round: the tile of this thread's entry and its rank among the wave's lanes of that tile
  auto rank_of = [&](int row, bool valid, int& tile, uint64_t& peers) {
    tile = valid ? row / R : 0;
    peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 7; ++bit) {
      const bool on = (tile >> bit) & 1;
      const uint64_t bb = __ballot(valid && on);
      peers &= on ? bb : ~bb;
    }
    return __popcll(peers & ((1ull << lane) - 1ull));
  };
  // up to kVgRegRounds rounds (6,144 entries: Q <= 384 at L 3, P 4) are loaded ONCE, all together, and kept
  // in registers for both passes; larger groups reload four rounds at a time
  constexpr int kVgRegRounds = 24;
  int2 vr[kVgRegRounds];
  const bool in_regs = NR <= kVgRegRounds;
  if (in_regs) {
#pragma unroll
    for (int u = 0; u < kVgRegRounds; ++u) {
      const int e = u * 256 + tid;
      vr[u] = (u < NR && e < n) ? src[e] : make_int2(-1, 0);
    }
  }
  for (int pass = 0; pass < 2; ++pass) {
    for (int rd0 = 0; rd0 < NR; rd0 += 4) {
      int2 v[4];
      if (in_regs) {
#pragma unroll
        for (int q = 0; q < kVgRegRounds / 4; ++q)  // (static register indices: select the four rounds)
          if (4 * q == rd0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = vr[4 * q + u];
          }
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // four rounds' loads in flight
          const int e = (rd0 + u) * 256 + tid;
          v[u] = (rd0 + u < NR && e < n) ? src[e] : make_int2(-1, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (rd0 + u >= NR) break;
        const bool valid = v[u].x >= 0;
        int tile;
        uint64_t peers;
        const int rank = rank_of(v[u].x, valid, tile, peers);
        int* c = cnt + ((rd0 + u) * 4 + wave) * nt + tile;
        if (pass == 0) {
          if (valid && rank == 0) *c = __popcll(peers);
        } else if (valid) {
          sorted[(size_t)grp * n + base[tile] + *c + rank] = make_int4(v[u].x, v[u].y, (rd0 + u) * 256 + tid, 0);
        }
      }
    }
    if (pass == 1) break;
    __syncthreads();
    // per tile (thread = tile): offsets over (round, wave) in order, then the scan over tiles
    int tot = 0;
    if (tid < nt) {
      for (int i = 0; i < NR * 4; ++i) {
        const int c = cnt[i * nt + tid];
        cnt[i * nt + tid] = tot;
        tot += c;
      }
    }
    int inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int x = __shfl_up(inc, o);
      if (lane >= o) inc += x;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int b0 = 0;
    for (int w = 0; w < wave; ++w) b0 += wtot[w];
    int32_t* to = toff + (size_t)grp * (kVgTilesMax + 1);
    if (tid < nt) {
      base[tid] = b0 + inc - tot;
      to[tid] = b0 + inc - tot;
    }
    if (tid == nt - 1) to[nt] = b0 + inc;
    __syncthreads();
  }
}

// One workgroup per (b, h, level, tile of R <= 256 rows); 8 groups of 32
// lanes, group g owns the tile rows r % 8 == g (up to 32 row sums per lane of
// D / 32 channels each, in registers across chunks).  A chunk holds one entry
// per thread and is sorted by (row, entry) with no comparison sort: each wave
// finds the lanes holding the same row from 8 ballots of the row bits (rank =
// the peers below the lane), the per-wave row counts are scanned over the
// rows, and every entry lands at rowstart + earlier waves' count + rank.  The
// grad_out rows of the sorted chunk are staged in LDS (bf16) with their
// weights, so a row's sum reads only LDS; the next chunk's entries are loaded
// before this chunk is summed.
template <int D>
__global__ __launch_bounds__(256) void msda_vgrad_tile_kernel(const int4* __restrict__ sorted,
                                                              const int32_t* __restrict__ toff, VgLevels lv,
                                                              const uint16_t* __restrict__ grad_out, int S, int Q,
                                                              int H, int L, int P, int tiles_bh, long long ldv,
                                                              uint16_t* __restrict__ grad_value) {
  constexpr int CH = kVgChunk, RPG = kVgRows / 8;
  constexpr int DL = D / 32;   // channels per lane
  constexpr int PPR = D / 8;   // 16-B pieces per grad_out row
  static_assert(CH == 256 && kVgRows == 256, "one entry per thread, one row per thread in the scan");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* sg = reinterpret_cast<uint16_t*>(smem);                   // [CH][D] grad_out rows, sorted order
  int4* sent = reinterpret_cast<int4*>(sg + CH * D);                  // [CH] the chunk's entries (entry order)
  float* sw = reinterpret_cast<float*>(sent + CH);                    // [CH] weights, sorted order
  int* sidx = reinterpret_cast<int*>(sw + CH);                        // [CH] sorted position -> chunk index
  int* wcnt = sidx + CH;                                              // [4][256] per-wave row counts -> offsets
  int* rs = wcnt + 4 * 256;                                           // [256] first sorted position of a row
  int* re = rs + 256;                                                 // [256] one past its last
  int* wtot = re + 256;                                               // [4] scan: wave totals
  const int tid = threadIdx.x, gk = tid >> 5, ln = tid & 31, wave = tid >> 6, lane = tid & 63;
  const int bh = blockIdx.x / tiles_bh;
  int rem = blockIdx.x - bh * tiles_bh, l = 0;
  while (l < L - 1 && rem >= lv.nt[l]) rem -= lv.nt[l++];
  const int R = lv.R[l], t = rem, b = bh / H, h = bh - b * H;
  const int grp = bh * L + l, n = Q * P * 4;
  const int32_t* to = toff + (size_t)grp * (kVgTilesMax + 1);
  const int j0 = to[t], j1 = to[t + 1];
  const int r0 = t * R, rows = min(R, lv.hw[l] - r0);
  const int4* ent = sorted + (size_t)grp * n;
  const uint16_t* gob = grad_out + ((size_t)b * Q * H + h) * D;  // + q H D: the query's row for head h
  float acc[RPG][DL];
#pragma unroll
  for (int i = 0; i < RPG; ++i)
#pragma unroll
    for (int u = 0; u < DL; ++u) acc[i][u] = 0.f;
  int4 e = make_int4(0, 0, 0, 0);
  if (j0 + tid < j1) e = ent[j0 + tid];
  for (int c0 = j0; c0 < j1; c0 += CH) {
    const int cn = min(CH, j1 - c0);
    const bool valid = tid < cn;
    const int row = valid ? e.x - r0 : 0;
    __syncthreads();  // (the previous chunk's sums are done)
    sent[tid] = e;
    if (c0 + CH + tid < j1) e = ent[c0 + CH + tid];  // the next chunk's entry, in flight meanwhile
#pragma unroll
    for (int w = 0; w < 4; ++w) wcnt[w * 256 + tid] = 0;
    // the wave's lanes holding this lane's row, and this lane's rank among them
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (row >> bit) & 1;
      const uint64_t bb = __ballot(valid && on);
      peers &= on ? bb : ~bb;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    __syncthreads();
    if (valid && rank == 0) wcnt[wave * 256 + row] = __popcll(peers);
    __syncthreads();
    {  // thread = row: earlier waves' counts, the row total, and its exclusive scan over rows
      const int c0w = wcnt[tid], c1w = wcnt[256 + tid], c2w = wcnt[512 + tid], c3w = wcnt[768 + tid];
      wcnt[256 + tid] = c0w;
      wcnt[512 + tid] = c0w + c1w;
      wcnt[768 + tid] = c0w + c1w + c2w;
      wcnt[tid] = 0;
      const int tot = c0w + c1w + c2w + c3w;
      int inc = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(inc, o);
        if (lane >= o) inc += x;
      }
      if (lane == 63) wtot[wave] = inc;
      __syncthreads();
      int base = 0;
      for (int w = 0; w < wave; ++w) base += wtot[w];
      rs[tid] = base + inc - tot;
      re[tid] = base + inc;
    }
    __syncthreads();
    if (valid) sidx[rs[row] + wcnt[wave * 256 + row] + rank] = tid;
    __syncthreads();
    // stage the sorted chunk's grad_out rows (bf16) and weights: all loads of a thread first
    for (int i0 = tid; i0 < cn * PPR; i0 += 256 * 4) {
      uint4 g[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = min(i0 + 256 * u, cn * PPR - 1);
        const int p = i / PPR, pc = i - p * PPR;
        g[u] = reinterpret_cast<const uint4*>(gob + (size_t)(sent[sidx[p]].z / (P * 4)) * H * D)[pc];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 256 * u;
        if (i < cn * PPR) reinterpret_cast<uint4*>(sg)[i] = g[u];
      }
    }
    if (valid) sw[tid] = __int_as_float(sent[sidx[tid]].y);
    __syncthreads();
    // each group adds its rows' terms in sorted order (fp32 fma, as the atomic path's products)
#pragma unroll
    for (int i = 0; i < RPG; ++i) {
      const int r = gk + 8 * i;
      const int p1 = re[r];
      for (int p = rs[r]; p < p1; ++p) {
        const float w = sw[p];
#pragma unroll
        for (int u = 0; u < DL; ++u) acc[i][u] = fmaf(w, bf2f(sg[p * D + ln * DL + u]), acc[i][u]);
      }
    }
  }
  // the tile's rows out as bf16 straight from the sums (a row's D channels: one 64/128-B segment per group),
  // zeros where nothing landed
  uint16_t* gv = grad_value + ((size_t)b * S + lv.start[l] + r0) * ldv + (size_t)h * D;
#pragma unroll
  for (int i = 0; i < RPG; ++i) {
    const int r = gk + 8 * i;
    if (r < rows) {
      if constexpr (DL == 1) {
        gv[(size_t)r * ldv + ln] = f2bf(acc[i][0]);
      } else {
        *reinterpret_cast<uint32_t*>(gv + (size_t)r * ldv + 2 * ln) = pack2bf(acc[i][0], acc[i][1]);
      }
    }
  }
}

}  // namespace moe

using namespace moe;

static int msda_check(int B, int S, int Q, int H, int D, int L, int P) {
  if (B <= 0 || S <= 0 || Q < 0 || H <= 0 || L < 1 || L > 4 || P < 1 || P > 16)
    return fail("msda: bad shape (need L in [1,4], P in [1,16])");
  if (D != 32 && D != 64) return fail("msda: head dim must be 32 or 64");
  return 0;
}

// The argument checks of the fused (atomic) entry points: the shape, L * P
// samples within a group's registers, and a value row stride that holds a row
// and keeps the 4-B channel-pair accesses aligned.
static int msda_fused_check(int B, int S, int Q, int H, int D, int L, int P, long long ldv) {
  if (msda_check(B, S, Q, H, D, L, P)) return -1;
  if (L * P > MSDA_LP_MAX) return fail("msda_fused: L * P must be <= 16");
  if (ldv < (long long)H * D || ldv % 2 != 0) return fail("msda_fused: ldv must be >= H * D and even");
  return 0;
}

static int msda_grid(long long groups, int lpg) {
  long long g = (groups * lpg + 255) / 256;
  return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

// The kernels are instantiated for the two head dims msda_check admits: calls
// f with LPG = D / 2 (lanes per group) as a std::integral_constant.
template <class F>
static void msda_with_lpg(int D, F&& f) {
  if (D == 32)
    f(std::integral_constant<int, 16>{});
  else
    f(std::integral_constant<int, 32>{});
}

static const uint16_t* bf(const void* p) { return static_cast<const uint16_t*>(p); }
static uint16_t* bf(void* p) { return static_cast<uint16_t*>(p); }

extern "C" int rtdetr_msda_fwd(const void* value, const int32_t* shapes, const int32_t* starts,
                               const float* loc, const float* attn, int B, int S, int Q, int H, int D, int L,
                               int P, void* out, hipStream_t stream) {
  if (msda_check(B, S, Q, H, D, L, P)) return -1;
  if (Q == 0) return 0;
  const long long groups = (long long)B * Q * H;
  // bytes: 4 bilinear corners of D bf16 per sample, loc+attn per sample, output rows
  const double samples = (double)groups * L * P;
  ProfScope prof(stream, PROF_MSDA, samples * (8.0 * D + 12.0) + 2.0 * groups * D);
  msda_with_lpg(D, [&](auto lpg) {
    constexpr int LPG = decltype(lpg)::value;
    MOE_LAUNCH(prof, msda_fwd_kernel<LPG>, dim3(msda_grid(groups, LPG)), dim3(256), 0, stream, bf(value), shapes,
               starts, loc, attn, B, S, Q, H, L, P, bf(out));
  });
  return check_launch("rtdetr_msda_fwd");
}

static int msda_bwd_impl(const void* value, const int32_t* shapes, const int32_t* starts, const float* loc,
                         const float* attn, const void* grad_out, int B, int S, int Q, int H, int D, int L, int P,
                         void* grad_value, bool gv16, float* grad_loc, float* grad_attn, hipStream_t stream) {
  if (msda_check(B, S, Q, H, D, L, P)) return -1;
  const size_t gv_bytes = (size_t)B * S * H * D * (gv16 ? 2 : 4);
  const hipError_t e = hipMemsetAsync(grad_value, 0, gv_bytes, stream);
  if (e != hipSuccess) return fail(std::string("rtdetr_msda_bwd: memset: ") + hipGetErrorString(e));
  if (Q == 0) return 0;
  const long long groups = (long long)B * Q * H;
  // bytes: forward's gathers + 4 corner read-modify-writes of D per sample, grad_loc/attn, grad_out
  const double samples = (double)groups * L * P;
  ProfScope prof(stream, PROF_MSDA, samples * (8.0 * D + (gv16 ? 8.0 : 16.0) * D + 24.0) + 2.0 * groups * D);
  msda_with_lpg(D, [&](auto lpg) {
    constexpr int LPG = decltype(lpg)::value;
    const auto kern = gv16 ? msda_bwd_kernel<LPG, true> : msda_bwd_kernel<LPG, false>;
    MOE_LAUNCH(prof, kern, dim3(msda_grid(groups, LPG)), dim3(256), 0, stream, bf(value), shapes, starts, loc, attn,
               bf(grad_out), B, S, Q, H, L, P, grad_value, grad_loc, grad_attn);
  });
  return check_launch("rtdetr_msda_bwd");
}

extern "C" int rtdetr_msda_bwd(const void* value, const int32_t* shapes, const int32_t* starts,
                               const float* loc, const float* attn, const void* grad_out, int B, int S, int Q,
                               int H, int D, int L, int P, float* grad_value, float* grad_loc, float* grad_attn,
                               hipStream_t stream) {
  return msda_bwd_impl(value, shapes, starts, loc, attn, grad_out, B, S, Q, H, D, L, P, grad_value, false, grad_loc,
                       grad_attn, stream);
}

extern "C" int rtdetr_msda_bwd_bf16(const void* value, const int32_t* shapes, const int32_t* starts,
                                    const float* loc, const float* attn, const void* grad_out, int B, int S, int Q,
                                    int H, int D, int L, int P, void* grad_value, float* grad_loc, float* grad_attn,
                                    hipStream_t stream) {
  return msda_bwd_impl(value, shapes, starts, loc, attn, grad_out, B, S, Q, H, D, L, P, grad_value, true, grad_loc,
                       grad_attn, stream);
}

// Strided-value entry points: token (b, s) of the value starts ldv elements
// after token (b, s-1) -- the decoder's six value projections computed as one
// [B*S, 6*H*D] GEMM, each layer reading (and its backward accumulating into)
// its own column slice.  zero_grad_value = 0 leaves grad_value as it is (the
// caller zeroed the shared buffer once).
extern "C" int rtdetr_msda_fused_fwd_ld(const void* value, long long ldv, const int32_t* shapes,
                                        const int32_t* starts, const void* off, const float* ref, const void* logits,
                                        float offset_scale, int B, int S, int Q, int H, int D, int L, int P, void* out,
                                        hipStream_t stream) {
  if (msda_fused_check(B, S, Q, H, D, L, P, ldv)) return -1;
  if (Q == 0) return 0;
  const long long groups = (long long)B * Q * H;
  const double samples = (double)groups * L * P;
  ProfScope prof(stream, PROF_MSDA, samples * (8.0 * D + 6.0) + groups * (2.0 * D + 16.0 / H));
  const uint16_t *v = bf(value), *o = bf(off), *lg = bf(logits);
  uint16_t* y = bf(out);
  const bool lp34 = L == 3 && P == 4 && !(g_msda_generic & 1);
  msda_with_lpg(D, [&](auto lpg) {
    constexpr int LPG = decltype(lpg)::value;
    const dim3 grid(msda_grid(groups, LPG));
    if (lp34)
      MOE_LAUNCH(prof, (msda_fused_fwd_lp_kernel<LPG, 3, 4>), grid, dim3(256), 0, stream, v, shapes, starts, o, ref,
                 lg, offset_scale, B, S, Q, H, ldv, y);
    else
      MOE_LAUNCH(prof, msda_fused_fwd_kernel<LPG>, grid, dim3(256), 0, stream, v, shapes, starts, o, ref, lg,
                 offset_scale, B, S, Q, H, L, P, ldv, y);
  });
  return check_launch("rtdetr_msda_fused_fwd");
}

extern "C" int rtdetr_msda_fused_bwd_ld(const void* value, long long ldv, const int32_t* shapes,
                                        const int32_t* starts, const void* off, const float* ref, const void* logits,
                                        float offset_scale, const void* grad_out, int B, int S, int Q, int H, int D,
                                        int L, int P, void* grad_value, int zero_grad_value, void* grad_off,
                                        void* grad_logits, hipStream_t stream) {
  if (msda_fused_check(B, S, Q, H, D, L, P, ldv)) return -1;
  if (zero_grad_value) {
    if (ldv != (long long)H * D) return fail("msda_fused: zero_grad_value needs a dense grad_value (ldv == H * D)");
    const hipError_t e = hipMemsetAsync(grad_value, 0, (size_t)B * S * H * D * 2, stream);
    if (e != hipSuccess) return fail(std::string("rtdetr_msda_fused_bwd: memset: ") + hipGetErrorString(e));
  }
  if (Q == 0) return 0;
  const long long groups = (long long)B * Q * H;
  const double samples = (double)groups * L * P;
  ProfScope prof(stream, PROF_MSDA, samples * (16.0 * D + 10.0) + groups * (2.0 * D + 16.0 / H));
  const uint16_t *v = bf(value), *o = bf(off), *lg = bf(logits), *go = bf(grad_out);
  uint16_t *gv = bf(grad_value), *gof = bf(grad_off), *glg = bf(grad_logits);
  const bool lp34 = L == 3 && P == 4 && !(g_msda_generic & 2);
  msda_with_lpg(D, [&](auto lpg) {
    constexpr int LPG = decltype(lpg)::value;
    const dim3 grid(msda_grid(groups, LPG));
    if (lp34)
      MOE_LAUNCH(prof, (msda_fused_bwd_lp_kernel<LPG, 3, 4>), grid, dim3(256), 0, stream, v, shapes, starts, o, ref,
                 lg, offset_scale, go, B, S, Q, H, ldv, gv, gof, glg, static_cast<int2*>(nullptr));
    else
      MOE_LAUNCH(prof, msda_fused_bwd_kernel<LPG>, grid, dim3(256), 0, stream, v, shapes, starts, o, ref, lg,
                 offset_scale, go, B, S, Q, H, L, P, ldv, gv, gof, glg);
  });
  return check_launch("rtdetr_msda_fused_bwd");
}

extern "C" int rtdetr_msda_fused_fwd(const void* value, const int32_t* shapes, const int32_t* starts, const void* off,
                                     const float* ref, const void* logits, float offset_scale, int B, int S, int Q,
                                     int H, int D, int L, int P, void* out, hipStream_t stream) {
  return rtdetr_msda_fused_fwd_ld(value, (long long)H * D, shapes, starts, off, ref, logits, offset_scale, B, S, Q, H,
                                  D, L, P, out, stream);
}

extern "C" int rtdetr_msda_fused_bwd(const void* value, const int32_t* shapes, const int32_t* starts, const void* off,
                                     const float* ref, const void* logits, float offset_scale, const void* grad_out,
                                     int B, int S, int Q, int H, int D, int L, int P, void* grad_value,
                                     void* grad_off, void* grad_logits, hipStream_t stream) {
  return rtdetr_msda_fused_bwd_ld(value, (long long)H * D, shapes, starts, off, ref, logits, offset_scale, grad_out,
                                  B, S, Q, H, D, L, P, grad_value, 1, grad_off, grad_logits, stream);
}

// ---------------------------------------------------------------------------
// Deterministic decoder MSDA backward (L = 3, P = 4): the fused backward in
// REC mode, then the per-group tile sort and the per-tile fp32 sums.  Writes
// EVERY element of its grad_value column slice (no zeroing needed).
// hw_host: the L level sizes h_l w_l in HOST memory (they size the tile grid).
// ---------------------------------------------------------------------------
extern "C" long long rtdetr_msda_vgrad_workspace(int B, int Q, int H, int L, int P) {
  const long long n = (long long)B * H * L * Q * P * 4;
  return n * 8 + n * 16 + (long long)B * H * L * (kVgTilesMax + 1) * 4 + 256;
}

extern "C" int rtdetr_msda_fused_bwd_det(const void* value, long long ldv, const int32_t* shapes,
                                         const int32_t* starts, const int32_t* hw_host, const void* off,
                                         const float* ref, const void* logits, float offset_scale,
                                         const void* grad_out, int B, int S, int Q, int H, int D, int L, int P,
                                         void* grad_value, void* grad_off, void* grad_logits, void* work,
                                         long long work_bytes, hipStream_t stream) {
  if (msda_check(B, S, Q, H, D, L, P)) return -1;
  if (L != 3 || P != 4) return fail("msda_fused_bwd_det: needs L = 3, P = 4 (the RT-DETR decoder)");
  if (ldv < (long long)H * D || ldv % 8 != 0) return fail("msda_fused_bwd_det: ldv must be >= H * D, a multiple of 8");
  if (hw_host == nullptr || work == nullptr) return fail("msda_fused_bwd_det: NULL hw_host / work");
  if (work_bytes < rtdetr_msda_vgrad_workspace(B, Q, H, L, P)) return fail("msda_fused_bwd_det: workspace too small");
  if (reinterpret_cast<uintptr_t>(work) % 16 || reinterpret_cast<uintptr_t>(grad_value) % 16)
    return fail("msda_fused_bwd_det: work and grad_value must be 16-B aligned");
  VgLevels lv{};
  int tiles_bh = 0, ntmax = 0, start = 0;
  for (int l = 0; l < L; ++l) {
    const int hw = hw_host[l];
    if (hw < 1 || hw > kVgRows * kVgTilesMax)
      return fail("msda_fused_bwd_det: every level needs 1 .. 32,768 value rows");
    int R = kVgRows;
    while (R > 16 && (hw + R - 1) / R < 16) R >>= 1;  // at least 16 tiles where rows allow, R >= 16
    lv.hw[l] = hw;
    lv.R[l] = R;
    lv.nt[l] = (hw + R - 1) / R;
    lv.start[l] = start;
    start += hw;
    tiles_bh += lv.nt[l];
    ntmax = std::max(ntmax, lv.nt[l]);
  }
  // every row of the slice must belong to a level: the tile kernel writes
  // exactly the level rows, and the caller's buffer is not zeroed
  if (start != S) return fail("msda_fused_bwd_det: the level sizes must sum to S");
  if (Q == 0) {  // no samples: the value gradient is zero (written, not left as it was)
    if (hipMemset2DAsync(grad_value, (size_t)ldv * 2, 0, (size_t)H * D * 2, (size_t)B * S, stream) != hipSuccess)
      return fail("msda_fused_bwd_det: zero fill failed");
    return 0;
  }
  const long long n = (long long)Q * P * 4, n_all = n * B * H * L;
  int2* rec = static_cast<int2*>(work);
  int4* sorted = reinterpret_cast<int4*>(static_cast<char*>(work) + n_all * 8);
  int32_t* toff = reinterpret_cast<int32_t*>(static_cast<char*>(work) + n_all * 24);
  const long long groups = (long long)B * Q * H;
  const uint16_t* go = bf(grad_out);
  uint16_t* gv = bf(grad_value);
  {
    const double samples = (double)groups * L * P;
    ProfScope prof(stream, PROF_MSDA, samples * (8.0 * D + 32.0 + 10.0) + groups * (2.0 * D + 16.0 / H));
    msda_with_lpg(D, [&](auto lpg) {
      constexpr int LPG = decltype(lpg)::value;
      MOE_LAUNCH(prof, (msda_fused_bwd_lp_kernel<LPG, 3, 4, true>), dim3(msda_grid(groups, LPG)), dim3(256), 0,
                 stream, bf(value), shapes, starts, bf(off), ref, bf(logits), offset_scale, go, B, S, Q, H, ldv, gv,
                 bf(grad_off), bf(grad_logits), rec);
    });
    if (int rc = check_launch("rtdetr_msda_fused_bwd_det (samples)")) return rc;
  }
  {
    ProfScope prof(stream, PROF_MSDA, (double)n_all * (8.0 + 16.0) + (double)B * H * L * (kVgTilesMax + 1) * 4);
    const size_t slds = ((size_t)((n + 255) / 256) * 4 * ntmax + kVgTilesMax + 4) * 4;
    if (slds > 150 * 1024) return fail("msda_fused_bwd_det: too many samples per group for the tile sort");
    static unsigned long long sset = 0;  // per-device bitmask
    if (int rc = allow_dyn_lds(reinterpret_cast<const void*>(msda_vgrad_sort_kernel), 150 * 1024, &sset,
                               "msda_fused_bwd_det: LDS attribute"))
      return rc;
    MOE_LAUNCH(prof, msda_vgrad_sort_kernel, dim3(B * H * L), dim3(256), slds, stream, rec, lv, L, (int)n, sorted,
               toff);
    if (int rc = check_launch("rtdetr_msda_fused_bwd_det (sort)")) return rc;
  }
  const size_t lds = (size_t)kVgChunk * (D * 2 + 16 + 4 + 4) + 256 * 24 + 16;
  double rows = 0;
  for (int l = 0; l < L; ++l) rows += hw_host[l];
  ProfScope prof(stream, PROF_MSDA, (double)n_all * (16.0 + 2.0 * D) + rows * B * H * D * 2.0);
  int rc = 0;
  msda_with_lpg(D, [&](auto lpg) {
    constexpr int DD = 2 * decltype(lpg)::value;
    static unsigned long long allowed = 0;  // per-device bitmask (one per instantiation)
    rc = allow_dyn_lds(reinterpret_cast<const void*>(msda_vgrad_tile_kernel<DD>), (int)lds, &allowed,
                       "msda_fused_bwd_det: LDS attribute");
    if (rc) return;
    MOE_LAUNCH(prof, msda_vgrad_tile_kernel<DD>, dim3(B * H * tiles_bh), dim3(256), lds, stream, sorted, toff, lv, go,
               S, Q, H, L, P, tiles_bh, ldv, gv);
  });
  if (rc) return rc;
  return check_launch("rtdetr_msda_fused_bwd_det");
}
