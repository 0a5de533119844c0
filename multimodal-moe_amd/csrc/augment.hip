// Training-time batch augmentation (src/rtdetr_moe/augment.py states the
// semantics; augment_reference there is the plain-torch restatement).
//
//   train_augment_images  one launch per batch: every output pixel of the
//       channels_last [B,3,Hp,Wp] destination goes through its image's inverse
//       2x3 matrix to the source, is sampled bilinearly (a tap outside the
//       content rectangle w x h contributes `fill`), gets the HSV jitter, and
//       is stored as bf16 or fp32.  Each lane produces four adjacent pixels of
//       one row (12 values: three 8-B stores for bf16, three 16-B stores for
//       fp32); a workgroup's 256 lanes cover 1024 consecutive pixels, so the
//       stores of a wave are one contiguous run.  The per-image table row sits
//       at a workgroup-uniform address (scalar loads: one read per wave, held
//       in SGPRs).  The source is addressed through explicit element strides,
//       so NCHW and channels_last, uint8 and fp32 need no pass in front; uint8
//       taps go through a 256-entry LDS table of i / 255 (the same rounded
//       quotient torch's x / 255 gives).  Arithmetic is fp32 in every
//       instance; the source coordinate is formed with unfused multiplies and
//       adds in the reference's order, so the kernel picks the same taps as
//       the fp32 reference bit for bit.
//   train_augment_boxes   one wave per image maps the padded targets through
//       the forward matrix, clips, applies Ultralytics' box_candidates test
//       and compacts the survivors in order (ballot + popcount prefix, 64
//       slots per round); a single-workgroup kernel then sums the new counts
//       (no atomics: a fixed order).
#include "moe_common.h"
#include "prof.h"

namespace moe {

constexpr int kAugTable = 16;  // floats per image: fwd 2x3, inv 2x3, dh, gs, gv, s

template <typename S>
__device__ __forceinline__ float aug_tap(const S* p, const float* lut);
template <>
__device__ __forceinline__ float aug_tap<uint8_t>(const uint8_t* p, const float* lut) {
  return lut[*p];
}
template <>
__device__ __forceinline__ float aug_tap<float>(const float* p, const float*) {
  return *p;
}

// RGB -> HSV, h' = frac(h + dh), s' = min(1, s gs), v' = min(1, v gv), -> RGB
__device__ __forceinline__ void aug_hsv(float& r, float& g, float& b, float dh, float gs, float gv) {
  const float mx = fmaxf(r, fmaxf(g, b));
  const float mn = fminf(r, fminf(g, b));
  const float d = mx - mn;
  const float s = mx > 0.f ? d / mx : 0.f;
  float h6 = 0.f;
  if (d > 0.f) {
    const float num = mx == r ? g - b : (mx == g ? b - r : r - g);
    const float off = mx == r ? 0.f : (mx == g ? 2.f : 4.f);
    h6 = off + num / d;
  }
  float hh = h6 / 6.f + dh;
  hh = hh - floorf(hh);
  const float s2 = fminf(1.f, s * gs);
  const float v2 = fminf(1.f, mx * gv);
  const float c = v2 * s2;
  float out[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float k = (float)(5 - 2 * i) + 6.f * hh;
    k = k >= 6.f ? k - 6.f : k;
    const float a = fminf(fmaxf(fminf(k, 4.f - k), 0.f), 1.f);
    out[i] = v2 - c * a;
  }
  r = out[0];
  g = out[1];
  b = out[2];
}

template <typename S, bool BF16>
__global__ __launch_bounds__(256) void augment_images_kernel(const S* __restrict__ src, long long sn, long long sc,
                                                             long long sh, long long sw, void* __restrict__ dst,
                                                             const float* __restrict__ table, int Hp, int Wp, int h,
                                                             int w, float fill) {
  __shared__ float lut[256];
  if constexpr (sizeof(S) == 1) {
    lut[threadIdx.x] = (float)threadIdx.x / 255.f;
    __syncthreads();
  }
  const int n = blockIdx.y;
  const float* t = table + (long long)n * kAugTable;  // workgroup-uniform: scalar loads
  const float ia = t[6], ib = t[7], ic = t[8], id = t[9], ie = t[10], ig = t[11];
  const float dh = t[12], gs = t[13], gv = t[14];
  const bool colour = !(dh == 0.f && gs == 1.f && gv == 1.f);
  const int Wq = Wp >> 2;
  const long long nq = (long long)Hp * Wq;
  const long long q0 = (long long)blockIdx.x * 256;
  const long long q = q0 + threadIdx.x;
  if (q >= nq) return;
  const int y = (int)(q / Wq);
  const int xq = (int)(q - (long long)y * Wq) * 4;
  float o[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) o[i] = 0.f;
  // q0 / Wq is the first row of this workgroup: past the content's last row -> padding only, zeros
  if ((int)(q0 / Wq) < h && y < h) {
    const S* img = src + (long long)n * sn;
    const float yc = (float)y + 0.5f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = xq + j;
      if (x >= w) continue;
      const float xc = (float)x + 0.5f;
      // unfused, in the reference's order: (ia xc + ib yc) + ic
      const float u = __fadd_rn(__fadd_rn(__fmul_rn(ia, xc), __fmul_rn(ib, yc)), ic);
      const float v = __fadd_rn(__fadd_rn(__fmul_rn(id, xc), __fmul_rn(ie, yc)), ig);
      const float fx = u - 0.5f, fy = v - 0.5f;
      const float flx = floorf(fx), fly = floorf(fy);
      // no tap inside the content rectangle (also NaN / huge coordinates): fill, no colour
      if (!(flx >= -1.f && flx <= (float)(w - 1) && fly >= -1.f && fly <= (float)(h - 1))) {
        o[3 * j] = o[3 * j + 1] = o[3 * j + 2] = fill;
        continue;
      }
      const float ax = fx - flx, ay = fy - fly;
      const int xi = (int)flx, yi = (int)fly;  // in [-1, w-1] x [-1, h-1]
      const bool vx0 = xi >= 0, vx1 = xi + 1 <= w - 1;
      const bool vy0 = yi >= 0, vy1 = yi + 1 <= h - 1;
      const float w00 = (1.f - ax) * (1.f - ay), w01 = ax * (1.f - ay);
      const float w10 = (1.f - ax) * ay, w11 = ax * ay;
      const long long off = (long long)yi * sh + (long long)xi * sw;
      float px[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const S* p = img + c * sc + off;
        const float p00 = vx0 && vy0 ? aug_tap<S>(p, lut) : fill;
        const float p01 = vx1 && vy0 ? aug_tap<S>(p + sw, lut) : fill;
        const float p10 = vx0 && vy1 ? aug_tap<S>(p + sh, lut) : fill;
        const float p11 = vx1 && vy1 ? aug_tap<S>(p + sh + sw, lut) : fill;
        px[c] = p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11;
      }
      if (colour) aug_hsv(px[0], px[1], px[2], dh, gs, gv);
      o[3 * j] = px[0];
      o[3 * j + 1] = px[1];
      o[3 * j + 2] = px[2];
    }
  }
  const long long e = ((long long)n * nq + q) * 12;  // element offset of this lane's 4 pixels x 3 channels
  if constexpr (BF16) {
    uint2* d2 = reinterpret_cast<uint2*>(static_cast<uint16_t*>(dst) + e);
#pragma unroll
    for (int i = 0; i < 3; ++i)
      d2[i] = make_uint2(pack2bf(o[4 * i], o[4 * i + 1]), pack2bf(o[4 * i + 2], o[4 * i + 3]));
  } else {
    float4* d4 = reinterpret_cast<float4*>(static_cast<float*>(dst) + e);
#pragma unroll
    for (int i = 0; i < 3; ++i) d4[i] = make_float4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
  }
}

// One wave per image.  Slot j of round r is r * 64 + lane; survivors of a
// round land at base + (kept lanes below this one), base = survivors so far.
__global__ __launch_bounds__(64) void augment_boxes_kernel(const float4* __restrict__ boxes,
                                                           const long long* __restrict__ labels,
                                                           const int32_t* __restrict__ n_valid,
                                                           const float* __restrict__ table, int M, int Hp, int Wp,
                                                           int h, int w, float4* __restrict__ boxes_out,
                                                           long long* __restrict__ labels_out,
                                                           int32_t* __restrict__ n_valid_out) {
  const int n = blockIdx.x;
  const int lane = threadIdx.x;
  const float* t = table + (long long)n * kAugTable;
  const float fa = t[0], fb = t[1], fc = t[2], fd = t[3], fe = t[4], ff = t[5], s = t[15];
  const int nv = min(max(n_valid[n], 0), M);
  const long long row = (long long)n * M;
  const float fw = (float)w, fh = (float)h, fWp = (float)Wp, fHp = (float)Hp;
  int base = 0;
  for (int j0 = 0; j0 < M; j0 += 64) {
    const int j = j0 + lane;
    bool keep = false;
    float4 ob = make_float4(0.f, 0.f, 0.f, 0.f);
    long long lab = 0;
    if (j < nv) {
      const float4 bx = boxes[row + j];
      lab = labels[row + j];
      const float x1 = (bx.x - 0.5f * bx.z) * fWp, x2 = (bx.x + 0.5f * bx.z) * fWp;
      const float y1 = (bx.y - 0.5f * bx.w) * fHp, y2 = (bx.y + 0.5f * bx.w) * fHp;
      const float X1 = fa * x1 + fb * y1 + fc, X2 = fa * x2 + fb * y2 + fc;
      const float Y1 = fd * x1 + fe * y1 + ff, Y2 = fd * x2 + fe * y2 + ff;
      const float nx1 = fminf(fmaxf(fminf(X1, X2), 0.f), fw), nx2 = fminf(fmaxf(fmaxf(X1, X2), 0.f), fw);
      const float ny1 = fminf(fmaxf(fminf(Y1, Y2), 0.f), fh), ny2 = fminf(fmaxf(fmaxf(Y1, Y2), 0.f), fh);
      const float nw = nx2 - nx1, nh = ny2 - ny1;
      const float area_old = (x2 - x1) * (y2 - y1) * (s * s);
      keep = nw >= 2.f && nh >= 2.f && fmaxf(nw, nh) < 100.f * fminf(nw, nh) && nw * nh > 0.1f * area_old;
      ob = make_float4((nx1 + nx2) * 0.5f / fWp, (ny1 + ny2) * 0.5f / fHp, nw / fWp, nh / fHp);
    }
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int pos = base + mbcnt(m);
      boxes_out[row + pos] = ob;
      labels_out[row + pos] = lab;
    }
    base += __popcll(m);
  }
  for (int j = base + lane; j < M; j += 64) {  // criterion.PAD_BOX, label 0
    boxes_out[row + j] = make_float4(0.5f, 0.5f, 0.1f, 0.1f);
    labels_out[row + j] = 0;
  }
  if (lane == 0) n_valid_out[n] = base;
}

// total[0] = sum of n_valid[0..B), B <= 1024: one workgroup, integer sums in a fixed order
__global__ __launch_bounds__(1024) void augment_total_kernel(const int32_t* __restrict__ n_valid, int B,
                                                             float* __restrict__ total) {
  __shared__ int part[16];
  int v = (int)threadIdx.x < B ? n_valid[threadIdx.x] : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int i = 0; i < 16; ++i) sum += part[i];
    total[0] = (float)sum;
  }
}

}  // namespace moe

using namespace moe;

extern "C" int train_augment_images(const void* src, int src_dtype, long long sn, long long sc, long long sh,
                                    long long sw, void* dst, int dst_dtype, const float* table, int B, int Hp, int Wp,
                                    int h, int w, float fill, hipStream_t stream) {
  if (src == nullptr || dst == nullptr || table == nullptr) return fail("train_augment_images: NULL operand");
  if (src_dtype != 0 && src_dtype != 1) return fail("train_augment_images: src_dtype must be 0 (uint8) or 1 (fp32)");
  if (dst_dtype != 0 && dst_dtype != 1) return fail("train_augment_images: dst_dtype must be 0 (bf16) or 1 (fp32)");
  if (B < 1 || B > 65535 || Hp < 1 || Wp < 1 || h < 1 || w < 1 || h > Hp || w > Wp)
    return fail("train_augment_images: need 1 <= B <= 65535 and a content rectangle 1 <= h <= Hp, 1 <= w <= Wp");
  if (Wp % 4) return fail("train_augment_images: Wp must be a multiple of 4 (four pixels per lane)");
  if (reinterpret_cast<uintptr_t>(dst) % 16) return fail("train_augment_images: dst must be 16-B aligned");
  if (src_dtype == 1 && reinterpret_cast<uintptr_t>(src) % 4) return fail("train_augment_images: misaligned fp32 src");
  if (sn < 0 || sc < 0 || sh < 0 || sw < 0) return fail("train_augment_images: negative source stride");
  const long long nq = (long long)Hp * (Wp / 4);
  const long long blocks = (nq + 255) / 256;
  if (blocks > 0x7fffffffLL) return fail("train_augment_images: image too large");
  const double px = (double)B * Hp * Wp * 3;
  // bytes: every source element once (the taps of neighbouring pixels overlap) + the destination
  ProfScope prof(stream, PROF_AUGMENT, (double)B * h * w * 3 * (src_dtype ? 4 : 1) + px * (dst_dtype ? 4 : 2));
  const dim3 grid((unsigned)blocks, (unsigned)B), block(256);
#define AUG_LAUNCH(S, BF)                                                                                      \
  MOE_LAUNCH(prof, (augment_images_kernel<S, BF>), grid, block, 0, stream, static_cast<const S*>(src), sn, sc, \
             sh, sw, dst, table, Hp, Wp, h, w, fill)
  if (src_dtype == 0 && dst_dtype == 0) AUG_LAUNCH(uint8_t, true);
  else if (src_dtype == 0) AUG_LAUNCH(uint8_t, false);
  else if (dst_dtype == 0) AUG_LAUNCH(float, true);
  else AUG_LAUNCH(float, false);
#undef AUG_LAUNCH
  return check_launch("train_augment_images");
}

extern "C" int train_augment_boxes(const float* boxes, const int64_t* labels, const int32_t* n_valid,
                                   const float* table, int B, int M, int Hp, int Wp, int h, int w, float* boxes_out,
                                   int64_t* labels_out, int32_t* n_valid_out, float* total_out, hipStream_t stream) {
  if (boxes == nullptr || labels == nullptr || n_valid == nullptr || table == nullptr || boxes_out == nullptr ||
      labels_out == nullptr || n_valid_out == nullptr || total_out == nullptr)
    return fail("train_augment_boxes: NULL operand");
  if (M < 1 || M > 1024) return fail("train_augment_boxes: M must lie in 1..1024 (one wave per image)");
  if (B < 1 || B > 1024) return fail("train_augment_boxes: B must lie in 1..1024 (one workgroup sums the counts)");
  if (Hp < 1 || Wp < 1 || h < 1 || w < 1 || h > Hp || w > Wp)
    return fail("train_augment_boxes: need a content rectangle 1 <= h <= Hp, 1 <= w <= Wp");
  if (reinterpret_cast<uintptr_t>(boxes) % 16 || reinterpret_cast<uintptr_t>(boxes_out) % 16)
    return fail("train_augment_boxes: boxes and boxes_out must be 16-B aligned");
  if (reinterpret_cast<uintptr_t>(labels) % 8 || reinterpret_cast<uintptr_t>(labels_out) % 8)
    return fail("train_augment_boxes: labels and labels_out must be 8-B aligned");
  if (boxes == boxes_out || labels == labels_out || n_valid == n_valid_out)
    return fail("train_augment_boxes: in-place compaction is not supported (outputs must not alias inputs)");
  {
    ProfScope prof(stream, PROF_AUGMENT, (double)B * (M * 48.0 + 8.0 + 4.0 * kAugTable));
    MOE_LAUNCH(prof, augment_boxes_kernel, dim3(B), dim3(64), 0, stream, reinterpret_cast<const float4*>(boxes),
               reinterpret_cast<const long long*>(labels), n_valid, table, M, Hp, Wp, h, w,
               reinterpret_cast<float4*>(boxes_out), reinterpret_cast<long long*>(labels_out), n_valid_out);
    if (int rc = check_launch("train_augment_boxes")) return rc;
  }
  ProfScope prof(stream, PROF_AUGMENT, 4.0 * B + 4.0);
  MOE_LAUNCH(prof, augment_total_kernel, dim3(1), dim3(1024), 0, stream,
             static_cast<const int32_t*>(n_valid_out), B, total_out);
  return check_launch("train_augment_boxes (total)");
}
