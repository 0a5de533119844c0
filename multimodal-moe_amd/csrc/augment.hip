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
//   train_mosaic_images / train_mosaic_boxes   the same two steps with a
//       four-image canvas (2w x 2h around an integer centre (xc, yc)) between
//       the batch and the output: a [B,24] table row carries the centre and
//       the four source indices (TL, TR, BL, BR; -1 = empty) behind the 16
//       columns above, whose matrices then map canvas <-> output.  Every tap
//       resolves its own quadrant, so the four taps of a sample may read four
//       images; the tap weights, the blend, the HSV step and the store are
//       the functions the plain kernel uses, so a row with one quadrant
//       (xc = w, yc = h, TL only) gives the plain kernel's bits.  The box
//       kernel walks the four sources in that order and compacts into a
//       separate output capacity M_out, which it never exceeds.
#include "moe_common.h"
#include "prof.h"

namespace moe {

constexpr int kAugTable = 16;  // floats per image: fwd 2x3, inv 2x3, dh, gs, gv, s
constexpr int kMosTable = 24;  // the same + xc, yc, four source indices (TL TR BL BR, -1 = empty), two zeros

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

// bilinear weights of the taps 00, 01, 10, 11 (x fastest) at the fractions (ax, ay)
__device__ __forceinline__ void aug_weights(float ax, float ay, float (&wt)[4]) {
  wt[0] = (1.f - ax) * (1.f - ay);
  wt[1] = ax * (1.f - ay);
  wt[2] = (1.f - ax) * ay;
  wt[3] = ax * ay;
}

__device__ __forceinline__ float aug_blend(float p00, float p01, float p10, float p11, const float (&wt)[4]) {
  return p00 * wt[0] + p01 * wt[1] + p10 * wt[2] + p11 * wt[3];
}

// a lane's 4 pixels x 3 channels to element offset e of the channels_last destination
template <bool BF16>
__device__ __forceinline__ void aug_store(void* __restrict__ dst, long long e, const float (&o)[12]) {
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
      float wt[4];
      aug_weights(ax, ay, wt);
      const long long off = (long long)yi * sh + (long long)xi * sw;
      float px[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const S* p = img + c * sc + off;
        const float p00 = vx0 && vy0 ? aug_tap<S>(p, lut) : fill;
        const float p01 = vx1 && vy0 ? aug_tap<S>(p + sw, lut) : fill;
        const float p10 = vx0 && vy1 ? aug_tap<S>(p + sh, lut) : fill;
        const float p11 = vx1 && vy1 ? aug_tap<S>(p + sh + sw, lut) : fill;
        px[c] = aug_blend(p00, p01, p10, p11, wt);
      }
      if (colour) aug_hsv(px[0], px[1], px[2], dh, gs, gv);
      o[3 * j] = px[0];
      o[3 * j + 1] = px[1];
      o[3 * j + 2] = px[2];
    }
  }
  aug_store<BF16>(dst, ((long long)n * nq + q) * 12, o);
}

// A source index of a mosaic table row: an integer-valued float in [0, B_src), anything else
// (-1, NaN, an index past the batch) is an empty quadrant, so a bad table reads nothing
__device__ __forceinline__ int mos_index(float f, int B_src) { return f >= 0.f && f < (float)B_src ? (int)f : -1; }

// The mosaic centre, clamped so that the integer arithmetic around it cannot overflow whatever the table holds
__device__ __forceinline__ int mos_centre(float f) { return (int)fminf(fmaxf(f, -1.0e9f), 1.0e9f); }

// Canvas column (or row) X against the centre c of a quadrant pair of extent len: the source coordinate in
// the near (X < c) or far quadrant, and whether the tap lies on the canvas [0, 2 len) and in that image
__device__ __forceinline__ void mos_axis(int X, int c, int len, int& s, bool& far, bool& ok) {
  far = X >= c;
  s = X - (far ? c : c - len);
  ok = X >= 0 && X < 2 * len && s >= 0 && s < len;
}

template <typename S, bool BF16>
__global__ __launch_bounds__(256) void mosaic_images_kernel(const S* __restrict__ src, long long sn, long long sc,
                                                            long long sh, long long sw, int B_src,
                                                            void* __restrict__ dst, const float* __restrict__ table,
                                                            int Hp, int Wp, int h, int w, float fill) {
  __shared__ float lut[256];
  if constexpr (sizeof(S) == 1) {
    lut[threadIdx.x] = (float)threadIdx.x / 255.f;
    __syncthreads();
  }
  const int n = blockIdx.y;
  const float* t = table + (long long)n * kMosTable;  // workgroup-uniform: scalar loads
  const float ia = t[6], ib = t[7], ic = t[8], id = t[9], ie = t[10], ig = t[11];
  const float dh = t[12], gs = t[13], gv = t[14];
  const bool colour = !(dh == 0.f && gs == 1.f && gv == 1.f);
  const int cx = mos_centre(t[16]), cy = mos_centre(t[17]);
  const int qTL = mos_index(t[18], B_src), qTR = mos_index(t[19], B_src);
  const int qBL = mos_index(t[20], B_src), qBR = mos_index(t[21], B_src);
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
  if ((int)(q0 / Wq) < h && y < h) {
    const float yc = (float)y + 0.5f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = xq + j;
      if (x >= w) continue;
      const float xc = (float)x + 0.5f;
      // unfused, in the reference's order: (ia xc + ib yc) + ic -> canvas coordinates
      const float u = __fadd_rn(__fadd_rn(__fmul_rn(ia, xc), __fmul_rn(ib, yc)), ic);
      const float v = __fadd_rn(__fadd_rn(__fmul_rn(id, xc), __fmul_rn(ie, yc)), ig);
      const float fx = u - 0.5f, fy = v - 0.5f;
      const float flx = floorf(fx), fly = floorf(fy);
      // no tap on the canvas (also NaN / huge coordinates): fill, no colour
      if (!(flx >= -1.f && flx <= (float)(2 * w - 1) && fly >= -1.f && fly <= (float)(2 * h - 1))) {
        o[3 * j] = o[3 * j + 1] = o[3 * j + 2] = fill;
        continue;
      }
      const float ax = fx - flx, ay = fy - fly;
      const int X0 = (int)flx, Y0 = (int)fly;  // in [-1, 2w-1] x [-1, 2h-1]
      int sx0, sx1, sy0, sy1;
      bool rx0, rx1, by0, by1, vx0, vx1, vy0, vy1;
      mos_axis(X0, cx, w, sx0, rx0, vx0);
      mos_axis(X0 + 1, cx, w, sx1, rx1, vx1);
      mos_axis(Y0, cy, h, sy0, by0, vy0);
      mos_axis(Y0 + 1, cy, h, sy1, by1, vy1);
      // each tap's own quadrant: bottom ? (right ? BR : BL) : (right ? TR : TL)
      const int i00 = by0 ? (rx0 ? qBR : qBL) : (rx0 ? qTR : qTL);
      const int i01 = by0 ? (rx1 ? qBR : qBL) : (rx1 ? qTR : qTL);
      const int i10 = by1 ? (rx0 ? qBR : qBL) : (rx0 ? qTR : qTL);
      const int i11 = by1 ? (rx1 ? qBR : qBL) : (rx1 ? qTR : qTL);
      const bool k00 = vx0 && vy0 && i00 >= 0, k01 = vx1 && vy0 && i01 >= 0;
      const bool k10 = vx0 && vy1 && i10 >= 0, k11 = vx1 && vy1 && i11 >= 0;
      if (!(k00 || k01 || k10 || k11)) {  // no valid tap: fill, no colour
        o[3 * j] = o[3 * j + 1] = o[3 * j + 2] = fill;
        continue;
      }
      float wt[4];
      aug_weights(ax, ay, wt);
      // an invalid tap is never dereferenced; its offset may be anything
      const long long o00 = (long long)i00 * sn + (long long)sy0 * sh + (long long)sx0 * sw;
      const long long o01 = (long long)i01 * sn + (long long)sy0 * sh + (long long)sx1 * sw;
      const long long o10 = (long long)i10 * sn + (long long)sy1 * sh + (long long)sx0 * sw;
      const long long o11 = (long long)i11 * sn + (long long)sy1 * sh + (long long)sx1 * sw;
      float px[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const S* p = src + c * sc;
        const float p00 = k00 ? aug_tap<S>(p + o00, lut) : fill;
        const float p01 = k01 ? aug_tap<S>(p + o01, lut) : fill;
        const float p10 = k10 ? aug_tap<S>(p + o10, lut) : fill;
        const float p11 = k11 ? aug_tap<S>(p + o11, lut) : fill;
        px[c] = aug_blend(p00, p01, p10, p11, wt);
      }
      if (colour) aug_hsv(px[0], px[1], px[2], dh, gs, gv);
      o[3 * j] = px[0];
      o[3 * j + 1] = px[1];
      o[3 * j + 2] = px[2];
    }
  }
  aug_store<BF16>(dst, ((long long)n * nq + q) * 12, o);
}

// A box (xyxy in px, frame of the forward matrix's input) through table row t: both corners mapped, min /
// max, clipped to the content rectangle; kept by box_candidates' test in its division-free form, against
// the incoming area times s^2.  ob: the new box, cxcywh normalised to the padded tensor.
__device__ __forceinline__ bool aug_box_map(float x1, float y1, float x2, float y2, const float* __restrict__ t,
                                            float fw, float fh, float fWp, float fHp, float4& ob) {
  const float fa = t[0], fb = t[1], fc = t[2], fd = t[3], fe = t[4], ff = t[5], s = t[15];
  const float X1 = fa * x1 + fb * y1 + fc, X2 = fa * x2 + fb * y2 + fc;
  const float Y1 = fd * x1 + fe * y1 + ff, Y2 = fd * x2 + fe * y2 + ff;
  const float nx1 = fminf(fmaxf(fminf(X1, X2), 0.f), fw), nx2 = fminf(fmaxf(fmaxf(X1, X2), 0.f), fw);
  const float ny1 = fminf(fmaxf(fminf(Y1, Y2), 0.f), fh), ny2 = fminf(fmaxf(fmaxf(Y1, Y2), 0.f), fh);
  const float nw = nx2 - nx1, nh = ny2 - ny1;
  const float area_old = (x2 - x1) * (y2 - y1) * (s * s);
  ob = make_float4((nx1 + nx2) * 0.5f / fWp, (ny1 + ny2) * 0.5f / fHp, nw / fWp, nh / fHp);
  return nw >= 2.f && nh >= 2.f && fmaxf(nw, nh) < 100.f * fminf(nw, nh) && nw * nh > 0.1f * area_old;
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
      keep = aug_box_map(x1, y1, x2, y2, t, fw, fh, fWp, fHp, ob);
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

// One wave per OUTPUT image: the quadrants in the order TL, TR, BL, BR, within a quadrant the source image's
// valid slots in rounds of 64.  A box goes to content px, is shifted by its quadrant's origin, clipped to the
// canvas (the area the keep test refers to is the clipped one) and mapped like a plain box.  Survivors land
// at base + (kept lanes below); nothing is written at or past M_out, and the count is clamped there.
__global__ __launch_bounds__(64) void mosaic_boxes_kernel(const float4* __restrict__ boxes,
                                                          const long long* __restrict__ labels,
                                                          const int32_t* __restrict__ n_valid,
                                                          const float* __restrict__ table, int B, int M_in, int M_out,
                                                          int Hp, int Wp, int h, int w, float4* __restrict__ boxes_out,
                                                          long long* __restrict__ labels_out,
                                                          int32_t* __restrict__ n_valid_out) {
  const int n = blockIdx.x;
  const int lane = threadIdx.x;
  const float* t = table + (long long)n * kMosTable;
  const int cx = mos_centre(t[16]), cy = mos_centre(t[17]);
  const long long row_out = (long long)n * M_out;
  const float fw = (float)w, fh = (float)h, fWp = (float)Wp, fHp = (float)Hp;
  int base = 0;
  for (int quad = 0; quad < 4; ++quad) {
    const int src = mos_index(t[18 + quad], B);  // wave-uniform
    if (src < 0) continue;
    const float ox = (float)((quad & 1) ? cx : cx - w), oy = (float)((quad & 2) ? cy : cy - h);
    const int nv = min(max(n_valid[src], 0), M_in);
    const long long row = (long long)src * M_in;
    for (int j0 = 0; j0 < nv; j0 += 64) {
      const int j = j0 + lane;
      bool keep = false;
      float4 ob = make_float4(0.f, 0.f, 0.f, 0.f);
      long long lab = 0;
      if (j < nv) {
        const float4 bx = boxes[row + j];
        lab = labels[row + j];
        float x1 = (bx.x - 0.5f * bx.z) * fWp, x2 = (bx.x + 0.5f * bx.z) * fWp;
        float y1 = (bx.y - 0.5f * bx.w) * fHp, y2 = (bx.y + 0.5f * bx.w) * fHp;
        x1 = fminf(fmaxf(x1 + ox, 0.f), 2.f * fw);
        x2 = fminf(fmaxf(x2 + ox, 0.f), 2.f * fw);
        y1 = fminf(fmaxf(y1 + oy, 0.f), 2.f * fh);
        y2 = fminf(fmaxf(y2 + oy, 0.f), 2.f * fh);
        keep = aug_box_map(x1, y1, x2, y2, t, fw, fh, fWp, fHp, ob);
      }
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const int pos = base + mbcnt(m);
        if (pos < M_out) {
          boxes_out[row_out + pos] = ob;
          labels_out[row_out + pos] = lab;
        }
      }
      base += __popcll(m);
    }
  }
  base = min(base, M_out);
  for (int j = base + lane; j < M_out; j += 64) {  // criterion.PAD_BOX, label 0
    boxes_out[row_out + j] = make_float4(0.5f, 0.5f, 0.1f, 0.1f);
    labels_out[row_out + j] = 0;
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

extern "C" int train_mosaic_images(const void* src, int src_dtype, long long sn, long long sc, long long sh,
                                   long long sw, int B_src, void* dst, int dst_dtype, const float* table, int B,
                                   int Hp, int Wp, int h, int w, float fill, hipStream_t stream) {
  if (src == nullptr || dst == nullptr || table == nullptr) return fail("train_mosaic_images: NULL operand");
  if (src_dtype != 0 && src_dtype != 1) return fail("train_mosaic_images: src_dtype must be 0 (uint8) or 1 (fp32)");
  if (dst_dtype != 0 && dst_dtype != 1) return fail("train_mosaic_images: dst_dtype must be 0 (bf16) or 1 (fp32)");
  if (B < 1 || B > 65535 || B_src < 1 || B_src > 65535 || Hp < 1 || Wp < 1 || h < 1 || w < 1 || h > Hp || w > Wp)
    return fail("train_mosaic_images: need 1 <= B, B_src <= 65535 and a content rectangle 1 <= h <= Hp, 1 <= w <= Wp");
  if (h > 0x3fffffff || w > 0x3fffffff) return fail("train_mosaic_images: image too large");
  if (Wp % 4) return fail("train_mosaic_images: Wp must be a multiple of 4 (four pixels per lane)");
  if (reinterpret_cast<uintptr_t>(dst) % 16) return fail("train_mosaic_images: dst must be 16-B aligned");
  if (reinterpret_cast<uintptr_t>(src) == reinterpret_cast<uintptr_t>(dst))
    return fail("train_mosaic_images: dst must not alias src");
  if (src_dtype == 1 && reinterpret_cast<uintptr_t>(src) % 4) return fail("train_mosaic_images: misaligned fp32 src");
  if (sn < 0 || sc < 0 || sh < 0 || sw < 0) return fail("train_mosaic_images: negative source stride");
  const long long nq = (long long)Hp * (Wp / 4);
  const long long blocks = (nq + 255) / 256;
  if (blocks > 0x7fffffffLL) return fail("train_mosaic_images: image too large");
  const double px = (double)B * Hp * Wp * 3;
  // bytes: as train_augment_images (an output image reads about one source image's worth of taps)
  ProfScope prof(stream, PROF_AUGMENT, (double)B * h * w * 3 * (src_dtype ? 4 : 1) + px * (dst_dtype ? 4 : 2));
  const dim3 grid((unsigned)blocks, (unsigned)B), block(256);
#define MOS_LAUNCH(S, BF)                                                                                     \
  MOE_LAUNCH(prof, (mosaic_images_kernel<S, BF>), grid, block, 0, stream, static_cast<const S*>(src), sn, sc, \
             sh, sw, B_src, dst, table, Hp, Wp, h, w, fill)
  if (src_dtype == 0 && dst_dtype == 0) MOS_LAUNCH(uint8_t, true);
  else if (src_dtype == 0) MOS_LAUNCH(uint8_t, false);
  else if (dst_dtype == 0) MOS_LAUNCH(float, true);
  else MOS_LAUNCH(float, false);
#undef MOS_LAUNCH
  return check_launch("train_mosaic_images");
}

extern "C" int train_mosaic_boxes(const float* boxes, const int64_t* labels, const int32_t* n_valid,
                                  const float* table, int B, int M_in, int M_out, int Hp, int Wp, int h, int w,
                                  float* boxes_out, int64_t* labels_out, int32_t* n_valid_out, float* total_out,
                                  hipStream_t stream) {
  if (boxes == nullptr || labels == nullptr || n_valid == nullptr || table == nullptr || boxes_out == nullptr ||
      labels_out == nullptr || n_valid_out == nullptr || total_out == nullptr)
    return fail("train_mosaic_boxes: NULL operand");
  if (M_in < 1 || M_in > 1024 || M_out < 1 || M_out > 1024)
    return fail("train_mosaic_boxes: M_in and M_out must lie in 1..1024 (one wave per image)");
  if (B < 1 || B > 1024) return fail("train_mosaic_boxes: B must lie in 1..1024 (one workgroup sums the counts)");
  if (Hp < 1 || Wp < 1 || h < 1 || w < 1 || h > Hp || w > Wp)
    return fail("train_mosaic_boxes: need a content rectangle 1 <= h <= Hp, 1 <= w <= Wp");
  if (h > 0x3fffffff || w > 0x3fffffff) return fail("train_mosaic_boxes: image too large");
  if (reinterpret_cast<uintptr_t>(boxes) % 16 || reinterpret_cast<uintptr_t>(boxes_out) % 16)
    return fail("train_mosaic_boxes: boxes and boxes_out must be 16-B aligned");
  if (reinterpret_cast<uintptr_t>(labels) % 8 || reinterpret_cast<uintptr_t>(labels_out) % 8)
    return fail("train_mosaic_boxes: labels and labels_out must be 8-B aligned");
  if (boxes == boxes_out || labels == labels_out || n_valid == n_valid_out)
    return fail("train_mosaic_boxes: in-place compaction is not supported (outputs must not alias inputs)");
  {
    ProfScope prof(stream, PROF_AUGMENT, (double)B * (4.0 * M_in * 24.0 + M_out * 24.0 + 8.0 + 4.0 * kMosTable));
    MOE_LAUNCH(prof, mosaic_boxes_kernel, dim3(B), dim3(64), 0, stream, reinterpret_cast<const float4*>(boxes),
               reinterpret_cast<const long long*>(labels), n_valid, table, B, M_in, M_out, Hp, Wp, h, w,
               reinterpret_cast<float4*>(boxes_out), reinterpret_cast<long long*>(labels_out), n_valid_out);
    if (int rc = check_launch("train_mosaic_boxes")) return rc;
  }
  ProfScope prof(stream, PROF_AUGMENT, 4.0 * B + 4.0);
  MOE_LAUNCH(prof, augment_total_kernel, dim3(1), dim3(1024), 0, stream,
             static_cast<const int32_t*>(n_valid_out), B, total_out);
  return check_launch("train_mosaic_boxes (total)");
}
