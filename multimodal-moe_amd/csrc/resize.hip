// Inference preprocessing on the GPU (preprocess.py, engine.predict): a batch
// of decoded frames -- uint8 HWC RGB, any sizes, packed back to back in one
// buffer and described by a [B, 4] table -- resized with the antialiased
// bilinear (triangle) filter of PIL / torch's F.interpolate(antialias=True),
// scaled by 1/255, zero-padded and written as the fp32 channels-last input of
// the model, in ONE launch that writes every element of dst exactly once (no
// memset, no atomics, no workspace).
//
// Per axis (n_in -> n_out): scale = n_in / n_out, support = max(scale, 1),
// output i has centre c = scale (i + 0.5) and taps
// [max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n_in)) of weight
// max(0, 1 - |(j - c + 0.5) / support|) over their sum.  Tap ranges and weights
// are fp64 (a coordinate near 4000 has an fp32 ulp of 2.4e-4, which moves
// weights by 4e-5), rounded to fp32 once normalised; both passes accumulate in
// fp32 in ascending tap order, the intermediate stays fp32, and the result is
// a true division by 255.0f, so a frame at identity scale (weights 1 and 0)
// gives float(x) / 255.0f bit for bit.
//
// One 256-thread workgroup per 8 x 32 tile of the padded output.  The tile's
// 40 filter lines (32 columns, 8 rows) are built once in LDS; the horizontal
// pass reads the source rows of the tile's footprint from global memory
// (lanes run over (column, channel): adjacent bytes, cache lines shared by
// neighbours) into an fp32 LDS tile [rows][32 x 3]; the vertical pass reads
// that tile conflict-free and stores 384-byte rows, coalesced.  The LDS tile
// holds 80 source rows, which covers a reduction of 8 per axis (<= 17 taps,
// <= 73 rows); a slot reduced further takes the direct form -- every output
// pixel sums its taps from global memory with the same arithmetic -- which is
// correct at every scale.  Tiles of the padding, and slots whose descriptor is
// empty (h or w <= 0) or malformed, are zero-filled.
//
// rtdetr_resize_pad_u8_flip (predict(flip=True)'s mirrored passes) is the same kernel's second instantiation: a
// flag per slot, and a flagged slot reads its window's columns right to left in both forms.
#include "moe_common.h"
#include "prof.h"

namespace moe {

constexpr int kRsTW = 32, kRsTH = 8;        // output tile: columns x rows
constexpr int kRsTaps = 20;                 // taps per filter line in LDS (17 at the 8x limit)
constexpr int kRsWS = 21;                   // line stride of the fp32 weights (odd: no bank conflicts)
constexpr int kRsRows = 80;                 // source rows of the fp32 LDS tile (73 at the 8x limit)
constexpr int kRsLines = kRsTW + kRsTH;     // filter lines of a tile
constexpr int kRsRowF = kRsTW * 3;          // floats per LDS tile row
constexpr int kRsThreads = 256;
constexpr int kRsMaxReduce = 8;             // per-axis reduction the tiled form holds
constexpr long long kRsMaxSide = 16384;

struct TapLine {
  double c, inv;
  int lo, hi;
};

// taps of output index i of one axis
__device__ __forceinline__ TapLine tap_line(int i, int n_in, int n_out) {
#pragma clang fp contract(off)
  TapLine t;
  const double scale = (double)n_in / (double)n_out;
  const double support = fmax(scale, 1.0);
  t.inv = 1.0 / support;
  t.c = scale * ((double)i + 0.5);
  t.lo = max((int)(t.c - support + 0.5), 0);
  t.hi = min((int)(t.c + support + 0.5), n_in);
  return t;
}

__device__ __forceinline__ double tap_weight(int j, const TapLine& t) {
#pragma clang fp contract(off)
  const double d = ((double)j - t.c + 0.5) * t.inv;
  return fmax(0.0, 1.0 - fabs(d));
}

// one output value straight from global memory (any scale); mirror: tap j reads source column w - 1 - j
template <bool kFlip>
__device__ float resize_direct(const uint8_t* __restrict__ img, int h, int w, long long stride, int out_h, int out_w,
                               int y, int x, int ch, bool mirror) {
  const TapLine ty = tap_line(y, h, out_h), tx = tap_line(x, w, out_w);
  double sy = 0.0, sx = 0.0;
  for (int j = ty.lo; j < ty.hi; ++j) sy += tap_weight(j, ty);
  for (int j = tx.lo; j < tx.hi; ++j) sx += tap_weight(j, tx);
  float acc = 0.f;
  for (int jy = ty.lo; jy < ty.hi; ++jy) {
    const uint8_t* row = img + (long long)jy * stride + ch;
    float hacc = 0.f;
    for (int jx = tx.lo; jx < tx.hi; ++jx) {
      const int col = kFlip && mirror ? w - 1 - jx : jx;
      hacc += (float)(tap_weight(jx, tx) / sx) * (float)row[3 * (long long)col];
    }
    acc += (float)(tap_weight(jy, ty) / sy) * hacc;
  }
  return acc / 255.0f;
}

// kFlip = false is rtdetr_resize_pad_u8's kernel as it always was (``flip`` is NULL and never read); kFlip = true is
// rtdetr_resize_pad_u8_flip's: ``flip`` int32 [B], and a slot with a non-zero value (uniform over the workgroup: one
// slot per blockIdx.z) is read right to left -- wherever the unmirrored form reads column j of the descriptor's
// window it reads column w - 1 - j, with the same tap ranges, weights and order, so the slot's image is, bit for bit,
// the one the unmirrored form gives for a host-mirrored copy of the same pixels.
template <bool kFlip>
__global__ __launch_bounds__(kRsThreads) void resize_pad_u8_kernel(const uint8_t* __restrict__ src,
                                                                   const long long* __restrict__ desc, int out_h,
                                                                   int out_w, int pad_h, int pad_w,
                                                                   float* __restrict__ dst,
                                                                   const int32_t* __restrict__ flip) {
  // fp32 [kRsRows][kRsRowF] tile of the horizontal pass; before that, the raw fp64 weights [kRsLines][kRsTaps]
  __shared__ __attribute__((aligned(16))) float tile[kRsRows * kRsRowF];
  __shared__ float wts[kRsLines * kRsWS];
  __shared__ int lo_s[kRsLines], cnt_s[kRsLines];
  static_assert(sizeof(double) * kRsLines * kRsTaps <= sizeof(float) * kRsRows * kRsRowF, "raw weights fit the tile");

  const int tid = threadIdx.x, b = blockIdx.z;
  const bool mirror = kFlip && flip[b] != 0;
  const int x0 = blockIdx.x * kRsTW, y0 = blockIdx.y * kRsTH;
  const int vr = min(kRsTH, pad_h - y0), vc3 = 3 * min(kRsTW, pad_w - x0);  // the tile's part of dst
  float* __restrict__ out = dst + (((size_t)b * pad_h + y0) * pad_w + x0) * 3;
  const size_t orow = (size_t)pad_w * 3;

  const long long off = desc[4 * b], h64 = desc[4 * b + 1], w64 = desc[4 * b + 2], stride = desc[4 * b + 3];
  const bool empty = h64 <= 0 || w64 <= 0 || h64 > kRsMaxSide || w64 > kRsMaxSide || off < 0 || stride < 3 * w64;
  if (empty || x0 >= out_w || y0 >= out_h) {  // padding, or an empty slot: zeros
    for (int e = tid; e < vr * vc3; e += kRsThreads) out[(e / vc3) * orow + e % vc3] = 0.f;
    return;
  }
  const int h = (int)h64, w = (int)w64;
  const uint8_t* __restrict__ img = src + off;

  if (w64 > (long long)kRsMaxReduce * out_w || h64 > (long long)kRsMaxReduce * out_h) {  // direct form
    for (int e = tid; e < vr * vc3; e += kRsThreads) {
      const int r = e / vc3, xc = e % vc3, y = y0 + r, x = x0 + xc / 3;
      out[r * orow + xc] = (y < out_h && x < out_w) ? resize_direct<kFlip>(img, h, w, stride, out_h, out_w, y, x,
                                                                             xc % 3, mirror)
                                                    : 0.f;
    }
    return;
  }

  // filter lines: 0..31 the tile's columns, 32..39 its rows; a line outside the content has no taps
  double* raw = reinterpret_cast<double*>(tile);
  for (int it = tid; it < kRsLines * kRsTaps; it += kRsThreads) {
    const int line = it / kRsTaps, k = it % kRsTaps;
    const bool is_x = line < kRsTW;
    const int i = is_x ? x0 + line : y0 + line - kRsTW;
    const bool valid = i < (is_x ? out_w : out_h);
    const TapLine t = tap_line(valid ? i : 0, is_x ? w : h, is_x ? out_w : out_h);
    const int cnt = valid ? min(t.hi - t.lo, kRsTaps) : 0;
    raw[it] = k < cnt ? tap_weight(t.lo + k, t) : 0.0;
    if (k == 0) {
      lo_s[line] = t.lo;
      cnt_s[line] = cnt;
    }
  }
  __syncthreads();
  for (int it = tid; it < kRsLines * kRsTaps; it += kRsThreads) {
    const int line = it / kRsTaps, k = it % kRsTaps, cnt = cnt_s[line];
    double sum = 0.0;
    for (int kk = 0; kk < cnt; ++kk) sum += raw[line * kRsTaps + kk];
    wts[line * kRsWS + k] = k < cnt ? (float)(raw[it] / sum) : 0.f;
  }
  __syncthreads();  // raw is dead from here: the tile takes its place

  // source rows under the tile's content rows (tap ranges grow with the output index)
  const int last = kRsTW + min(kRsTH, out_h - y0) - 1;
  const int r0 = lo_s[kRsTW];
  const int nrows = min(lo_s[last] + cnt_s[last] - r0, kRsRows);

  // horizontal pass: tile[r][x * 3 + ch]
  for (int it = tid; it < nrows * kRsRowF; it += kRsThreads) {
    const int r = it / kRsRowF, xc = it % kRsRowF, x = xc / 3, ch = xc - 3 * x;
    const int cnt = cnt_s[x];
    // mirrored: the byte pointer starts at the window's column w - 1 - lo and steps by -3
    const uint8_t* p = img + (long long)(r0 + r) * stride + 3 * (long long)(mirror ? w - 1 - lo_s[x] : lo_s[x]) + ch;
    const float* wx = wts + x * kRsWS;
    float acc = 0.f;
    int k = 0;
    if (mirror) {
      for (; k + 4 <= cnt; k += 4) {
        const float v0 = (float)p[-3 * k], v1 = (float)p[-3 * k - 3], v2 = (float)p[-3 * k - 6],
                    v3 = (float)p[-3 * k - 9];
        acc += wx[k] * v0;
        acc += wx[k + 1] * v1;
        acc += wx[k + 2] * v2;
        acc += wx[k + 3] * v3;
      }
      for (; k < cnt; ++k) acc += wx[k] * (float)p[-3 * k];
    } else {
      for (; k + 4 <= cnt; k += 4) {  // four byte loads in flight, summed in tap order
        const float v0 = (float)p[3 * k], v1 = (float)p[3 * k + 3], v2 = (float)p[3 * k + 6], v3 = (float)p[3 * k + 9];
        acc += wx[k] * v0;
        acc += wx[k + 1] * v1;
        acc += wx[k + 2] * v2;
        acc += wx[k + 3] * v3;
      }
      for (; k < cnt; ++k) acc += wx[k] * (float)p[3 * k];
    }
    tile[it] = acc;
  }
  __syncthreads();

  // vertical pass, / 255, store
  for (int e = tid; e < kRsTH * kRsRowF; e += kRsThreads) {
    const int r = e / kRsRowF, xc = e % kRsRowF;
    if (r >= vr || xc >= vc3) continue;
    const int lo = lo_s[kRsTW + r] - r0, cnt = min(cnt_s[kRsTW + r], nrows - lo);
    const float* wy = wts + (kRsTW + r) * kRsWS;
    float acc = 0.f;
    for (int k = 0; k < cnt; ++k) acc += wy[k] * tile[(lo + k) * kRsRowF + xc];
    out[r * orow + xc] = acc / 255.0f;
  }
}

}  // namespace moe

using namespace moe;

extern "C" int rtdetr_resize_pad_u8(const uint8_t* src, const long long* desc, int B, int out_h, int out_w,
                                    int pad_h, int pad_w, float* dst, hipStream_t stream) {
  if (B < 0) return fail("rtdetr_resize_pad_u8: need B >= 0");
  if (out_h < 1 || out_w < 1) return fail("rtdetr_resize_pad_u8: need out_h >= 1 and out_w >= 1");
  if (pad_h < out_h || pad_w < out_w) return fail("rtdetr_resize_pad_u8: need pad_h >= out_h and pad_w >= out_w");
  if (B == 0) return 0;
  if (!src || !desc || !dst) return fail("rtdetr_resize_pad_u8: NULL pointer");
  const dim3 grid((pad_w + kRsTW - 1) / kRsTW, (pad_h + kRsTH - 1) / kRsTH, B);
  if (grid.y > 65535u || grid.z > 65535u) return fail("rtdetr_resize_pad_u8: need pad_h <= 524280 and B <= 65535");
  // the source sizes live in the device descriptor: the launch is priced by what it writes
  ProfScope prof(stream, PROF_RESIZE, 12.0 * pad_h * pad_w * B + 32.0 * B);
  MOE_LAUNCH(prof, resize_pad_u8_kernel<false>, grid, dim3(kRsThreads), 0, stream, src, desc, out_h, out_w, pad_h,
             pad_w, dst, (const int32_t*)nullptr);
  return check_launch("rtdetr_resize_pad_u8");
}

extern "C" int rtdetr_resize_pad_u8_flip(const uint8_t* src, const long long* desc, const int32_t* flip, int B,
                                         int out_h, int out_w, int pad_h, int pad_w, float* dst, hipStream_t stream) {
  if (B < 0) return fail("rtdetr_resize_pad_u8_flip: need B >= 0");
  if (out_h < 1 || out_w < 1) return fail("rtdetr_resize_pad_u8_flip: need out_h >= 1 and out_w >= 1");
  if (pad_h < out_h || pad_w < out_w) return fail("rtdetr_resize_pad_u8_flip: need pad_h >= out_h and pad_w >= out_w");
  if (!flip) return fail("rtdetr_resize_pad_u8_flip: NULL flip (rtdetr_resize_pad_u8 is the entry without flags)");
  if (B == 0) return 0;
  if (!src || !desc || !dst) return fail("rtdetr_resize_pad_u8_flip: NULL pointer");
  const dim3 grid((pad_w + kRsTW - 1) / kRsTW, (pad_h + kRsTH - 1) / kRsTH, B);
  if (grid.y > 65535u || grid.z > 65535u)
    return fail("rtdetr_resize_pad_u8_flip: need pad_h <= 524280 and B <= 65535");
  ProfScope prof(stream, PROF_RESIZE, 12.0 * pad_h * pad_w * B + 36.0 * B);
  MOE_LAUNCH(prof, resize_pad_u8_kernel<true>, grid, dim3(kRsThreads), 0, stream, src, desc, out_h, out_w, pad_h,
             pad_w, dst, flip);
  return check_launch("rtdetr_resize_pad_u8_flip");
}
