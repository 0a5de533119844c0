// Camera-motion compensation for engine.track (TrackArgs.cmc): the global
// shift of a frame against its predecessor, motion.shift_reference /
// motion.sequence_shifts bit for bit (the rule is stated in motion.py).
//
// Three launches per batch, whatever F is; all sums are integers, so their
// order does not matter and nothing is a floating-point reduction:
//   1. motion_grey_kernel, grid (x tiles, y tiles, F), a thread per 4x4 pixel
//      block: the frame's grey image and coarse image into the workspace
//      (work image f).  Every workgroup finds its frame's place in the launch
//      from frame_slot[] (its nearest earlier frame of the same slot, whether a
//      later one exists, the slot's first frame); the workgroups of a slot's
//      LAST frame also move the slot's stored image into work image F + slot
//      if the slot's first frame needs it as its predecessor, and then store
//      their own as the slot's new image -- the same thread reads and then
//      writes the same bytes, so the launch has no other reader of them.
//      Workgroup (0, 0, f) writes the frame's plan (has a predecessor, which
//      work image it is, last of its slot, the slot) and zeroes its sums.
//   2. motion_coarse_kernel, grid (bands of 8 window rows, F), a thread per
//      shift (dx, dy) in [-R, R]^2: the band of the current coarse image and
//      the band + R rows above and below of the predecessor's stand in LDS;
//      every thread walks the band for its shifts with v_sad_u8 on four packed
//      bytes (the predecessor's bytes brought into line by a 64-bit shift of
//      two neighbouring LDS words) and adds its sum to the frame's SAD table
//      with one integer atomic per shift and band.
//   3. motion_fine_kernel, grid (bands of 8 window rows, F): every workgroup
//      picks the coarse winner from the SAD table (the rule's order as one
//      64-bit key, a minimum), applies the gate, and sums its band for the 25
//      fine shifts around 4 x the winner: the band of the grey image and the
//      band + 2 rows and columns of the predecessor's stand in LDS, a thread
//      per word of four pixels, 25 v_sad_u8 per word.  The band's 25 sums go
//      to the frame's table by integer atomics; the workgroup that arrives
//      last at the frame's ticket (agent-scope release before the ticket,
//      acquire after it, agent-scope atomic loads of the sums) picks the fine
//      winner and writes the frame's outputs.  Frames without an estimate and
//      gated frames are written by band 0.
//
// LDS, dynamic: at 704 x 1248 and radius 48 the coarse search holds 2.3 + 10.1
// KiB (band, predecessor's tile) and the fine search 9.0 + 13.5 KiB; at the
// limits (out_w 2048, radius 64) 3.8 + 20.5 KiB and 15.0 + 22.5 KiB.
#include "moe_common.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace moe {

constexpr int kMotMaxHW = 2048, kMotMaxPixels = 1 << 22, kMotMaxF = 1024, kMotMaxS = 1024;
constexpr int kMotCoarse = 33 * 33, kMotFine = 25;  // a frame's row of sums: coarse SADs, fine SADs, then the plan
constexpr int kPlanPred = kMotCoarse + kMotFine, kPlanImage = kPlanPred + 1, kPlanLast = kPlanPred + 2,
              kPlanSlot = kPlanPred + 3, kPlanTicket = kPlanPred + 4, kMotSums = kPlanPred + 7;
constexpr int kMotBand = 8, kMotMinWindow = 8;

struct MotGeom {
  int out_h, out_w, hc, wc, R, gate;
  int cx0, cw, cy0, cy1;  // the coarse window: first column, width, rows [cy0, cy1)
  int fx0, fw, fy0, fy1;  // the fine window
  int coarse_ok, fine_ok;
};

__device__ __forceinline__ int mot_quant(float v) {
  const float t = v * 255.0f + 0.5f;
  return t >= 0.f ? (int)fminf(t, 255.0f) : 0;  // NaN: 0
}

__device__ __forceinline__ uint32_t mot_grey(float r, float g, float b) {
  return (uint32_t)(77 * mot_quant(r) + 150 * mot_quant(g) + 29 * mot_quant(b) + 128) >> 8;
}

__device__ __forceinline__ unsigned long long mot_key(int sad, int dx, int dy) {
  const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  return ((unsigned long long)(uint32_t)sad << 32) | ((uint32_t)(ax + ay) << 24) | ((uint32_t)ay << 16) |
         ((uint32_t)(dy + 128) << 8) | (uint32_t)(dx + 128);
}

__device__ __forceinline__ unsigned long long mot_wave_min(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t hi = (uint32_t)__shfl_xor((int)(v >> 32), off, 64);
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

// four bytes of row ``row`` from column x on, as one word; columns >= limit read as 0
__device__ __forceinline__ uint32_t mot_word(const uint8_t* __restrict__ row, int x, int limit) {
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (x + k < limit) v |= (uint32_t)row[x + k] << (8 * k);
  return v;
}

__global__ __launch_bounds__(256) void motion_grey_kernel(
    const float* __restrict__ images, int F, int pad_h, int pad_w, int vec, const int32_t* __restrict__ frame_slot,
    const int32_t* __restrict__ frame_reset, int S, MotGeom g, uint8_t* __restrict__ prev_grey,
    uint8_t* __restrict__ prev_coarse, const int32_t* __restrict__ prev_valid, uint8_t* __restrict__ work_grey,
    uint8_t* __restrict__ work_coarse, int32_t* __restrict__ sums) {
  __shared__ int sh[3];
  const int f = blockIdx.z, tid = threadIdx.x;
  int32_t* sm = sums + (size_t)f * kMotSums;
  const bool lead = blockIdx.x == 0 && blockIdx.y == 0;
  const int s = frame_slot[f];
  if (s < 0 || s >= S) {  // nobody's frame: no estimate, nothing stored
    if (lead && tid < 7) sm[kPlanPred + tid] = tid == 3 ? -1 : 0;
    return;
  }
  if (tid == 0) {
    sh[0] = -1;       // the nearest earlier frame of the slot
    sh[1] = INT_MAX;  // the nearest later one
    sh[2] = INT_MAX;  // the slot's first frame
  }
  __syncthreads();
  for (int q = tid; q < F; q += blockDim.x) {
    if (frame_slot[q] != s) continue;
    if (q < f) atomicMax(&sh[0], q);
    if (q > f) atomicMin(&sh[1], q);
    atomicMin(&sh[2], q);
  }
  __syncthreads();
  const int pred = sh[0], first = sh[2];
  const bool last = sh[1] == INT_MAX;
  const bool stored = prev_valid[s] != 0;
  const bool need_old = last && stored && frame_reset[first] == 0;  // the first frame's predecessor is the stored image
  if (lead) {
    for (int i = tid; i < kPlanPred; i += blockDim.x) sm[i] = 0;
    if (tid == 0) {
      sm[kPlanPred] = frame_reset[f] == 0 && (pred >= 0 || stored) ? 1 : 0;
      sm[kPlanImage] = pred >= 0 ? pred : F + s;
      sm[kPlanLast] = last ? 1 : 0;
      sm[kPlanSlot] = s;
      sm[kPlanTicket] = 0;
      sm[kPlanTicket + 1] = 0;
      sm[kPlanTicket + 2] = 0;
    }
  }

  const int X = blockIdx.x * 64 + (tid & 63), Y = blockIdx.y * 4 + (tid >> 6);  // this thread's 4x4 block
  const int x0 = 4 * X, y0 = 4 * Y;
  if (x0 >= g.out_w || y0 >= g.out_h) return;
  const size_t gsz = (size_t)g.out_h * g.out_w, csz = (size_t)g.hc * g.wc;
  uint8_t* wg = work_grey + (size_t)f * gsz;
  uint8_t* og = work_grey + (size_t)(F + s) * gsz;
  uint8_t* pg = prev_grey + (size_t)s * gsz;
  const bool words = (g.out_w & 3) == 0;  // a block's four bytes of a row are one aligned word
  int sum = 0;
  for (int r = 0; r < 4; ++r) {
    const int y = y0 + r;
    if (y >= g.out_h) break;
    const float* src = images + (((size_t)f * pad_h + y) * pad_w + x0) * 3;
    float v[12];
    if (vec) {
      const float4* s4 = reinterpret_cast<const float4*>(src);
      const float4 a = s4[0], b = s4[1], c = s4[2];
      v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
      v[8] = c.x, v[9] = c.y, v[10] = c.z, v[11] = c.w;
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) v[k] = x0 + k / 3 < g.out_w ? src[k] : 0.f;
    }
    uint32_t px[4], word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      px[k] = mot_grey(v[3 * k], v[3 * k + 1], v[3 * k + 2]);
      word |= px[k] << (8 * k);
      sum += (int)px[k];
    }
    const size_t at = (size_t)y * g.out_w + x0;
    if (words) {
      *reinterpret_cast<uint32_t*>(wg + at) = word;
      if (last) {
        if (need_old) *reinterpret_cast<uint32_t*>(og + at) = *reinterpret_cast<const uint32_t*>(pg + at);
        *reinterpret_cast<uint32_t*>(pg + at) = word;
      }
    } else {
      for (int k = 0; k < 4 && x0 + k < g.out_w; ++k) {
        wg[at + k] = (uint8_t)px[k];
        if (last) {
          if (need_old) og[at + k] = pg[at + k];
          pg[at + k] = (uint8_t)px[k];
        }
      }
    }
  }
  if (X < g.wc && Y < g.hc) {  // a whole block: its coarse pixel
    const uint8_t c = (uint8_t)((sum + 8) >> 4);
    const size_t at = (size_t)Y * g.wc + X;
    work_coarse[(size_t)f * csz + at] = c;
    if (last) {
      uint8_t* pc = prev_coarse + (size_t)s * csz;
      if (need_old) work_coarse[(size_t)(F + s) * csz + at] = pc[at];
      pc[at] = c;
    }
  }
}

__global__ __launch_bounds__(256) void motion_coarse_kernel(MotGeom g, const uint8_t* __restrict__ work_coarse,
                                                            int32_t* __restrict__ sums,
                                                            int32_t* __restrict__ prev_valid) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int f = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  int32_t* sm = sums + (size_t)f * kMotSums;
  if (b == 0 && tid == 0 && sm[kPlanLast] != 0) prev_valid[sm[kPlanSlot]] = 1;  // launch 1 stored the slot's image
  if (!g.coarse_ok || sm[kPlanPred] == 0) return;
  const int R = g.R, side = 2 * R + 1;
  const int y0 = g.cy0 + b * kMotBand, nrows = min(kMotBand, g.cy1 - y0);
  if (nrows <= 0) return;
  const size_t csz = (size_t)g.hc * g.wc;
  const uint8_t* cur = work_coarse + (size_t)f * csz;
  const uint8_t* prev = work_coarse + (size_t)sm[kPlanImage] * csz;
  const int cw = (g.cw + 3) >> 2;                // words in a window row
  const int pws = (cw + (2 * R) / 4 + 2) | 1;    // words in a row of the predecessor's tile, odd: rows on other banks
  uint32_t* cur_l = lds;                         // [kMotBand][cw]
  uint32_t* prev_l = lds + kMotBand * cw;        // [kMotBand + 2 R][pws]: rows y0 - R on, columns 0 on
  for (int i = tid; i < nrows * cw; i += blockDim.x) {
    const int r = i / cw, w = i - r * cw;
    cur_l[i] = mot_word(cur + (size_t)(y0 + r) * g.wc + g.cx0, 4 * w, g.cw);
  }
  for (int i = tid; i < (nrows + 2 * R) * pws; i += blockDim.x) {
    const int r = i / pws, w = i - r * pws;
    prev_l[i] = mot_word(prev + (size_t)(y0 - R + r) * g.wc, 4 * w, g.wc);
  }
  __syncthreads();
  const int rem = g.cw & 3;
  const uint32_t tail = rem ? (1u << (8 * rem)) - 1u : ~0u;  // the window's bytes of a row's last word
  for (int sidx = tid; sidx < side * side; sidx += blockDim.x) {
    const int dy = sidx / side - R, dx = sidx % side - R;
    const int k = R - dx, kb = (k & 3) * 8;  // the window's column i is the tile's column i + k
    uint32_t acc = 0;
    for (int r = 0; r < nrows; ++r) {
      const uint32_t* prow = prev_l + (r + R - dy) * pws + (k >> 2);
      const uint32_t* crow = cur_l + r * cw;
      uint32_t lo = prow[0];
      for (int w = 0; w < cw; ++w) {
        const uint32_t hi = prow[w + 1];
        uint32_t p = (uint32_t)(((((unsigned long long)hi) << 32) | lo) >> kb);
        if (w == cw - 1) p &= tail;
        acc = __builtin_amdgcn_sad_u8(crow[w], p, acc);
        lo = hi;
      }
    }
    atomicAdd(&sm[sidx], (int)acc);
  }
}

__global__ __launch_bounds__(256) void motion_fine_kernel(MotGeom g, const uint8_t* __restrict__ work_grey,
                                                          int32_t* __restrict__ sums, int32_t* __restrict__ out_shift,
                                                          int32_t* __restrict__ out_info) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ unsigned long long wkey[4];
  __shared__ int fsum[kMotFine];
  __shared__ int is_last;
  const int f = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t* sm = sums + (size_t)f * kMotSums;
  const bool writer = b == 0 && tid == 0;
  if (!g.coarse_ok || sm[kPlanPred] == 0) {
    if (writer) {
      out_shift[2 * f] = out_shift[2 * f + 1] = 0;
      out_info[4 * f] = out_info[4 * f + 1] = out_info[4 * f + 2] = out_info[4 * f + 3] = 0;
    }
    return;
  }
  // the coarse winner
  const int R = g.R, side = 2 * R + 1;
  unsigned long long key = ~0ull;
  for (int sidx = tid; sidx < side * side; sidx += blockDim.x) {
    const unsigned long long k = mot_key(sm[sidx], sidx % side - R, sidx / side - R);
    key = k < key ? k : key;
  }
  key = mot_wave_min(key);
  if (lane == 0) wkey[wave] = key;
  if (tid < kMotFine) fsum[tid] = 0;
  __syncthreads();
  for (int w = 0; w < 4; ++w) key = wkey[w] < key ? wkey[w] : key;
  const int sadc = (int)(key >> 32), dyc = (int)((key >> 8) & 0xFF) - 128, dxc = (int)(key & 0xFF) - 128;
  const int sad0 = sm[R * side + R];
  const bool gated = (dxc != 0 || dyc != 0) && 1000ll * sadc > (long long)(1000 - g.gate) * sad0;
  if (gated || !g.fine_ok) {
    if (writer) {
      out_shift[2 * f] = out_shift[2 * f + 1] = 0;
      out_info[4 * f] = gated ? 2 : 0;
      out_info[4 * f + 1] = sad0;
      out_info[4 * f + 2] = sadc;
      out_info[4 * f + 3] = 0;
    }
    return;
  }
  // this band's 25 sums
  const int y0 = g.fy0 + b * kMotBand, nrows = min(kMotBand, g.fy1 - y0);
  const size_t gsz = (size_t)g.out_h * g.out_w;
  const uint8_t* cur = work_grey + (size_t)f * gsz;
  const uint8_t* prev = work_grey + (size_t)sm[kPlanImage] * gsz;
  const int cw = (g.fw + 3) >> 2, pws = (cw + 2) | 1;
  uint32_t* cur_l = lds;                    // [kMotBand][cw]
  uint32_t* prev_l = lds + kMotBand * cw;   // [kMotBand + 4][pws]: rows y0 - 4 dyc - 2 on, columns fx0 - 4 dxc - 2 on
  uint32_t acc[kMotFine];
#pragma unroll
  for (int i = 0; i < kMotFine; ++i) acc[i] = 0;
  if (nrows > 0) {
    const int py0 = y0 - 4 * dyc - 2, px0 = g.fx0 - 4 * dxc - 2;
    for (int i = tid; i < nrows * cw; i += blockDim.x) {
      const int r = i / cw, w = i - r * cw;
      cur_l[i] = mot_word(cur + (size_t)(y0 + r) * g.out_w + g.fx0, 4 * w, g.fw);
    }
    for (int i = tid; i < (nrows + 4) * pws; i += blockDim.x) {
      const int r = i / pws, w = i - r * pws;
      prev_l[i] = mot_word(prev + (size_t)(py0 + r) * g.out_w + px0, 4 * w, g.out_w - px0);
    }
    __syncthreads();
    const int rem = g.fw & 3;
    const uint32_t tail = rem ? (1u << (8 * rem)) - 1u : ~0u;
    for (int i = tid; i < nrows * cw; i += blockDim.x) {
      const int r = i / cw, w = i - r * cw;
      const uint32_t m = w == cw - 1 ? tail : ~0u;
      const uint32_t c = cur_l[i];
#pragma unroll
      for (int a = 0; a < 5; ++a) {  // oy = 2 - a: the tile's row r + a
        const uint32_t lo = prev_l[(r + a) * pws + w], hi = prev_l[(r + a) * pws + w + 1];
        const unsigned long long v = (((unsigned long long)hi) << 32) | lo;
#pragma unroll
        for (int e = 0; e < 5; ++e) {  // ox = 2 - e: the tile's column i + e
          uint32_t& sum = acc[(4 - a) * 5 + (4 - e)];
          sum = __builtin_amdgcn_sad_u8(c, (uint32_t)(v >> (8 * e)) & m, sum);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kMotFine; ++i) {
    int v = (int)acc[i];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0 && v != 0) atomicAdd(&fsum[i], v);
  }
  __syncthreads();
  if (tid < kMotFine && fsum[tid] != 0) atomicAdd(&sm[kMotCoarse + tid], fsum[tid]);
  // the frame's last band to arrive reads every band's sums
  __threadfence();
  __syncthreads();
  if (tid == 0) is_last = atomicAdd(&sm[kPlanTicket], 1) == (int)gridDim.x - 1;
  __syncthreads();
  if (!is_last || wave != 0) return;
  __threadfence();
  unsigned long long fk = ~0ull;
  if (lane < kMotFine) {
    const int sad = __hip_atomic_load(&sm[kMotCoarse + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    fk = mot_key(sad, 4 * dxc + lane % 5 - 2, 4 * dyc + lane / 5 - 2);
  }
  fk = mot_wave_min(fk);
  if (lane == 0) {
    out_shift[2 * f] = (int)(fk & 0xFF) - 128;
    out_shift[2 * f + 1] = (int)((fk >> 8) & 0xFF) - 128;
    out_info[4 * f] = 1;
    out_info[4 * f + 1] = sad0;
    out_info[4 * f + 2] = sadc;
    out_info[4 * f + 3] = (int)(fk >> 32);
  }
}

}  // namespace moe

using namespace moe;

extern "C" int rtdetr_frame_shift(const float* images, int F, int out_h, int out_w, int pad_h, int pad_w,
                                  const int32_t* frame_slot, const int32_t* frame_reset, int S, int radius,
                                  int gate_permille, int r0, int r1, uint8_t* prev_grey, uint8_t* prev_coarse,
                                  int32_t* prev_valid, uint8_t* work_grey, uint8_t* work_coarse, int32_t* sums,
                                  int work_images, int32_t* out_shift, int32_t* out_info, hipStream_t stream) {
  const std::string what = "rtdetr_frame_shift";
  if (F < 0 || S < 0 || F > kMotMaxF || S > kMotMaxS) return fail(what + ": need 0 <= F <= 1024 and 0 <= S <= 1024");
  if (radius < 4 || radius > 64 || radius % 4 != 0) return fail(what + ": radius must be a multiple of 4 in [4, 64]");
  if (gate_permille < 0 || gate_permille > 999) return fail(what + ": gate_permille must be in [0, 999]");
  if (out_h < 1 || out_w < 1 || out_h > pad_h || out_w > pad_w)
    return fail(what + ": need 1 <= out_h <= pad_h and 1 <= out_w <= pad_w");
  if (out_h > kMotMaxHW || out_w > kMotMaxHW || (long long)out_h * out_w > kMotMaxPixels)
    return fail(what + ": out_h and out_w must be at most 2048 with at most 2^22 pixels");
  if (F == 0) return 0;
  if (S < 1) return fail(what + ": need S >= 1 state slots with F > 0");
  if (!images || !frame_slot || !frame_reset) return fail(what + ": NULL input pointer");
  if (!prev_grey || !prev_coarse || !prev_valid) return fail(what + ": NULL state pointer");
  if (!work_grey || !work_coarse || !sums) return fail(what + ": NULL workspace pointer");
  if (!out_shift || !out_info) return fail(what + ": NULL output pointer");
  if (work_images < F + S) return fail(what + ": the workspace must hold F + S images");
  if ((reinterpret_cast<uintptr_t>(prev_grey) | reinterpret_cast<uintptr_t>(work_grey)) & 3)
    return fail(what + ": prev_grey and work_grey must be 4-byte aligned");
  MotGeom g;
  g.out_h = out_h, g.out_w = out_w, g.hc = out_h / 4, g.wc = out_w / 4, g.R = radius / 4, g.gate = gate_permille;
  r0 = std::max(r0, 0), r1 = std::min(r1, g.hc);
  g.cx0 = g.R, g.cw = g.wc - 2 * g.R, g.cy0 = std::max(g.R, r0), g.cy1 = std::min(g.hc - g.R, r1);
  g.coarse_ok = g.cw >= kMotMinWindow && g.cy1 - g.cy0 >= kMotMinWindow;
  const int M = 4 * g.R + 2;
  g.fx0 = M, g.fw = out_w - 2 * M, g.fy0 = std::max(M, 4 * r0), g.fy1 = std::min(out_h - M, 4 * r1);
  g.fine_ok = g.fw >= kMotMinWindow && g.fy1 - g.fy0 >= kMotMinWindow;
  const int vec = pad_w % 4 == 0 && (reinterpret_cast<uintptr_t>(images) & 15) == 0;
  const double px = (double)F * out_h * out_w;
  {
    ProfScope prof(stream, PROF_MOTION, px * (12.0 + 3.0 + 3.0 / 16.0));
    const dim3 grid(((out_w + 3) / 4 + 63) / 64, ((out_h + 3) / 4 + 3) / 4, F);
    MOE_LAUNCH(prof, motion_grey_kernel, grid, dim3(256), 0, stream, images, F, pad_h, pad_w, vec, frame_slot,
               frame_reset, S, g, prev_grey, prev_coarse, prev_valid, work_grey, work_coarse, sums);
  }
  {
    const int bands = g.coarse_ok ? (g.cy1 - g.cy0 + kMotBand - 1) / kMotBand : 1;
    const int cw = g.coarse_ok ? (g.cw + 3) / 4 : 1;
    const size_t shmem = 4 * ((size_t)kMotBand * cw + (size_t)(kMotBand + 2 * g.R) * ((cw + (2 * g.R) / 4 + 2) | 1));
    ProfScope prof(stream, PROF_MOTION, px / 16.0 * 2.0);
    MOE_LAUNCH(prof, motion_coarse_kernel, dim3(bands, F), dim3(256), shmem, stream, g, work_coarse, sums, prev_valid);
  }
  {
    const bool run = g.coarse_ok && g.fine_ok;
    const int bands = run ? (g.fy1 - g.fy0 + kMotBand - 1) / kMotBand : 1;
    const int cw = run ? (g.fw + 3) / 4 : 1;
    const size_t shmem = 4 * ((size_t)kMotBand * cw + (size_t)(kMotBand + 4) * ((cw + 2) | 1));
    ProfScope prof(stream, PROF_MOTION, px * 2.5 + F * 24.0);
    MOE_LAUNCH(prof, motion_fine_kernel, dim3(bands, F), dim3(256), shmem, stream, g, work_grey, sums, out_shift,
               out_info);
  }
  return check_launch("rtdetr_frame_shift");
}
