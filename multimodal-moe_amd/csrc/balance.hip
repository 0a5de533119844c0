// Loss-free expert load balancing (Wang et al. 2024): the per-expert selection
// bias of every MoE layer, moved once per optimizer step by the sign of the
// expert's load error (src/moe/balance.py states the rule, balance_reference).
//
//   load[l][e] += hist[l][e]                                   every micro-step
// and, when `apply` (once per optimizer step, after any sum over ranks):
//   total = sum_e load[l][e]            (0: bias unchanged, maxvio 0)
//   s_e   = sign(total - E load[l][e])  exact in int64
//   bias[l][e] = fl32(bias[l][e] + s_e rate), then minus min_e of the new bias
//   maxvio[l]  = float((double)(E max_e load - total) / (double)total)
//   load[l][:] = 0
//
// One launch for all L layers: a 64-lane workgroup per layer, lane e owns
// expert e; total, max and min are wave butterflies in int64 / fp32.  No
// atomics and no order-dependent float sum: bit for bit the reference.
//
// The per-context form (moe_balance_step_ctx; bias fp32 [C, E] per layer, load
// int64 [L, C, E], maxvio [L, C]) is the same rule on every (layer, context)
// row: workgroup (c, l) counts the top-k indices of the layer's images whose
// context is c into integer LDS counters, adds them to load[l][c][:], and with
// `apply` runs the row update (balance_row_apply, shared with the per-expert
// kernel).  A row belongs to one workgroup and every sum is an integer sum, so
// the result does not depend on the order the workgroups run in.
#include <climits>
#include <cmath>

#include "moe_common.h"
#include "prof.h"

namespace moe {

struct BalanceLayer {  // 16 B, mirrored by src/moe/balance.py
  const int32_t* hist;  // int32 [E] of the layer's last forward, or nullptr (nothing to add)
  float* bias;          // fp32 [E] the layer's selection bias
};
static_assert(sizeof(BalanceLayer) == 16, "BalanceLayer layout");

// The rule on one row, by one full 64-lane wave: lane e owns expert e and holds its summed load v (0 for
// e >= E).  Zeroes the row's load, moves and recentres the row's bias, writes the row's max violation.
__device__ __forceinline__ void balance_row_apply(long long v, int e, int E, long long* __restrict__ load_row,
                                                  float* __restrict__ bias_row, float rate,
                                                  float* __restrict__ maxvio_out) {
  const bool own = e < E;
  long long total = v;
  long long mx = own ? v : LLONG_MIN;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    total += __shfl_xor(total, o, 64);
    const long long om = __shfl_xor(mx, o, 64);
    mx = om > mx ? om : mx;
  }
  if (own) load_row[e] = 0;
  if (total == 0) {  // wave-uniform
    if (e == 0 && maxvio_out != nullptr) *maxvio_out = 0.f;
    return;
  }
  const long long err = total - (long long)E * v;
  const float s = err > 0 ? 1.f : (err < 0 ? -1.f : 0.f);
  const float b = own ? bias_row[e] + s * rate : INFINITY;  // (s rate is exact: a contraction changes nothing)
  float mn = b;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
  if (own) bias_row[e] = b - mn;
  if (e == 0 && maxvio_out != nullptr) *maxvio_out = (float)((double)((long long)E * mx - total) / (double)total);
}

__global__ __launch_bounds__(64) void balance_step_kernel(const BalanceLayer* __restrict__ tab, int E,
                                                          long long* __restrict__ load, float rate, int apply,
                                                          float* __restrict__ maxvio) {
  const int l = blockIdx.x;
  const int e = threadIdx.x;
  const bool own = e < E;
  const BalanceLayer rec = tab[l];
  long long v = 0;
  if (own) {
    v = load[(size_t)l * E + e];
    if (rec.hist != nullptr) v += rec.hist[e];
  }
  if (!apply) {
    if (own) load[(size_t)l * E + e] = v;
    return;
  }
  balance_row_apply(v, e, E, load + (size_t)l * E, rec.bias, rate, maxvio != nullptr ? maxvio + l : nullptr);
}

struct BalanceCtxLayer {  // 32 B, mirrored by src/moe/balance.py
  const int32_t* topk_idx;  // int32 [T, k] the layer's last forward's selections, or nullptr (nothing to add)
  float* bias;              // fp32 [C, E] the layer's per-context selection bias
  const int32_t* ctx_img;   // int32 [ceil(T / tokens_per_image)] the images' context ids
  int T;                    // tokens of that forward
  int tokens_per_image;
};
static_assert(sizeof(BalanceCtxLayer) == 32, "BalanceCtxLayer layout");

constexpr int kBalanceCtxThreads = 256;

// grid (C, L): workgroup (c, l) owns row (l, c) of load, bias and maxvio.  An expert id outside [0, E) and a
// context id outside [0, C) count nowhere (route_stats' convention).
__global__ __launch_bounds__(kBalanceCtxThreads) void balance_step_ctx_kernel(
    const BalanceCtxLayer* __restrict__ tab, int C, int E, int k, long long* __restrict__ load, float rate, int apply,
    float* __restrict__ maxvio) {
  constexpr int NW = kBalanceCtxThreads / 64;
  __shared__ int s_cnt[NW][64];  // a counter row per wave: a quarter of the same-address LDS adds each
  const int c = blockIdx.x, l = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const BalanceCtxLayer rec = tab[l];
  s_cnt[wave][lane] = 0;
  __syncthreads();
  if (rec.topk_idx != nullptr && rec.T > 0 && rec.tokens_per_image > 0) {
    const int tpi = rec.tokens_per_image;
    const int B = (rec.T + tpi - 1) / tpi;
    for (int b = 0; b < B; ++b) {
      if (rec.ctx_img[b] != c) continue;  // workgroup-uniform
      const int t1 = min((b + 1) * tpi, rec.T);
      const int32_t* src = rec.topk_idx + (size_t)b * tpi * k;
      const int n = (t1 - b * tpi) * k;
      for (int i = tid; i < n; i += kBalanceCtxThreads) {
        const int e = src[i];
        if ((unsigned)e < (unsigned)E) atomicAdd(&s_cnt[wave][e], 1);
      }
    }
  }
  __syncthreads();
  if (wave != 0) return;
  const int e = lane;
  const size_t row = (size_t)l * C + c;
  long long v = 0;
  if (e < E) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) n += s_cnt[w][e];
    v = load[row * E + e] + n;
  }
  if (!apply) {
    if (e < E) load[row * E + e] = v;
    return;
  }
  balance_row_apply(v, e, E, load + row * E, rec.bias + (size_t)c * E, rate, maxvio != nullptr ? maxvio + row : nullptr);
}

}  // namespace moe

using namespace moe;

extern "C" int moe_balance_step(const void* table, int L, int E, long long* load, float rate, int apply,
                                float* maxvio, hipStream_t stream) {
  if (E < 1 || E > 64) return fail("balance_step: need 1 <= E <= 64");
  if (L < 0) return fail("balance_step: L < 0");
  if (L == 0) return 0;
  if (table == nullptr || load == nullptr) return fail("balance_step: NULL pointer");
  // bytes: the load table read and written, hist read, bias read and written when applied
  ProfScope prof(stream, PROF_OPTIM, (double)L * E * (16.0 + 4.0 + (apply ? 8.0 : 0.0)));
  MOE_LAUNCH(prof, balance_step_kernel, dim3(L), dim3(64), 0, stream, static_cast<const BalanceLayer*>(table), E,
             load, rate, apply, maxvio);
  return check_launch("moe_balance_step");
}

extern "C" int moe_balance_step_ctx(const void* table, int L, int C, int E, int k, long long* load, float rate,
                                    int apply, float* maxvio, hipStream_t stream) {
  if (E < 1 || E > 64) return fail("balance_step_ctx: need 1 <= E <= 64");
  if (k < 1 || k > 8 || k > E) return fail("balance_step_ctx: need 1 <= k <= min(8, E)");
  if (C < 1) return fail("balance_step_ctx: need C >= 1");
  if (L < 0 || L > 65535) return fail("balance_step_ctx: need 0 <= L <= 65535");
  if (L == 0) return 0;
  if (table == nullptr || load == nullptr) return fail("balance_step_ctx: NULL pointer");
  // bytes: the load rows read and written, bias rows read and written when applied (the indices' size is in
  // the device table: not counted)
  ProfScope prof(stream, PROF_OPTIM, (double)L * C * E * (16.0 + (apply ? 8.0 : 0.0)));
  MOE_LAUNCH(prof, balance_step_ctx_kernel, dim3(C, L), dim3(kBalanceCtxThreads), 0, stream,
             static_cast<const BalanceCtxLayer*>(table), C, E, k, load, rate, apply, maxvio);
  return check_launch("moe_balance_step_ctx");
}
