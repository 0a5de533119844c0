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
  long long total = v;
  long long mx = own ? v : LLONG_MIN;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    total += __shfl_xor(total, o, 64);
    const long long om = __shfl_xor(mx, o, 64);
    mx = om > mx ? om : mx;
  }
  if (own) load[(size_t)l * E + e] = 0;
  if (total == 0) {  // wave-uniform
    if (e == 0 && maxvio != nullptr) maxvio[l] = 0.f;
    return;
  }
  const long long err = total - (long long)E * v;
  const float s = err > 0 ? 1.f : (err < 0 ? -1.f : 0.f);
  const float b = own ? rec.bias[e] + s * rate : INFINITY;  // (s rate is exact: a contraction changes nothing)
  float mn = b;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
  if (own) rec.bias[e] = b - mn;
  if (e == 0 && maxvio != nullptr) maxvio[l] = (float)((double)((long long)E * mx - total) / (double)total);
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
