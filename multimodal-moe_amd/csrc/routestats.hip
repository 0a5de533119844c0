// Per-context routing statistics of one MoE layer forward (validation's
// context report, src/moe/stats.py): how often the tokens of context c went to
// expert e, with how much gate weight and router probability, and how many of
// those assignments the capacity dropped.
//
//   stats[c][e][0] += #{(t, j): idx[t,j] == e}                 assignments
//   stats[c][e][1] += #{t: idx[t,0] == e}                      top-1
//   stats[c][e][2] += #{(t, j): idx[t,j] == e, pos[t,j] < 0}   dropped
//   stats[c][e][3] += sum fix(w[t,j]) over idx[t,j] == e       gate mass
//   stats[c][e][4] += sum_t fix(probs[t,e])                    prob mass
// over the tokens t of the images whose context is c, fix(x) = (int64)
// rint(x 2^32).  Every term is an integer, so the sums do not depend on the
// order the workgroups arrive in: the table is bitwise reproducible and equals
// the host restatement (stats.route_stats_reference) exactly.
//
// One workgroup owns up to 128 consecutive tokens of ONE image, hence of one
// context.  Prob mass: the chunk's [tokens, E] block of probs is contiguous;
// the first S = (256 / E) E threads walk it with stride S, so a thread reads
// consecutive floats with its neighbours and always meets the same expert
// (tid % E): the sum stays in one 64-bit register per thread.  Slots: one
// thread per assignment adds into the expert's LDS counters.  The per-thread
// prob sums join them through LDS, and the workgroup leaves with at most 5 E
// 64-bit integer atomic adds to the table (zero sums are not added, so an
// out-of-range context or expert writes nothing).
#include "moe_common.h"
#include "prof.h"

namespace moe {

constexpr int kStatsChunk = 128;   // tokens per workgroup
constexpr int kStatsFields = 5;

__device__ __forceinline__ long long stats_fix(float x) {
  return __double2ll_rn((double)x * 4294967296.0);
}

__global__ __launch_bounds__(256) void route_stats_kernel(
    const int32_t* __restrict__ topk_idx, const float* __restrict__ topk_w, const int32_t* __restrict__ pos,
    const float* __restrict__ probs, const int32_t* __restrict__ ctx_img, int n_ctx, int tokens_per_image,
    int chunks_per_image, int E, int k, unsigned long long* __restrict__ stats) {
  __shared__ unsigned long long s_mass[64][2];  // gate, prob
  __shared__ int s_cnt[64][3];                  // assignments, top-1, dropped
  const int tid = threadIdx.x;
  const int img = blockIdx.x / chunks_per_image;
  const int chunk = blockIdx.x - img * chunks_per_image;
  const int c = ctx_img != nullptr ? ctx_img[img] : 0;
  if (c < 0 || c >= n_ctx) return;  // workgroup-uniform: before any barrier
  const int tok0 = chunk * kStatsChunk;
  const int ntok = min(kStatsChunk, tokens_per_image - tok0);
  const size_t t0 = (size_t)img * tokens_per_image + tok0;

  if (tid < E) {
    s_mass[tid][0] = 0ull;
    s_mass[tid][1] = 0ull;
    s_cnt[tid][0] = 0;
    s_cnt[tid][1] = 0;
    s_cnt[tid][2] = 0;
  }
  __syncthreads();

  // prob mass: thread tid < S meets expert tid % E at every step of stride S
  const int S = (256 / E) * E;
  long long pm = 0;
  if (tid < S) {
    const float* p = probs + t0 * E;
    const int n = ntok * E;
    for (int i = tid; i < n; i += S) pm += stats_fix(p[i]);
  }

  // the k slots: one thread per assignment
  const int na = ntok * k;
  for (int a = tid; a < na; a += 256) {
    const size_t ga = t0 * k + a;
    const int e = topk_idx[ga];
    if (e < 0 || e >= E) continue;
    atomicAdd(&s_cnt[e][0], 1);
    if (a % k == 0) atomicAdd(&s_cnt[e][1], 1);
    if (pos != nullptr && pos[ga] < 0) atomicAdd(&s_cnt[e][2], 1);
    atomicAdd(&s_mass[e][0], (unsigned long long)stats_fix(topk_w[ga]));
  }
  if (tid < S && pm != 0) atomicAdd(&s_mass[tid % E][1], (unsigned long long)pm);
  __syncthreads();

  for (int i = tid; i < E * kStatsFields; i += 256) {
    const int e = i / kStatsFields, f = i - e * kStatsFields;
    const unsigned long long v = f < 3 ? (unsigned long long)s_cnt[e][f] : s_mass[e][f - 3];
    if (v != 0ull) atomicAdd(stats + ((size_t)c * E + e) * kStatsFields + f, v);
  }
}

}  // namespace moe

using namespace moe;

extern "C" int moe_route_stats(const int32_t* topk_idx, const float* topk_w, const int32_t* pos, const float* probs,
                               const int32_t* ctx_img, int n_ctx, int tokens_per_image, int T, int E, int k,
                               long long* stats, hipStream_t stream) {
  if (E < 1 || E > 64 || k < 1 || k > 8 || k > E) return fail("route_stats: need 1<=E<=64, 1<=k<=min(8,E)");
  if (n_ctx < 1) return fail("route_stats: n_ctx must be >= 1");
  if (ctx_img == nullptr && n_ctx != 1) return fail("route_stats: ctx_img is NULL, so n_ctx must be 1");
  if (T < 0 || tokens_per_image < 1 || T % tokens_per_image != 0)
    return fail("route_stats: T must be a non-negative multiple of tokens_per_image >= 1");
  if (T == 0) return 0;
  if (topk_idx == nullptr || topk_w == nullptr || probs == nullptr || stats == nullptr)
    return fail("route_stats: NULL pointer");
  const int chunks = (tokens_per_image + kStatsChunk - 1) / kStatsChunk;
  const long long grid = (long long)(T / tokens_per_image) * chunks;
  if (grid > 0x7fffffffLL) return fail("route_stats: too many workgroups");
  // bytes: idx + w (+ pos) per assignment and probs per (token, expert) read; the table's adds
  ProfScope prof(stream, PROF_ROUTE_STATS,
                 (double)T * (k * (pos != nullptr ? 12.0 : 8.0) + 4.0 * E) + 8.0 * n_ctx * E * kStatsFields);
  MOE_LAUNCH(prof, route_stats_kernel, dim3((unsigned)grid), dim3(256), 0, stream, topk_idx, topk_w, pos, probs,
             ctx_img, n_ctx, tokens_per_image, chunks, E, k, reinterpret_cast<unsigned long long*>(stats));
  return check_launch("moe_route_stats");
}
