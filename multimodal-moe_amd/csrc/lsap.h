// The rectangular assignment solver shared by the set criterion's matcher
// (matcher.hip) and the tracking evaluator (moteval.hip): scipy 1.15's
// linear_sum_assignment (Crouse's shortest augmenting path, the form it runs on
// the transposed [n, Q] problem) restated step for step so that the matching --
// ties included -- is the one scipy returns: the same double arithmetic in the
// same order, the same "remaining" column list with swap removal, and the same
// tie rule for the next column (the lowest reduced cost; among equal ones the
// LAST unassigned in list order, else the first).  One 64-lane workgroup per
// problem: the wave parallelises the column scan of every Dijkstra step and the
// dual updates; bookkeeping is done by lane 0.
//
// lsap_solve(cost_qm, n, Q, M, out, status, smem): cost_qm(q, m) for Q queries
// and the first n of M targets, n <= Q and n <= M; out[m] = the query of target
// m, -1 for m >= n.  smem: M * 8 + 2 * Q * 8 + 3 * Q * 4 + M * 4 + M + Q bytes,
// 8-byte aligned.  Consecutive solves of one workgroup reuse smem and the static
// shared scalars below: put a __syncthreads() between them.
//
// lsap_solve<true> is the same solver inside a wider workgroup (the tracker's,
// up to 256 threads): threads 0..63 are the solver, threads 64 and up do no work
// and take the same barriers.  Every branch that lies between two barriers is
// then decided by a block-uniform value: the arguments n, Q, M; the loop counters
// cur and nrem; and s_sink and s_minval, read from LDS after the barrier that
// follows lane 0's write and before the barrier that precedes its next write
// (s_minval is L, which only the solver's wave holds in a register).  With
// kWide == false nothing changes: the code is the one-wave form.
#pragma once

#include "moe_common.h"

namespace moe {

__device__ __forceinline__ double wave_min_d(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmin(x, __shfl_xor(x, o, 64));
  return x;
}
__device__ __forceinline__ int wave_max_i(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o, 64));
  return x;
}
__device__ __forceinline__ int wave_min_i(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64));
  return x;
}

// cost(q, m) of one problem: an explicit [Q][M] matrix
struct MatrixCost {
  const float* C;
  int M;
  __device__ __forceinline__ float operator()(int q, int m) const { return C[(size_t)q * M + m]; }
};

template <bool kWide = false, class CostFn>
__device__ void lsap_solve(const CostFn& cost_qm, int n, int Q, int M, int32_t* __restrict__ out,
                           int32_t* __restrict__ status, char* smem) {
  double* u = reinterpret_cast<double*>(smem);  // [M]
  double* v = u + M;                            // [Q]
  double* spc = v + Q;                          // [Q] shortest path costs
  int* path = reinterpret_cast<int*>(spc + Q);  // [Q]
  int* row4col = path + Q;                      // [Q]
  int* remaining = row4col + Q;                 // [Q]
  int* col4row = remaining + Q;                 // [M]
  uint8_t* SR = reinterpret_cast<uint8_t*>(col4row + M);  // [M]
  uint8_t* SC = SR + M;                                   // [Q]
  __shared__ int s_i, s_sink, s_index;
  __shared__ double s_minval;

  // an idle thread of the wide form: a lane past every bound, so every "lane, lane + 64, ..." loop below is empty
  // for it and it is never lane 0
  const int lane = (!kWide || threadIdx.x < 64) ? (int)threadIdx.x : 0x40000000;
  for (int m = lane; m < M; m += 64) out[m] = -1;
  if (n <= 0) return;
  if (n > Q || n > M) {
    if (lane == 0) atomicExch(status, 1);
    return;
  }
  // scipy transposes when rows > cols: rows = targets, cols = queries (Q > n);
  // a square problem (n == Q) keeps rows = queries, cols = targets
  const bool tr = Q > n;
  const int nr = n, nc = tr ? Q : n;
  for (int m = lane; m < nr; m += 64) {
    u[m] = 0.0;
    col4row[m] = -1;
  }
  for (int j = lane; j < nc; j += 64) {
    v[j] = 0.0;
    row4col[j] = -1;
    path[j] = -1;
  }
  __syncthreads();

  for (int cur = 0; cur < nr; ++cur) {
    for (int it = lane; it < nc; it += 64) {
      remaining[it] = nc - it - 1;
      spc[it] = INFINITY;
      SC[it] = 0;
    }
    for (int m = lane; m < nr; m += 64) SR[m] = 0;
    if (lane == 0) {
      s_i = cur;
      s_sink = -1;
      s_minval = 0.0;
    }
    int nrem = nc;
    __syncthreads();
    while (true) {
      const int i = s_i;
      const double minval = s_minval;
      if (lane == 0) SR[i] = 1;
      const double ui = u[i];
      // relax every remaining column, then the lowest reduced cost with scipy's tie rule
      double lo = INFINITY;
      for (int it = lane; it < nrem; it += 64) {
        const int j = remaining[it];
        const double r = minval + (double)(tr ? cost_qm(j, i) : cost_qm(i, j)) - ui - v[j];
        if (r < spc[j]) {
          path[j] = i;
          spc[j] = r;
        }
        lo = fmin(lo, spc[j]);
      }
      const double L = wave_min_d(lo);
      int last_un = -1, first_eq = 0x7fffffff;
      for (int it = lane; it < nrem; it += 64) {
        const int j = remaining[it];
        if (spc[j] == L) {
          first_eq = min(first_eq, it);
          if (row4col[j] == -1) last_un = max(last_un, it);
        }
      }
      last_un = wave_max_i(last_un);
      first_eq = wave_min_i(first_eq);
      __syncthreads();  // every lane has read remaining / spc before lane 0 edits them
      if (lane == 0) {
        const int index = last_un >= 0 ? last_un : first_eq;
        const int j = remaining[index];
        s_minval = L;
        if (L == INFINITY) {
          // no remaining column is reachable at a finite cost: infeasible, as scipy
          // decides BEFORE it looks at the column (its path entry was never written)
        } else if (row4col[j] == -1) s_sink = j;
        else s_i = row4col[j];
        SC[j] = 1;
        remaining[index] = remaining[nrem - 1];
        s_index = index;
      }
      --nrem;
      __syncthreads();
      // wide: lane 0 stored L in s_minval before the barrier above and writes it next after the next one
      const double Lb = kWide ? s_minval : L;
      if (s_sink != -1 || Lb == INFINITY || nrem == 0) break;  // nrem == 0 only if infeasible
    }
    const double minval = s_minval;
    if (s_sink == -1) {  // infeasible (non-finite costs)
      if (lane == 0) atomicExch(status, 2);
      return;
    }
    // dual updates (u of the visited rows other than cur use spc before any v change)
    for (int m = lane; m < nr; m += 64)
      if (SR[m] && m != cur) u[m] += minval - spc[col4row[m]];
    if (lane == 0) u[cur] += minval;
    for (int j = lane; j < nc; j += 64)
      if (SC[j]) v[j] -= minval - spc[j];
    __syncthreads();
    if (lane == 0) {  // augment along the path back to cur (at most cur + 1 hops)
      int j = s_sink;
      for (int hop = 0; hop <= cur; ++hop) {
        const int i = path[j];
        row4col[j] = i;
        const int t = col4row[i];
        col4row[i] = j;
        j = t;
        if (i == cur) break;
      }
    }
    __syncthreads();
  }
  for (int r = lane; r < nr; r += 64) {
    if (tr) out[r] = col4row[r];  // row = target
    else out[col4row[r]] = r;     // row = query
  }
}

}  // namespace moe
