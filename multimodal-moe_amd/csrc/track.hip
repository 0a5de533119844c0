// The tracker of engine.track on the GPU (track.py: track_reference, which
// engine.predict(track=...) runs on the host with MOE_PREDICT_TRACK=0): links
// a sequence's detections from frame to frame by greedy IoU association in two
// score bands (BYTE), with a fixed-gain filter on each track's box.
//
// One workgroup per state slot (a sequence), one thread per track slot (T
// rounded up to whole waves).  The workgroup reads frame_slot[] front to back
// and handles its own frames in frame order; the sequence's tracks are read
// from HBM into LDS before its first frame and written back once after its
// last.  A slot without frames touches nothing.  The frames of a slot outside
// [0, S) get empty outputs from workgroup f % S.  Per frame:
//   1. The rows go into LDS (box, score, label, and rstate: kRowOut / kRowLow /
//      kRowHigh, later the slot that took the row); every live track predicts:
//      box = box + vel and, with a frame_shift table (rtdetr_track_update_shift:
//      camera-motion compensation), box = (box + vel) + the frame's shift.
//   2. Association, stage 1 (live tracks x high rows, match_iou), then stage 2
//      (tracks still unmatched with age 0 and hits >= min_hits x low rows,
//      second_iou).  Every track scans the stage's free rows (an LDS broadcast
//      read per row) and keeps its best admissible one as a 64-bit key: iou
//      bits << 32 | ~row << 16 | ~slot.  Each round takes the workgroup-wide
//      maximum key (wave shuffles, then one LDS word per wave, double buffered:
//      one barrier a round) -- the admissible pair with the largest iou, the
//      lower row, then the lower slot -- and only the tracks whose best row was
//      just taken scan again.  A round matches one pair, so at most min(T, K)
//      rounds; the iou of a pair never changes within a frame, so a rescan
//      reproduces the bits.  The division runs only where inter != 0.
//   3. Update / age / free, each thread its own track.
//   4. Births: the free slots are ranked (ballots + per-wave counts) into a
//      list; the unmatched high rows with score >= new_thr are ranked in row
//      order the same way and the j-th takes the j-th free slot, id next_id +
//      j; the rest are counted in dropped.
//   5. Report: every row's id and filtered box, -1 and zeros elsewhere; count.
//
// Decisions and boxes are track_reference's bit for bit: fp32, each operation
// rounded on its own, no FMA contraction (pragma below), one correctly rounded
// division.
//
// rtdetr_track_sweep (tune.py) runs G configurations of the same rule in one launch: workgroup (s, g) of a (S, G)
// grid is the workgroup above under the g-th row of two device tables, on the same read-only inputs, with state
// [G][S] and, in place of step 5, the compact report: the j-th reported row in row order at position j of out_id
// [G][F][T], out_boxes [G][F][T][4] and out_row [G][F][T] (a slot is taken by one row a frame, so count <= T),
// ranked by trk_block_rank as the births are; -1 / zeros / -1 past count.
//
// LDS (dynamic, every offset a multiple of 16): rows 28 K bytes, tracks 52 T
// bytes, the free list 4 T, 192 bytes of keys and counters: 41.2 KiB at the
// limits K = 1024, T = 256.
//
// rtdetr_track_update_assoc / rtdetr_track_sweep_assoc (TrackArgs.assoc) are trk_run<.., kAssoc = true>: a second
// pair of kernels, so that the three entries above keep the code they had (kAssoc = false compiles none of what
// follows).  With assoc != 0 (block-uniform: a launch's argument, or the configuration's table entry) step 2 of a
// stage is track.py's step 4 "lsap" instead of the greedy rounds:
//   a. every eligible track scans the stage's rows as the greedy scan does, notes whether it has an admissible row
//      and marks those rows in an LDS flag array (plain stores of 1; several tracks may mark one row);
//   b. the tracks with a row and the marked rows are compacted into two ascending index lists (trk_block_rank);
//   c. lsap_solve<true> (lsap.h: threads 0..63 solve, the other waves take the same barriers) on the pruned problem,
//      the larger side as the queries (equal: the tracks), cost -(iou if admissible else 0) computed by TrkCost from
//      the boxes in LDS through the two lists -- the predicted boxes are stored to tbox before the stage for this;
//   d. a returned pair that is admissible sets rstate[row] and the track's matched row.
// Its LDS is TrkLds plus TrkAssocLds: the lists 4 T + 4 K, the flags 4 K, the matched rows 4 T, the solver's out 4 M
// and scratch 12 M + 29 Q + M bytes at Q = max(T, K), M = min(T, K): 85.4 KiB at the limits, raised past the 64 KiB
// default with allow_dyn_lds.
#include "moe_common.h"
#include "lsap.h"
#include "prof.h"

#pragma clang fp contract(off)

namespace moe {

constexpr int kTrkMaxK = 1024, kTrkMaxT = 256, kTrkMaxF = 1024, kTrkMaxS = 1024, kTrkMaxWaves = 4;
constexpr int kTrkHitsCap = 1 << 30;
constexpr int kTrkMaxG = 1024, kTrkSweepF = 7, kTrkSweepI = 3;  // rtdetr_track_sweep: configurations, table widths
constexpr int kRowOut = -3, kRowLow = -2, kRowHigh = -1;  // rstate: not taking part / free low / free high; >= 0: its slot

__host__ __device__ constexpr size_t trk_up16(size_t n) { return (n + 15) & ~(size_t)15; }

struct TrkLds {
  size_t rbox, rscore, rlabel, rstate, tbox, tvel, tscore, tmeta, freelist, wkey, wcnt, ctl, total;
  __host__ __device__ TrkLds(int K, int T) {
    rbox = 0;                                           // float4 [K]
    rscore = rbox + (size_t)K * 16;                     // float [K]
    rlabel = rscore + trk_up16((size_t)K * 4);          // int32 [K]
    rstate = rlabel + trk_up16((size_t)K * 4);          // int32 [K]
    tbox = rstate + trk_up16((size_t)K * 4);            // float4 [T]
    tvel = tbox + (size_t)T * 16;                       // float4 [T]
    tscore = tvel + (size_t)T * 16;                     // float [T]
    tmeta = tscore + trk_up16((size_t)T * 4);           // int4 [T]: label, id, age, hits
    freelist = tmeta + (size_t)T * 16;                  // int32 [T]
    wkey = freelist + trk_up16((size_t)T * 4);          // uint64 [2][kTrkMaxWaves]
    wcnt = wkey + 2 * kTrkMaxWaves * 8;                 // int32 [kTrkMaxWaves]
    ctl = wcnt + trk_up16(kTrkMaxWaves * 4);            // int32 [4]: next_id, dropped, reported
    total = ctl + 16;
  }
};

// what kAssoc adds after TrkLds's bytes
constexpr size_t kTrkStaticLds = 32;  // lsap_solve's shared scalars
struct TrkAssocLds {
  size_t slist, rlist, aflag, smatch, aout, solver, total;
  __host__ __device__ TrkAssocLds(int K, int T) {
    const size_t Q = K > T ? K : T, M = K > T ? T : K;
    slist = TrkLds(K, T).total;                          // int32 [T]: the tracks with an admissible row, ascending
    rlist = slist + trk_up16((size_t)T * 4);             // int32 [K]: the rows with an admissible track, ascending
    aflag = rlist + trk_up16((size_t)K * 4);             // int32 [K]: row d is marked
    smatch = aflag + trk_up16((size_t)K * 4);            // int32 [T]: the row the solve gave track t, -1
    aout = smatch + trk_up16((size_t)T * 4);             // int32 [M]: lsap_solve's out
    solver = aout + trk_up16(M * 4);                     // lsap_solve's scratch
    total = solver + trk_up16(M * 8 + 2 * Q * 8 + 3 * Q * 4 + M * 4 + M + Q);
  }
};

struct TrkParams {
  float track_high, track_low, new_thr, match_iou, second_iou, alpha, beta;
  int max_age, min_hits, class_agnostic;
};

__device__ __forceinline__ float trk_area(float4 b) { return fmaxf(b.z - b.x, 0.f) * fmaxf(b.w - b.y, 0.f); }

__device__ __forceinline__ float trk_iou(float4 t, float ta, float4 d) {
  const float iw = fmaxf(fminf(t.z, d.z) - fmaxf(t.x, d.x), 0.f);
  const float ih = fmaxf(fminf(t.w, d.w) - fmaxf(t.y, d.y), 0.f);
  const float inter = iw * ih;
  if (inter == 0.f) return 0.f;  // 0 / den and the den <= 0 case alike
  const float den = (ta + trk_area(d)) - inter;
  return den > 0.f ? __fdiv_rn(inter, den) : 0.f;
}

// the admissibility of (track, row) under the stage's threshold, and the pair's iou: the one statement of it for the
// lsap stage's scan, its cost and its matches, so that the three agree to the bit
__device__ __forceinline__ bool trk_adm(float4 t, float ta, int tlabel, float4 d, int dlabel, float thr,
                                        int agnostic, float* iou) {
  *iou = 0.f;
  if (!agnostic && dlabel != tlabel) return false;
  *iou = trk_iou(t, ta, d);
  return *iou > thr;  // false for NaN
}

// lsap_solve's cost of (query, target) through the two index lists: -(iou if admissible else 0)
struct TrkCost {
  const float4* tbox;
  const int4* tmeta;
  const float4* rbox;
  const int32_t* rlabel;
  const int32_t* slist;
  const int32_t* rlist;
  float thr;
  int agnostic;
  bool sq;  // the tracks are the queries
  __device__ __forceinline__ float operator()(int q, int m) const {
    const int t = slist[sq ? q : m], d = rlist[sq ? m : q];
    const float4 tb = tbox[t];
    float iou;
    const bool adm = trk_adm(tb, trk_area(tb), tmeta[t].x, rbox[d], rlabel[d], thr, agnostic, &iou);
    return -(adm ? iou : 0.f);
  }
};

__device__ __forceinline__ unsigned long long trk_wave_max(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t hi = (uint32_t)__shfl_xor((int)(v >> 32), off, 64);
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

// the rank of this thread among the workgroup's threads with ``flag``, in thread order, and their number.
// Two barriers; wcnt is free again on return.
__device__ __forceinline__ int trk_block_rank(bool flag, int32_t* wcnt, int lane, int wave, int nwaves, int* total) {
  const unsigned long long bal = __ballot(flag);
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  if (lane == 0) wcnt[wave] = __popcll(bal);
  __syncthreads();
  int base = 0, sum = 0;
  for (int w = 0; w < nwaves; ++w) {
    const int c = wcnt[w];
    if (w < wave) base += c;
    sum += c;
  }
  __syncthreads();
  *total = sum;
  return base + __popcll(bal & below);
}

// The frames of state slot ``s`` for one configuration ``p``: the whole rule, shared by track_update_kernel and
// track_sweep_kernel.  gbox / gscore / gmeta / gseq are the state slot's own buffers; out_id, out_boxes, out_row and
// count are the launch's (the configuration's, in a sweep).  kCompact chooses the form of step 5: false, out_id [F][K]
// and out_boxes [F][K][4] per row (out_row unused); true, the reported rows alone, in row order, in out_id [F][T],
// out_boxes [F][T][4] and out_row [F][T], padded with -1 / zeros / -1.  kAssoc: the kernels that take ``assoc`` (0
// greedy, else lsap; block-uniform); with kAssoc false ``assoc`` is not read and none of the lsap stage is compiled.
template <bool kCompact, bool kAssoc>
__device__ __forceinline__ void trk_run(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ n_valid, const int32_t* __restrict__ frame_slot,
    const int32_t* __restrict__ frame_reset, const float* __restrict__ frame_shift, int F, int K, int S, int T,
    const int s, const TrkParams& p, const int assoc, float4* __restrict__ gbox, float* __restrict__ gscore,
    int4* __restrict__ gmeta, int32_t* __restrict__ gseq, int32_t* __restrict__ out_id,
    float* __restrict__ out_boxes, int32_t* __restrict__ out_row, int32_t* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const TrkLds o(K, T);
  float4* rbox = reinterpret_cast<float4*>(smem + o.rbox);
  float* rscore = reinterpret_cast<float*>(smem + o.rscore);
  int32_t* rlabel = reinterpret_cast<int32_t*>(smem + o.rlabel);
  int32_t* rstate = reinterpret_cast<int32_t*>(smem + o.rstate);
  float4* tbox = reinterpret_cast<float4*>(smem + o.tbox);
  float4* tvel = reinterpret_cast<float4*>(smem + o.tvel);
  float* tscore = reinterpret_cast<float*>(smem + o.tscore);
  int4* tmeta = reinterpret_cast<int4*>(smem + o.tmeta);
  int32_t* freelist = reinterpret_cast<int32_t*>(smem + o.freelist);
  unsigned long long* wkey = reinterpret_cast<unsigned long long*>(smem + o.wkey);
  int32_t* wcnt = reinterpret_cast<int32_t*>(smem + o.wcnt);
  int32_t* ctl = reinterpret_cast<int32_t*>(smem + o.ctl);
  const TrkAssocLds oa(K, T);  // used with kAssoc only
  int32_t* slist = reinterpret_cast<int32_t*>(smem + oa.slist);
  int32_t* rlist = reinterpret_cast<int32_t*>(smem + oa.rlist);
  int32_t* aflag = reinterpret_cast<int32_t*>(smem + oa.aflag);
  int32_t* smatch = reinterpret_cast<int32_t*>(smem + oa.smatch);
  int32_t* aout = reinterpret_cast<int32_t*>(smem + oa.aout);

  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nwaves = nthr >> 6;
  const bool mine = tid < T;  // this thread owns track slot tid
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int W = kCompact ? T : K;  // the outputs' row length
  bool loaded = false;  // block-uniform: the sequence's tracks stand in LDS
  int parity = 0;       // which half of wkey the next round writes

  for (int f = 0; f < F; ++f) {
    const int fs = frame_slot[f];  // block-uniform
    float4* ob = reinterpret_cast<float4*>(out_boxes) + (size_t)f * W;
    int32_t* oi = out_id + (size_t)f * W;
    int32_t* orow = kCompact ? out_row + (size_t)f * W : nullptr;
    if (fs != s) {
      if ((fs < 0 || fs >= S) && f % S == s) {  // nobody's frame: the empty outputs
        for (int d = tid; d < W; d += nthr) {
          oi[d] = -1;
          ob[d] = zero4;
          if (kCompact) orow[d] = -1;
        }
        if (tid == 0) count[f] = 0;
      }
      continue;
    }
    const bool reset = frame_reset[f] != 0;
    if (reset || !loaded) {
      if (reset) {
        if (mine) {
          tbox[tid] = zero4;
          tvel[tid] = zero4;
          tscore[tid] = 0.f;
          tmeta[tid] = make_int4(0, 0, 0, 0);
        }
        if (tid == 0) {
          ctl[0] = 1;
          ctl[1] = 0;
        }
      } else {
        if (mine) {
          tbox[tid] = gbox[2 * tid];
          tvel[tid] = gbox[2 * tid + 1];
          tscore[tid] = gscore[tid];
          tmeta[tid] = gmeta[tid];
        }
        if (tid == 0) {
          ctl[0] = gseq[0];
          ctl[1] = gseq[1];
        }
      }
      loaded = true;
    }
    // 1. the rows, and the prediction
    const int n = n_valid != nullptr ? min(max(n_valid[f], 0), K) : K;
    const float4* bx = reinterpret_cast<const float4*>(boxes) + (size_t)f * K;
    for (int d = tid; d < K; d += nthr) {
      const float sc = scores[(size_t)f * K + d];
      rbox[d] = bx[d];
      rscore[d] = sc;
      rlabel[d] = labels[(size_t)f * K + d];
      const bool part = d < n && sc >= p.track_low && fabsf(sc) < INFINITY;  // false for NaN
      rstate[d] = !part ? kRowOut : (sc >= p.track_high ? kRowHigh : kRowLow);
    }
    int4 m = make_int4(0, 0, 0, 0);  // label, id, age, hits
    float4 tb = zero4;
    if (mine) {
      m = tmeta[tid];
      tb = tbox[tid];
      if (m.w > 0) {
        const float4 v = tvel[tid];
        tb = make_float4(tb.x + v.x, tb.y + v.y, tb.z + v.z, tb.w + v.w);
        if (frame_shift != nullptr) {  // NULL adds nothing: -0.0 + 0.0 would be +0.0
          const float sx = frame_shift[2 * f], sy = frame_shift[2 * f + 1];
          tb = make_float4(tb.x + sx, tb.y + sy, tb.z + sx, tb.w + sy);
        }
        if (kAssoc) tbox[tid] = tb;  // TrkCost reads other tracks' predicted boxes; step 3 stores every live box again
      }
    }
    if (tid == 0) ctl[2] = 0;
    __syncthreads();

    // 2. association
    const float ta = trk_area(tb);
    int matched = -1;  // the row this track took
    for (int stage = 0; stage < 2; ++stage) {
      const int want = stage == 0 ? kRowHigh : kRowLow;
      const float thr = stage == 0 ? p.match_iou : p.second_iou;
      const bool eligible = mine && m.w > 0 && matched < 0 && (stage == 0 || (m.z == 0 && m.w >= p.min_hits));
      if (kAssoc && assoc != 0) {  // block-uniform: the lsap stage (the file's head, a-d)
        for (int d = tid; d < K; d += nthr) aflag[d] = 0;
        if (mine) smatch[tid] = -1;
        __syncthreads();
        bool has = false;  // a. this track has an admissible row
        if (eligible) {
          for (int d = 0; d < K; ++d) {
            if (rstate[d] != want) continue;  // wave-uniform
            float iou;
            if (!trk_adm(tb, ta, m.x, rbox[d], rlabel[d], thr, p.class_agnostic, &iou)) continue;
            has = true;
            aflag[d] = 1;
          }
        }
        __syncthreads();
        int ns = 0, nr = 0;  // b. block-uniform: the tracks and the rows that are kept
        const int srank = trk_block_rank(has, wcnt, lane, wave, nwaves, &ns);
        if (has) slist[srank] = tid;
        for (int base = 0; base < K; base += nthr) {
          const int d = base + tid;
          const bool marked = d < K && aflag[d] != 0;
          int nc = 0;
          const int j = nr + trk_block_rank(marked, wcnt, lane, wave, nwaves, &nc);
          if (marked) rlist[j] = d;
          nr += nc;
        }
        __syncthreads();
        if (ns > 0) {  // block-uniform; a kept track has a kept row, so nr > 0 too
          const bool sq = ns >= nr;
          const int n = sq ? nr : ns;
          lsap_solve<true>(TrkCost{tbox, tmeta, rbox, rlabel, slist, rlist, thr, p.class_agnostic, sq}, n,
                           sq ? ns : nr, n, aout, &ctl[3], smem + oa.solver);  // c.
          __syncthreads();
          for (int mm = tid; mm < n; mm += nthr) {  // d.
            const int q = aout[mm];
            if (q < 0) continue;
            const int t = slist[sq ? q : mm], d = rlist[sq ? mm : q];
            const float4 b = tbox[t];
            float iou;
            if (!trk_adm(b, trk_area(b), tmeta[t].x, rbox[d], rlabel[d], thr, p.class_agnostic, &iou)) continue;
            rstate[d] = t;
            smatch[t] = d;
          }
          __syncthreads();  // rstate and smatch, before the next stage and the steps below read them
          if (has && smatch[tid] >= 0) matched = smatch[tid];
        }
        continue;
      }
      unsigned long long key = 0ull;
      bool scan = eligible;
      int taken = -1;  // the row the last round matched: taken, whether or not its rstate write has landed
      for (;;) {
        if (scan) {
          key = 0ull;
          for (int d = 0; d < K; ++d) {
            if (rstate[d] != want || d == taken) continue;  // wave-uniform
            if (!p.class_agnostic && rlabel[d] != m.x) continue;
            float iou = trk_iou(tb, ta, rbox[d]);
            if (!(iou > thr)) continue;
            if (iou == 0.f) iou = 0.f;  // -0.0 as +0.0
            const unsigned long long k = ((unsigned long long)__float_as_uint(iou) << 32) |
                                         ((uint32_t)(~d & 0xFFFF) << 16) | (uint32_t)(~tid & 0xFFFF);
            key = k > key ? k : key;  // equal iou: the lower row has the larger key
          }
        }
        const unsigned long long wmax = trk_wave_max(key);
        unsigned long long* wk = wkey + parity * kTrkMaxWaves;
        parity ^= 1;
        if (lane == 0) wk[wave] = wmax;
        __syncthreads();
        unsigned long long best = 0ull;
        for (int w = 0; w < nwaves; ++w) best = wk[w] > best ? wk[w] : best;
        if (best == 0ull) break;  // block-uniform
        const int bd = (int)(~(uint32_t)(best >> 16) & 0xFFFF), bt = (int)(~(uint32_t)best & 0xFFFF);
        taken = bd;
        scan = false;
        if (tid == bt) {
          matched = bd;
          rstate[bd] = bt;
          key = 0ull;
        } else if (key != 0ull && (int)(~(uint32_t)(key >> 16) & 0xFFFF) == bd) {
          scan = true;  // lost its best row
        }
      }
      __syncthreads();  // the last round's rstate write, before the next stage reads
    }

    // 3. update, age, free
    if (mine && m.w > 0) {
      if (matched >= 0) {
        const float4 d = rbox[matched];
        const float4 r = make_float4(d.x - tb.x, d.y - tb.y, d.z - tb.z, d.w - tb.w);
        const float4 v = tvel[tid];
        tb = make_float4(tb.x + p.alpha * r.x, tb.y + p.alpha * r.y, tb.z + p.alpha * r.z, tb.w + p.alpha * r.w);
        tvel[tid] = make_float4(v.x + p.beta * r.x, v.y + p.beta * r.y, v.z + p.beta * r.z, v.w + p.beta * r.w);
        tbox[tid] = tb;
        tscore[tid] = rscore[matched];
        m.z = 0;
        m.w = min(m.w + 1, kTrkHitsCap);
      } else {
        bool drop = m.w < p.min_hits;
        if (!drop) {
          m.z += 1;
          drop = m.z > p.max_age;
        }
        if (drop) {
          m = make_int4(0, 0, 0, 0);
          tb = zero4;
          tvel[tid] = zero4;
          tscore[tid] = 0.f;
        }
        tbox[tid] = tb;  // the predicted box of a coasting track
      }
      tmeta[tid] = m;
    }

    // 4. births
    int nfree = 0;
    const bool isfree = mine && m.w == 0;
    const int frank = trk_block_rank(isfree, wcnt, lane, wave, nwaves, &nfree);
    if (isfree) freelist[frank] = tid;
    __syncthreads();
    const int next_id = ctl[0];
    int births = 0;  // block-uniform: the candidates so far
    for (int base = 0; base < K; base += nthr) {
      const int d = base + tid;
      const bool cand = d < K && rstate[d] == kRowHigh && rscore[d] >= p.new_thr;
      int nc = 0;
      const int j = births + trk_block_rank(cand, wcnt, lane, wave, nwaves, &nc);
      if (cand && j < nfree) {
        const int t = freelist[j];
        tbox[t] = rbox[d];
        tvel[t] = zero4;
        tscore[t] = rscore[d];
        tmeta[t] = make_int4(rlabel[d], next_id + j, 0, 1);
        rstate[d] = t;
      }
      births += nc;
    }
    __syncthreads();
    if (tid == 0) {
      ctl[0] = next_id + min(births, nfree);
      ctl[1] += max(births - nfree, 0);
    }

    // 5. report
    if (kCompact) {
      // the j-th reported row, in row order, goes to position j; a slot is taken by one row, so at most T of them
      int reported = 0;  // block-uniform: the reported rows so far
      for (int base = 0; base < K; base += nthr) {
        const int d = base + tid;
        bool rep = false;
        int rid = -1;
        float4 rb = zero4;
        if (d < K) {
          const int t = rstate[d];
          if (t >= 0) {
            const int4 tm = tmeta[t];
            rep = tm.w >= p.min_hits;
            rid = tm.y;
            rb = tbox[t];
          }
        }
        int nr = 0;
        const int j = reported + trk_block_rank(rep, wcnt, lane, wave, nwaves, &nr);
        if (rep && j < T) {
          oi[j] = rid;
          ob[j] = rb;
          orow[j] = d;
        }
        reported += nr;
      }
      reported = min(reported, T);
      for (int j = reported + tid; j < T; j += nthr) {
        oi[j] = -1;
        ob[j] = zero4;
        orow[j] = -1;
      }
      if (tid == 0) count[f] = reported;
    } else {
      for (int base = 0; base < K; base += nthr) {
        const int d = base + tid;
        bool rep = false;
        if (d < K) {
          const int t = rstate[d];
          int4 tm = make_int4(0, 0, 0, 0);
          if (t >= 0) tm = tmeta[t];
          rep = t >= 0 && tm.w >= p.min_hits;
          oi[d] = rep ? tm.y : -1;
          ob[d] = rep ? tbox[t] : zero4;
        }
        const unsigned long long bal = __ballot(rep);
        if (lane == 0 && bal != 0ull) atomicAdd(&ctl[2], __popcll(bal));
      }
      __syncthreads();
      if (tid == 0) count[f] = ctl[2];
    }
    __syncthreads();  // before the next frame overwrites the rows and ctl[2]
  }

  if (loaded) {
    if (mine) {
      gbox[2 * tid] = tbox[tid];
      gbox[2 * tid + 1] = tvel[tid];
      gscore[tid] = tscore[tid];
      gmeta[tid] = tmeta[tid];
    }
    if (tid == 0) {
      gseq[0] = ctl[0];
      gseq[1] = ctl[1];
    }
  }
}

__global__ __launch_bounds__(256) void track_update_kernel(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ n_valid, const int32_t* __restrict__ frame_slot,
    const int32_t* __restrict__ frame_reset, const float* __restrict__ frame_shift, int F, int K, int S, int T,
    TrkParams p, float* __restrict__ trk_box,
    float* __restrict__ trk_score, int32_t* __restrict__ trk_meta, int32_t* __restrict__ seq_meta,
    int32_t* __restrict__ out_id, float* __restrict__ out_boxes, int32_t* __restrict__ count) {
  const int s = blockIdx.x;
  trk_run<false, false>(boxes, scores, labels, n_valid, frame_slot, frame_reset, frame_shift, F, K, S, T, s, p, 0,
                 reinterpret_cast<float4*>(trk_box) + (size_t)s * T * 2, trk_score + (size_t)s * T,
                 reinterpret_cast<int4*>(trk_meta) + (size_t)s * T, seq_meta + 2 * (size_t)s, out_id, out_boxes,
                 nullptr, count);
}

// track_update_kernel with the association chosen by ``assoc`` (rtdetr_track_update_assoc)
__global__ __launch_bounds__(256) void track_update_assoc_kernel(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ n_valid, const int32_t* __restrict__ frame_slot,
    const int32_t* __restrict__ frame_reset, const float* __restrict__ frame_shift, int F, int K, int S, int T,
    TrkParams p, int assoc, float* __restrict__ trk_box,
    float* __restrict__ trk_score, int32_t* __restrict__ trk_meta, int32_t* __restrict__ seq_meta,
    int32_t* __restrict__ out_id, float* __restrict__ out_boxes, int32_t* __restrict__ count) {
  const int s = blockIdx.x;
  trk_run<false, true>(boxes, scores, labels, n_valid, frame_slot, frame_reset, frame_shift, F, K, S, T, s, p, assoc,
                       reinterpret_cast<float4*>(trk_box) + (size_t)s * T * 2, trk_score + (size_t)s * T,
                       reinterpret_cast<int4*>(trk_meta) + (size_t)s * T, seq_meta + 2 * (size_t)s, out_id, out_boxes,
                       nullptr, count);
}

__device__ __forceinline__ TrkParams trk_table_params(const float* __restrict__ params_f,
                                                      const int32_t* __restrict__ params_i, int g) {
  const float* pf = params_f + (size_t)g * kTrkSweepF;
  const int32_t* pi = params_i + (size_t)g * kTrkSweepI;
  TrkParams p;
  p.track_high = pf[0];
  p.track_low = pf[1];
  p.new_thr = pf[2];
  p.match_iou = pf[3];
  p.second_iou = pf[4];
  p.alpha = pf[5];
  p.beta = pf[6];
  p.max_age = pi[0];
  p.min_hits = pi[1];
  p.class_agnostic = pi[2] != 0 ? 1 : 0;
  return p;
}

// track_sweep_kernel with configuration g's association in params_assoc[g] (rtdetr_track_sweep_assoc)
__global__ __launch_bounds__(256) void track_sweep_assoc_kernel(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ n_valid, const int32_t* __restrict__ frame_slot,
    const int32_t* __restrict__ frame_reset, const float* __restrict__ frame_shift, int F, int K, int S, int T,
    const float* __restrict__ params_f, const int32_t* __restrict__ params_i,
    const int32_t* __restrict__ params_assoc, float* __restrict__ trk_box,
    float* __restrict__ trk_score, int32_t* __restrict__ trk_meta, int32_t* __restrict__ seq_meta,
    int32_t* __restrict__ out_id, float* __restrict__ out_boxes, int32_t* __restrict__ out_row,
    int32_t* __restrict__ count) {
  const int s = blockIdx.x, g = blockIdx.y;
  const TrkParams p = trk_table_params(params_f, params_i, g);
  const size_t gs = (size_t)g * S + s, gf = (size_t)g * F;
  trk_run<true, true>(boxes, scores, labels, n_valid, frame_slot, frame_reset, frame_shift, F, K, S, T, s, p,
                      params_assoc[g], reinterpret_cast<float4*>(trk_box) + gs * T * 2, trk_score + gs * T,
                      reinterpret_cast<int4*>(trk_meta) + gs * T, seq_meta + 2 * gs, out_id + gf * T,
                      out_boxes + gf * T * 4, out_row + gf * T, count + gf);
}

// The parameter sweep (tune.py): workgroup (s, g) runs state slot s under configuration g of the two tables, on the
// same read-only inputs; the state is [G][S] slots, the outputs [G][F] frames in the compact form.
__global__ __launch_bounds__(256) void track_sweep_kernel(
    const float* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ n_valid, const int32_t* __restrict__ frame_slot,
    const int32_t* __restrict__ frame_reset, const float* __restrict__ frame_shift, int F, int K, int S, int T,
    const float* __restrict__ params_f, const int32_t* __restrict__ params_i, float* __restrict__ trk_box,
    float* __restrict__ trk_score, int32_t* __restrict__ trk_meta, int32_t* __restrict__ seq_meta,
    int32_t* __restrict__ out_id, float* __restrict__ out_boxes, int32_t* __restrict__ out_row,
    int32_t* __restrict__ count) {
  const int s = blockIdx.x, g = blockIdx.y;
  const float* pf = params_f + (size_t)g * kTrkSweepF;
  const int32_t* pi = params_i + (size_t)g * kTrkSweepI;
  TrkParams p;
  p.track_high = pf[0];
  p.track_low = pf[1];
  p.new_thr = pf[2];
  p.match_iou = pf[3];
  p.second_iou = pf[4];
  p.alpha = pf[5];
  p.beta = pf[6];
  p.max_age = pi[0];
  p.min_hits = pi[1];
  p.class_agnostic = pi[2] != 0 ? 1 : 0;
  const size_t gs = (size_t)g * S + s, gf = (size_t)g * F;
  trk_run<true, false>(boxes, scores, labels, n_valid, frame_slot, frame_reset, frame_shift, F, K, S, T, s, p, 0,
                reinterpret_cast<float4*>(trk_box) + gs * T * 2, trk_score + gs * T,
                reinterpret_cast<int4*>(trk_meta) + gs * T, seq_meta + 2 * gs, out_id + gf * T, out_boxes + gf * T * 4,
                out_row + gf * T, count + gf);
}

}  // namespace moe

using namespace moe;

// the dynamic LDS of the kAssoc kernels at (K, T), raised past the 64 KiB default once per device; only a shape
// past the CU's 160 KiB is refused (none within the limits is: 85.4 KiB at K = 1024, T = 256)
static int track_assoc_lds(const std::string& what, const void* kernel, unsigned long long* done, int K, int T,
                           size_t* shmem) {
  *shmem = TrkAssocLds(K, T).total;
  if (*shmem + kTrkStaticLds > 160 * 1024) return fail(what + ": K / T too large for the 160 KiB of LDS");
  if (*shmem + kTrkStaticLds <= 64 * 1024) return 0;
  return allow_dyn_lds(kernel, (int)TrkAssocLds(kTrkMaxK, kTrkMaxT).total, done, (what + ": LDS attribute").c_str());
}

// assoc < 0: the entries without the argument (track_update_kernel); 0 / 1: rtdetr_track_update_assoc
static int track_update(const std::string& what, const float* boxes, const float* scores, const int32_t* labels,
                        const int32_t* n_valid, const int32_t* frame_slot, const int32_t* frame_reset,
                        const float* frame_shift, int F, int K, int S, int T, float track_high, float track_low,
                        float new_thr, float match_iou, float second_iou, int max_age, int min_hits, float alpha,
                        float beta, int class_agnostic, float* trk_box, float* trk_score, int32_t* trk_meta,
                        int32_t* seq_meta, int32_t* out_id, float* out_boxes, int32_t* count, int assoc,
                        hipStream_t stream) {
  if (assoc > 1) return fail(what + ": assoc must be 0 (greedy) or 1 (lsap)");
  if (F < 0 || K < 0 || S < 0 || F > kTrkMaxF || K > kTrkMaxK || S > kTrkMaxS || T < 1 || T > kTrkMaxT)
    return fail(what + ": need 0 <= F <= 1024, 0 <= K <= 1024, 0 <= S <= 1024, 1 <= T <= 256");
  if (track_high != track_high || track_low != track_low || new_thr != new_thr || match_iou != match_iou ||
      second_iou != second_iou || alpha != alpha || beta != beta)
    return fail(what + ": thresholds and gains must not be NaN");
  if (max_age < 0 || max_age > kTrkHitsCap || min_hits < 1 || min_hits > kTrkHitsCap)
    return fail(what + ": need 0 <= max_age <= 2^30 and 1 <= min_hits <= 2^30");
  if (F == 0) return 0;
  if (S < 1) return fail(what + ": need S >= 1 state slots with F > 0");
  if (!frame_slot || !frame_reset) return fail(what + ": NULL frame table");
  if (!trk_box || !trk_score || !trk_meta || !seq_meta) return fail(what + ": NULL state pointer");
  if (!count || (K > 0 && (!out_id || !out_boxes))) return fail(what + ": NULL output pointer");
  if (K > 0 && (!boxes || !scores || !labels)) return fail(what + ": NULL input pointer");
  if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(out_boxes) |
       reinterpret_cast<uintptr_t>(trk_box) | reinterpret_cast<uintptr_t>(trk_meta)) & 15)
    return fail(what + ": boxes, out_boxes, trk_box and trk_meta must be 16-byte aligned");
  size_t shmem = TrkLds(K, T).total;
  if (shmem > 64 * 1024) return fail(what + ": K / T too large for LDS");
  if (assoc >= 0) {
    static unsigned long long done = 0;  // per-device bitmask
    if (int rc = track_assoc_lds(what, reinterpret_cast<const void*>(track_update_assoc_kernel), &done, K, T, &shmem))
      return rc;
  }
  const int threads = (T + 63) / 64 * 64;
  TrkParams p;
  p.track_high = track_high;
  p.track_low = track_low;
  p.new_thr = new_thr;
  p.match_iou = match_iou;
  p.second_iou = second_iou;
  p.alpha = alpha;
  p.beta = beta;
  p.max_age = max_age;
  p.min_hits = min_hits;
  p.class_agnostic = class_agnostic != 0 ? 1 : 0;
  ProfScope prof(stream, PROF_TRACK,
                 (double)F * (K * 44.0 + (n_valid ? 4.0 : 0.0) + (frame_shift ? 8.0 : 0.0) + 12.0) +
                     (double)S * (T * 104.0 + 16.0));
  if (assoc >= 0) {
    MOE_LAUNCH(prof, track_update_assoc_kernel, dim3(S), dim3(threads), shmem, stream, boxes, scores, labels, n_valid,
               frame_slot, frame_reset, frame_shift, F, K, S, T, p, assoc, trk_box, trk_score, trk_meta, seq_meta,
               out_id, out_boxes, count);
    return check_launch(what.c_str());
  }
  MOE_LAUNCH(prof, track_update_kernel, dim3(S), dim3(threads), shmem, stream, boxes, scores, labels, n_valid,
             frame_slot, frame_reset, frame_shift, F, K, S, T, p, trk_box, trk_score, trk_meta, seq_meta, out_id,
             out_boxes, count);
  return check_launch(what.c_str());
}

extern "C" int rtdetr_track_update(const float* boxes, const float* scores, const int32_t* labels,
                                   const int32_t* n_valid, const int32_t* frame_slot, const int32_t* frame_reset,
                                   int F, int K, int S, int T, float track_high, float track_low, float new_thr,
                                   float match_iou, float second_iou, int max_age, int min_hits, float alpha,
                                   float beta, int class_agnostic, float* trk_box, float* trk_score,
                                   int32_t* trk_meta, int32_t* seq_meta, int32_t* out_id, float* out_boxes,
                                   int32_t* count, hipStream_t stream) {
  return track_update("rtdetr_track_update", boxes, scores, labels, n_valid, frame_slot, frame_reset, nullptr, F, K,
                      S, T, track_high, track_low, new_thr, match_iou, second_iou, max_age, min_hits, alpha, beta,
                      class_agnostic, trk_box, trk_score, trk_meta, seq_meta, out_id, out_boxes, count, -1, stream);
}

extern "C" int rtdetr_track_update_shift(const float* boxes, const float* scores, const int32_t* labels,
                                         const int32_t* n_valid, const int32_t* frame_slot,
                                         const int32_t* frame_reset, int F, int K, int S, int T, float track_high,
                                         float track_low, float new_thr, float match_iou, float second_iou,
                                         int max_age, int min_hits, float alpha, float beta, int class_agnostic,
                                         float* trk_box, float* trk_score, int32_t* trk_meta, int32_t* seq_meta,
                                         int32_t* out_id, float* out_boxes, int32_t* count, const float* frame_shift,
                                         hipStream_t stream) {
  return track_update("rtdetr_track_update_shift", boxes, scores, labels, n_valid, frame_slot, frame_reset,
                      frame_shift, F, K, S, T, track_high, track_low, new_thr, match_iou, second_iou, max_age,
                      min_hits, alpha, beta, class_agnostic, trk_box, trk_score, trk_meta, seq_meta, out_id, out_boxes,
                      count, -1, stream);
}

extern "C" int rtdetr_track_update_assoc(const float* boxes, const float* scores, const int32_t* labels,
                                         const int32_t* n_valid, const int32_t* frame_slot,
                                         const int32_t* frame_reset, int F, int K, int S, int T, float track_high,
                                         float track_low, float new_thr, float match_iou, float second_iou,
                                         int max_age, int min_hits, float alpha, float beta, int class_agnostic,
                                         float* trk_box, float* trk_score, int32_t* trk_meta, int32_t* seq_meta,
                                         int32_t* out_id, float* out_boxes, int32_t* count, const float* frame_shift,
                                         int assoc, hipStream_t stream) {
  if (assoc < 0) return fail("rtdetr_track_update_assoc: assoc must be 0 (greedy) or 1 (lsap)");
  return track_update("rtdetr_track_update_assoc", boxes, scores, labels, n_valid, frame_slot, frame_reset,
                      frame_shift, F, K, S, T, track_high, track_low, new_thr, match_iou, second_iou, max_age,
                      min_hits, alpha, beta, class_agnostic, trk_box, trk_score, trk_meta, seq_meta, out_id, out_boxes,
                      count, assoc, stream);
}

// with_assoc: rtdetr_track_sweep_assoc (track_sweep_assoc_kernel, params_assoc required); else params_assoc is unused
static int track_sweep(const std::string& what, bool with_assoc, const float* boxes, const float* scores,
                       const int32_t* labels, const int32_t* n_valid, const int32_t* frame_slot,
                       const int32_t* frame_reset, int F, int K, int S, int T, int G, const float* params_f,
                       const int32_t* params_i, const int32_t* params_assoc, float* trk_box, float* trk_score,
                       int32_t* trk_meta, int32_t* seq_meta, int32_t* out_id, float* out_boxes, int32_t* out_row,
                       int32_t* count, const float* frame_shift, hipStream_t stream) {
  if (F < 0 || K < 0 || S < 0 || F > kTrkMaxF || K > kTrkMaxK || S > kTrkMaxS || T < 1 || T > kTrkMaxT)
    return fail(what + ": need 0 <= F <= 1024, 0 <= K <= 1024, 0 <= S <= 1024, 1 <= T <= 256");
  if (G < 1 || G > kTrkMaxG) return fail(what + ": need 1 <= G <= 1024 configurations");
  if (!params_f || !params_i || (with_assoc && !params_assoc)) return fail(what + ": NULL parameter table");
  if (F == 0) return 0;
  if (S < 1) return fail(what + ": need S >= 1 state slots with F > 0");
  if (!frame_slot || !frame_reset) return fail(what + ": NULL frame table");
  if (!trk_box || !trk_score || !trk_meta || !seq_meta) return fail(what + ": NULL state pointer");
  if (!count || !out_id || !out_boxes || !out_row) return fail(what + ": NULL output pointer");
  if (K > 0 && (!boxes || !scores || !labels)) return fail(what + ": NULL input pointer");
  if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(out_boxes) |
       reinterpret_cast<uintptr_t>(trk_box) | reinterpret_cast<uintptr_t>(trk_meta)) & 15)
    return fail(what + ": boxes, out_boxes, trk_box and trk_meta must be 16-byte aligned");
  size_t shmem = TrkLds(K, T).total;
  if (shmem > 64 * 1024) return fail(what + ": K / T too large for LDS");
  if (with_assoc) {
    static unsigned long long done = 0;  // per-device bitmask
    if (int rc = track_assoc_lds(what, reinterpret_cast<const void*>(track_sweep_assoc_kernel), &done, K, T, &shmem))
      return rc;
  }
  const int threads = (T + 63) / 64 * 64;
  // the inputs once (every configuration's workgroups read the same lines), the tables, and per configuration the
  // state read and written and the compact outputs
  ProfScope prof(stream, PROF_TRACK_SWEEP,
                 (double)F * (K * 24.0 + (n_valid ? 4.0 : 0.0) + (frame_shift ? 8.0 : 0.0) + 8.0) +
                     (double)G * ((kTrkSweepF + kTrkSweepI + (with_assoc ? 1 : 0)) * 4.0 +
                                  (double)S * (T * 104.0 + 16.0) + (double)F * (T * 24.0 + 4.0)));
  if (with_assoc) {
    MOE_LAUNCH(prof, track_sweep_assoc_kernel, dim3(S, G), dim3(threads), shmem, stream, boxes, scores, labels,
               n_valid, frame_slot, frame_reset, frame_shift, F, K, S, T, params_f, params_i, params_assoc, trk_box,
               trk_score, trk_meta, seq_meta, out_id, out_boxes, out_row, count);
    return check_launch(what.c_str());
  }
  MOE_LAUNCH(prof, track_sweep_kernel, dim3(S, G), dim3(threads), shmem, stream, boxes, scores, labels, n_valid,
             frame_slot, frame_reset, frame_shift, F, K, S, T, params_f, params_i, trk_box, trk_score, trk_meta,
             seq_meta, out_id, out_boxes, out_row, count);
  return check_launch(what.c_str());
}

extern "C" int rtdetr_track_sweep(const float* boxes, const float* scores, const int32_t* labels,
                                  const int32_t* n_valid, const int32_t* frame_slot, const int32_t* frame_reset,
                                  int F, int K, int S, int T, int G, const float* params_f, const int32_t* params_i,
                                  float* trk_box, float* trk_score, int32_t* trk_meta, int32_t* seq_meta,
                                  int32_t* out_id, float* out_boxes, int32_t* out_row, int32_t* count,
                                  const float* frame_shift, hipStream_t stream) {
  return track_sweep("rtdetr_track_sweep", false, boxes, scores, labels, n_valid, frame_slot, frame_reset, F, K, S, T,
                     G, params_f, params_i, nullptr, trk_box, trk_score, trk_meta, seq_meta, out_id, out_boxes,
                     out_row, count, frame_shift, stream);
}

extern "C" int rtdetr_track_sweep_assoc(const float* boxes, const float* scores, const int32_t* labels,
                                        const int32_t* n_valid, const int32_t* frame_slot,
                                        const int32_t* frame_reset, int F, int K, int S, int T, int G,
                                        const float* params_f, const int32_t* params_i, float* trk_box,
                                        float* trk_score, int32_t* trk_meta, int32_t* seq_meta, int32_t* out_id,
                                        float* out_boxes, int32_t* out_row, int32_t* count, const float* frame_shift,
                                        const int32_t* params_assoc, hipStream_t stream) {
  return track_sweep("rtdetr_track_sweep_assoc", true, boxes, scores, labels, n_valid, frame_slot, frame_reset, F, K,
                     S, T, G, params_f, params_i, params_assoc, trk_box, trk_score, trk_meta, seq_meta, out_id,
                     out_boxes, out_row, count, frame_shift, stream);
}
