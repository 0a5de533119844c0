"""HOTA (Luiten et al., IJCV 2021) for moteval.evaluate(..., hota=True): the
rule stated once in numpy / scipy, the metrics of a finished state, and the
device path that scores every frame in a workgroup of its own.

* ``hota_pass_a`` / ``hota_gas`` / ``hota_pass_b``: one frame of one sequence.
  The HIP kernels rtdetr_hota_pass_a / _gas / _pass_b (csrc/hota.hip) leave the
  same arrays bit for bit and are tested against these functions.
* ``hota_reference``: a sequence's frames through both passes, in any order.
* ``hota_metrics`` / ``combine_hota``: on the host, for both paths.
* ``run_reference_hota`` / ``run_device_hota``: moteval.evaluate's two paths.

The rule.  Dense indices, fp32 IoU and the ignore-region removal are
moteval.py's steps 1-2, unchanged: below, "rows" are the tracker rows that
remain, "truths" the scored ground-truth rows, gt_count / trk_count those of
moteval's step 8.  Unlike the CLEAR matching nothing here looks at the frame
before, so the frames of a sequence may run in ANY order -- that is what lets
the GPU give every frame a workgroup -- and the rule is written so that the
result is the same bits whatever the order:

 A. Every frame: sim = the fp32 IoU widened to fp64 [rows, truths].  A row's
    sum over the truths and a truth's sum over the rows are sequential fp64
    adds from 0.0 in ascending row order of the other side.  sim_iou = sim /
    ((rowsum + colsum) - sim) where that denominator exceeds
    np.finfo(float).eps, else 0.  pot_q[g][t] += int64(rint(sim_iou * 2^32)):
    an INTEGER accumulation, exact and commutative (a term is at most 2^32, so
    2^24 frames fit int64).  This fixed-point step is the one deliberate
    departure from TrackEval, which keeps a running fp64 sum whose last bits
    depend on the frame order; here parallel frames need integer atomics only.
    gt_count[g] / trk_count[t] += 1 per truth / row.
 G. gas[g][t] = fp64(pot_q) / fp64(2^32 (gt_count[g] + trk_count[t]) - pot_q),
    the denominator formed in int64, one IEEE fp64 division, rounded once to
    fp32; 0 where pot_q == 0.
 B. Every frame: score = gas[g][t] * iou, one fp32 multiply; the assignment on
    -score in moteval's orientation (_assign: the side with more rows first,
    tracker rows on a tie).  For each of the 19 thresholds ALPHA[a] an assigned
    pair counts iff float64(iou) >= ALPHA[a]: TP[a] += counted pairs, FN[a] +=
    truths - counted, FP[a] += rows - counted, mc[a][g][t] += 1 per counted
    pair.  The frame's loc partial [19]: the counted pairs' widened IoU added
    from 0.0 in ground-truth row order.  loc_sum[a] is the sum of the frames'
    partials from 0.0 IN FRAME ORDER -- this two-level order is part of the
    rule (TrackEval adds pair by pair into one running sum).
"""
from __future__ import annotations

import warnings

import numpy as np

from . import moteval
from .moteval import _assign, _rows, check_thr
from .track import _iou

N_ALPHA = 19
ALPHA = np.arange(0.05, 0.99, 0.05) - np.finfo(float).eps  # fp64 [19], the kernels are handed this table
Q32 = 1 << 32
# rtdetr_hota_*'s limits: M, K as rtdetr_mot_eval's; S * NG * NT cells per launch (mc: 19 int32 each, 152 MiB)
HOTA_MAX_K, HOTA_MAX_M, HOTA_MAX_F, HOTA_MAX_S, HOTA_MAX_CELLS = 1024, 256, 8192, 1024, 1 << 21
HOTA_ARRAYS = ("pot_q", "gt_count", "trk_count", "counts", "mc", "loc_sum")
HOTA_FIELDS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")
assert len(ALPHA) == N_ALPHA


def new_hota_state(NG: int, NT: int) -> dict:
    """An empty sequence state: pot_q int64 [NG, NT], gt_count int32 [NG], trk_count int32 [NT], counts int64
    [3, 19] (TP, FN, FP), mc int32 [19, NG, NT], loc_sum fp64 [19]."""
    NG, NT = int(NG), int(NT)
    return {"pot_q": np.zeros((NG, NT), np.int64), "gt_count": np.zeros(NG, np.int32),
            "trk_count": np.zeros(NT, np.int32), "counts": np.zeros((3, N_ALPHA), np.int64),
            "mc": np.zeros((N_ALPHA, NG, NT), np.int32), "loc_sum": np.zeros(N_ALPHA, np.float64)}


def hota_states_equal(a: dict, b: dict) -> bool:
    """Bit for bit: the fp64 sums compared as int64."""
    for k in HOTA_ARRAYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            return False
        if k == "loc_sum":
            x, y = x.view(np.int64), y.view(np.int64)
        if not np.array_equal(x, y):
            return False
    return True


def frame_rows(gt, trk, NG, NT, thr):
    """moteval's steps 1-2 -> (g of the truths [m], t of the rows [k], iou fp32 [k, m], keep bool over all tracker
    rows)."""
    f32 = np.float32
    thr32 = f32(thr)
    gb, gi, gf, tb, ti = _rows(gt, trk, NG, NT)
    iou = _iou(tb, gb)
    keep = np.ones(len(ti), bool)
    scored = gf != 0
    if not scored.all():
        ts, gs = _assign(np.where(iou >= thr32, -iou, f32(0)).astype(f32))
        for t, g in zip(ts, gs):
            if not scored[g] and iou[t, g] >= thr32:
                keep[t] = False
    tl, gl = np.nonzero(keep)[0], np.nonzero(scored)[0]
    return gi[gl], ti[tl], np.ascontiguousarray(iou[np.ix_(tl, gl)]).reshape(len(tl), len(gl)), keep


def hota_pass_a(state, gt, trk, thr=0.5):
    """Pass A of one frame: pot_q, gt_count and trk_count of ``state`` (new_hota_state), in place."""
    NG, NT = state["pot_q"].shape
    g, t, iou, _ = frame_rows(gt, trk, NG, NT, check_thr(thr))
    sim = iou.astype(np.float64)
    rowsum, colsum = np.zeros(len(t), np.float64), np.zeros(len(g), np.float64)
    for j in range(len(g)):  # a row's sum: sequential over the truths in row order
        rowsum = rowsum + sim[:, j]
    for q in range(len(t)):  # a truth's sum: sequential over the rows in row order
        colsum = colsum + sim[q, :]
    den = (rowsum[:, None] + colsum[None, :]) - sim
    ok = den > np.finfo(float).eps
    sim_iou = np.where(ok, sim / np.where(ok, den, 1.0), 0.0)
    state["pot_q"][g[None, :], t[:, None]] += np.rint(sim_iou * float(Q32)).astype(np.int64)
    state["gt_count"][g] += 1
    state["trk_count"][t] += 1


def hota_gas(state):
    """The global alignment score fp32 [NG, NT] of a state whose pass A is complete."""
    p = state["pot_q"].astype(np.int64)
    n = state["gt_count"].astype(np.int64)[:, None] + state["trk_count"].astype(np.int64)[None, :]
    den = (n * Q32 - p).astype(np.float64)
    ok = p != 0  # then den >= p > 0: a frame's term is at most 2^32 and is counted on both sides
    return np.where(ok, p.astype(np.float64) / np.where(ok, den, 1.0), 0.0).astype(np.float32)


def hota_pass_b(state, gas, gt, trk, thr=0.5):
    """Pass B of one frame: counts and mc of ``state`` in place -> the frame's loc partial fp64 [19]."""
    NG, NT = state["pot_q"].shape
    g, t, iou, _ = frame_rows(gt, trk, NG, NT, check_thr(thr))
    score = (gas[g[None, :], t[:, None]].astype(np.float32) * iou).astype(np.float32)
    ts, gs = _assign(-score)
    order = np.argsort(gs, kind="stable")  # ground-truth row order
    ts, gs = ts[order], gs[order]
    pair = iou[ts, gs].astype(np.float64)
    part = np.zeros(N_ALPHA, np.float64)
    for a in range(N_ALPHA):
        hit = pair >= ALPHA[a]
        n = int(hit.sum())
        state["counts"][0, a] += n
        state["counts"][1, a] += len(g) - n
        state["counts"][2, a] += len(t) - n
        state["mc"][a, g[gs[hit]], t[ts[hit]]] += 1
        acc = np.float64(0.0)
        for v in pair[hit]:
            acc = acc + v
        part[a] = acc
    return part


def reduce_loc(parts):
    """loc_sum fp64 [19] of a sequence's loc partials [F, 19]: sequential adds from 0.0 in frame order."""
    acc = np.zeros(N_ALPHA, np.float64)
    for p in np.asarray(parts, np.float64).reshape(-1, N_ALPHA):
        acc = acc + p
    return acc


def hota_reference(frames, NG, NT, thr=0.5, order=None, order_b=None):
    """A sequence's final state by the reference.  ``frames``: [(gt boxes, g, flags, trk boxes, t)].  ``order`` /
    ``order_b``: the order pass A / pass B visit the frames in (any permutation gives the same bits).  The state
    also carries "gas" fp32 [NG, NT] and "loc_part" fp64 [F, 19]."""
    st = new_hota_state(NG, NT)
    order = list(range(len(frames))) if order is None else list(order)
    order_b = order if order_b is None else list(order_b)
    for f in order:
        gb, gi, gf, tb, ti = frames[f]
        hota_pass_a(st, (gb, gi, gf), (tb, ti), thr)
    gas = hota_gas(st)
    parts = np.zeros((len(frames), N_ALPHA), np.float64)
    for f in order_b:
        gb, gi, gf, tb, ti = frames[f]
        parts[f] = hota_pass_b(st, gas, (gb, gi, gf), (tb, ti), thr)
    st["loc_sum"] = reduce_loc(parts)
    st["gas"], st["loc_part"] = gas, parts
    return st


# ---------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------
def _finish(tp, fn, fp, loc, ass_a, ass_re, ass_pr) -> dict:
    """The dict of hota_metrics / combine_hota from the per-threshold counts and association scores."""
    tp, fn, fp = (np.asarray(v, np.int64) for v in (tp, fn, fp))
    loc = np.asarray(loc, np.float64)
    arr = {"AssA": np.asarray(ass_a, np.float64), "AssRe": np.asarray(ass_re, np.float64),
           "AssPr": np.asarray(ass_pr, np.float64)}
    arr["DetA"] = tp / np.maximum(1, tp + fn + fp)
    arr["DetRe"] = tp / np.maximum(1, tp + fn)
    arr["DetPr"] = tp / np.maximum(1, tp + fp)
    arr["LocA"] = np.maximum(1e-10, loc) / np.maximum(1e-10, tp.astype(np.float64))
    arr["HOTA"] = np.sqrt(arr["DetA"] * arr["AssA"])
    m = {k: float(np.mean(arr[k])) for k in HOTA_FIELDS}
    m["HOTA(0)"], m["LocA(0)"] = float(arr["HOTA"][0]), float(arr["LocA"][0])
    m["HOTALocA(0)"] = float(arr["HOTA"][0] * arr["LocA"][0])
    m["alpha"] = [float(a) for a in ALPHA]
    m["arrays"] = {**{k: [float(v) for v in arr[k]] for k in HOTA_FIELDS},
                   "TP": [int(v) for v in tp], "FN": [int(v) for v in fn], "FP": [int(v) for v in fp],
                   "loc_sum": [float(v) for v in loc]}
    return m


def hota_metrics(state) -> dict:
    """The HOTA family of one sequence's finished state.  Per threshold: DetA = TP / (TP + FN + FP), DetRe = TP /
    (TP + FN), DetPr = TP / (TP + FP); AssA = sum mc * mc / max(1, gt_count + trk_count - mc) / max(1, TP), AssRe
    with gt_count and AssPr with trk_count as the denominator; LocA = max(1e-10, loc_sum) / max(1e-10, TP) (1.0
    without a counted pair, as TrackEval has it); HOTA = sqrt(DetA * AssA); an empty denominator gives 0.0.  ->
    the means over the 19 thresholds under HOTA_FIELDS, "HOTA(0)", "LocA(0)", "HOTALocA(0)" (the lowest
    threshold), "alpha" and "arrays": the 19 values of every field and of TP, FN, FP, loc_sum."""
    counts = np.asarray(state["counts"]).astype(np.int64)
    mc = np.asarray(state["mc"]).astype(np.float64)
    gc = np.asarray(state["gt_count"]).astype(np.float64)[None, :, None]
    tc = np.asarray(state["trk_count"]).astype(np.float64)[None, None, :]
    tp = np.maximum(1, counts[0]).astype(np.float64)
    ass = [(mc * (mc / np.maximum(1.0, d))).reshape(N_ALPHA, -1).sum(1) / tp for d in (gc + tc - mc, gc, tc)]
    return _finish(counts[0], counts[1], counts[2], np.asarray(state["loc_sum"]).reshape(N_ALPHA), *ass)


def combine_hota(metrics) -> dict:
    """The combined row of several sequences' hota_metrics, in the order given, as TrackEval combines sequences:
    TP, FN, FP and loc_sum are summed, AssA / AssRe / AssPr averaged with TP as the weight (sum x * TP / max(1, sum
    TP)) per threshold, and the rest derived from those."""
    tp, fn, fp = (np.zeros(N_ALPHA, np.int64) for _ in range(3))
    loc = np.zeros(N_ALPHA, np.float64)
    ass = {k: np.zeros(N_ALPHA, np.float64) for k in ("AssA", "AssRe", "AssPr")}
    for x in metrics:
        a = x["arrays"]
        w = np.asarray(a["TP"], np.int64)
        tp, fn, fp = tp + w, fn + np.asarray(a["FN"], np.int64), fp + np.asarray(a["FP"], np.int64)
        loc = loc + np.asarray(a["loc_sum"], np.float64)
        for k in ass:
            ass[k] = ass[k] + np.asarray(a[k], np.float64) * w
    den = np.maximum(1.0, tp.astype(np.float64))
    return _finish(tp, fn, fp, loc, *(ass[k] / den for k in ("AssA", "AssRe", "AssPr")))


# ---------------------------------------------------------------------------
# the device state and moteval.evaluate's two paths
# ---------------------------------------------------------------------------
class HotaEvalState:
    """S sequences' HOTA state on the device (the layout include/moe_hip.h documents), zeroed:
      pot_q  int64 [S, NG, NT]    gt_count int32 [S, NG]          trk_count int32 [S, NT]
      gas    fp32  [S, NG, NT]    counts   int64 [S, 3, 19]       mc        int32 [S, 19, NG, NT]
    one status word for all launches (0: fine) and ALPHA as the kernels' table of 19 doubles."""

    def __init__(self, S: int, NG: int, NT: int, device):
        import torch

        self.S, self.NG, self.NT = int(S), int(NG), int(NT)
        if not (1 <= self.S <= HOTA_MAX_S and self.NG >= 1 and self.NT >= 1
                and self.S * self.NG * self.NT <= HOTA_MAX_CELLS):
            raise ValueError(f"HotaEvalState: need 1 <= S <= {HOTA_MAX_S}, NG >= 1, NT >= 1 and S * NG * NT <= "
                             f"{HOTA_MAX_CELLS}, got {self.S}, {self.NG}, {self.NT}")
        S, NG, NT = self.S, self.NG, self.NT
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)  # noqa: E731
        self.pot_q = z((S, NG, NT), torch.int64)
        self.gt_count, self.trk_count = z((S, NG), torch.int32), z((S, NT), torch.int32)
        self.gas = z((S, NG, NT), torch.float32)
        self.counts = z((S, 3, N_ALPHA), torch.int64)
        self.mc = z((S, N_ALPHA, NG, NT), torch.int32)
        self.status = z((1,), torch.int32)
        self.alpha = torch.from_numpy(ALPHA.copy()).to(device)

    def export(self, s: int, loc_part) -> dict:
        """Slot s as the reference's named arrays; ``loc_part`` fp64 [F, 19]: its frames' partials in frame order."""
        out = {k: getattr(self, k)[s].cpu().numpy().copy() for k in ("pot_q", "gt_count", "trk_count", "counts", "mc")}
        out["gas"] = self.gas[s].cpu().numpy().copy()
        out["loc_part"] = np.asarray(loc_part, np.float64).reshape(-1, N_ALPHA)
        out["loc_sum"] = reduce_loc(out["loc_part"])
        return out


def run_reference_hota(seqs, thr) -> list:
    """Every sequence's final state by the reference (seqs: moteval.dense_sequence's)."""
    return [hota_reference(sq["frames"], sq["NG"], sq["NT"], thr) for sq in seqs]


def hota_groups(seqs):
    """Consecutive sequences grouped so that a group's padded tables stay under HOTA_MAX_CELLS (and HOTA_MAX_S)
    -> [(first, last + 1)]; a single sequence over the budget is a group of its own."""
    groups, lo, ng, nt = [], 0, 1, 1
    for j, sq in enumerate(seqs):
        ng2, nt2 = max(ng, sq["NG"], 1), max(nt, sq["NT"], 1)
        if j > lo and ((j - lo + 1) * ng2 * nt2 > HOTA_MAX_CELLS or j - lo + 1 > HOTA_MAX_S):
            groups.append((lo, j))
            lo, ng2, nt2 = j, max(sq["NG"], 1), max(sq["NT"], 1)
        ng, nt = ng2, nt2
    if lo < len(seqs):
        groups.append((lo, len(seqs)))
    return groups


def run_device_hota(seqs, thr, device) -> list:
    """Every sequence's final state by the HIP kernels.  Per group of sequences (hota_groups): the chunks of at
    most HOTA_MAX_F frames (moteval.pack_chunks) are uploaded and stay on the device, pass A runs over every
    chunk, one launch builds gas, pass B runs over every chunk, and the [F, 19] loc partials are reduced on the
    host in frame order.  (Uploading every chunk again for pass B instead of keeping it measured the same: DESIGN.md
    section 30.)  A single sequence over the table budget is scored by the reference."""
    import torch

    from ..moe import _lib

    states = [None] * len(seqs)
    for lo, hi in hota_groups(seqs):
        group = seqs[lo:hi]
        NG, NT = max(1, *(sq["NG"] for sq in group)), max(1, *(sq["NT"] for sq in group))
        if len(group) * NG * NT > HOTA_MAX_CELLS:
            warnings.warn(f"HOTA: a sequence's {NG} x {NT} table is over the device budget; scored on the host")
            states[lo] = hota_reference(group[0]["frames"], group[0]["NG"], group[0]["NT"], thr)
            continue
        st = HotaEvalState(len(group), NG, NT, device)
        chunks, _, _ = moteval.pack_chunks(group, HOTA_MAX_F)
        on_dev = [{k: torch.from_numpy(v).to(device) for k, v in c.items() if k != "frame_reset"} for c in chunks]
        keeps = [torch.empty(t["trk_idx"].shape, dtype=torch.uint8, device=device) for t in on_dev]
        for t, keep in zip(on_dev, keeps):
            _lib.hota_pass_a(st, t, keep, thr)
        _lib.hota_gas(st)
        parts = [_lib.hota_pass_b(st, t, keep) for t, keep in zip(on_dev, keeps)]
        _lib.hota_check(st)
        parts = [p.cpu().numpy() for p in parts]
        for j, sq in enumerate(group):
            loc = np.concatenate([p[c["frame_slot"] == j] for c, p in zip(chunks, parts)] or
                                 [np.zeros((0, N_ALPHA))])
            full = st.export(j, loc)
            n, k = sq["NG"], sq["NT"]
            states[lo + j] = {"pot_q": full["pot_q"][:n, :k], "gt_count": full["gt_count"][:n],
                              "trk_count": full["trk_count"][:k], "counts": full["counts"],
                              "mc": full["mc"][:, :n, :k], "loc_sum": full["loc_sum"], "gas": full["gas"][:n, :k],
                              "loc_part": full["loc_part"]}
    return states
