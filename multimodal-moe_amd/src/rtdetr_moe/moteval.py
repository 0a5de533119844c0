"""Tracking evaluation (engine.track(..., gt=...), scripts/eval_tracks.py): the
CLEAR-MOT metrics and the identity metrics of a tracker's output against
MOTChallenge ground truth, the rule stated once.

* ``mot_reference``: one frame of one sequence, plain numpy and scipy.  The HIP
  kernel rtdetr_mot_eval (_lib.mot_eval) leaves the same state bit for bit and
  is tested against this function; it is also the evaluator of the CPU device
  and of MOE_TRACK_EVAL=0.
* ``MotEvalState``: the device buffers the kernel keeps a sequence's state in
  between launches, with an export to the reference's arrays.
* ``mot_metrics``: the metrics of a finished state, on the host, for both paths.
* ``load_gt`` / ``parse_mot`` / ``evaluate``: MOTChallenge files in, metrics out.
  ``evaluate(..., hota=True)`` adds HOTA, whose rule, reference and device path
  are hota.py's (it shares steps 1-2 and the dense indices below).

The rule.  The host maps a sequence's raw ids to dense indices: ground truth g
in [0, NG), tracker t in [0, NT).  A frame brings ground-truth rows (box xyxy
fp32, g, flag: 1 scored, 0 ignore region) and tracker rows (box xyxy fp32, t),
each index at most once per side (a duplicate is a ValueError before anything
runs).  Coordinates must be finite and 0 < thr <= 1.  Per frame:
 1. IoU of every tracker row with every ground-truth row: track.py's rule 3
    (track._iou: fp32, every operation rounded on its own, no FMA, inter / den
    if den > 0 else 0).
 2. Ignore regions, only in a frame that has a flag-0 row (MOTChallenge's
    preprocessing, as TrackEval does it with distractor classes): the
    assignment of ALL tracker rows against ALL ground-truth rows with cost
    -iou if iou >= thr else 0 is solved; a tracker row assigned to a flag-0 row
    with iou >= thr is removed; then the flag-0 rows are removed.
 3. CLEAR matching of the scored rows with the remaining tracker rows: score =
    iou, or 1000 + iou (one fp32 add) where prev_step[g] == t, or 0 where iou <
    thr; cost = -score; the assignment is solved and a pair with score > 0 is a
    match.  Both assignments are scipy.optimize.linear_sum_assignment of the
    cost matrix with the side that has more rows first (equal: tracker rows
    first) -- the orientation csrc/lsap.h's lsap_solve solves, ties included.
 4. counts (int64): TP, FN, FP, IDSW (a matched g whose last_ever[g] is set and
    is not the tracker index it is matched to now), removed (step 2), frames.
 5. per_gt[g] = frames present (scored), frames matched, frag: + 1 when g is
    matched now and was not matched in its previous present frame (so the first
    match counts, and Frag = sum(max(frag - 1, 0))).
 6. motp_sum (fp64) += the matched pairs' iou widened from fp32, one add per
    pair, in frame order and within a frame in ground-truth row order.
 7. prev_step holds this frame's matches only; every other entry is cleared: -1,
    or -2 for an index that is absent since a frame it was matched in (cleared
    all the same -- no tracker index equals it -- it only carries step 5's
    "previous present frame" over the absence).  last_ever[g] = t on a match.
 8. pmc[g][t] += 1 for EVERY pair of a scored row and a remaining tracker row
    with iou >= thr, matched or not; gt_count[g] += 1 per scored row,
    trk_count[t] += 1 per remaining tracker row.
"""
from __future__ import annotations

import os
from pathlib import Path

import numpy as np

from .track import _iou

MOT_MAX_K, MOT_MAX_M, MOT_MAX_NG, MOT_MAX_NT, MOT_MAX_F, MOT_MAX_S = 1024, 256, 1024, 4096, 1024, 1024
MOT_MAX_FRAMES = 1 << 24  # pmc's counts are exact in fp32 up to here
COUNTS = ("TP", "FN", "FP", "IDSW", "removed", "frames")  # counts[0:6]; [6:8] are spare and stay 0
STATE_ARRAYS = ("prev_step", "last_ever", "per_gt", "counts", "motp_sum", "pmc", "gt_count", "trk_count")
INT_METRICS = ("TP", "FN", "FP", "IDSW", "removed", "frames", "GT", "MT", "PT", "ML", "Frag", "IDTP", "IDFN", "IDFP")


def new_state(NG: int, NT: int) -> dict:
    """An empty sequence state for NG ground-truth and NT tracker indices."""
    NG, NT = int(NG), int(NT)
    return {"prev_step": np.full(NG, -1, np.int32), "last_ever": np.full(NG, -1, np.int32),
            "per_gt": np.zeros((NG, 3), np.int32), "counts": np.zeros(8, np.int64),
            "motp_sum": np.zeros(1, np.float64), "pmc": np.zeros((NG, NT), np.int32),
            "gt_count": np.zeros(NG, np.int32), "trk_count": np.zeros(NT, np.int32)}


def copy_state(state: dict) -> dict:
    return {k: np.array(state[k], copy=True) for k in STATE_ARRAYS}


def states_equal(a: dict, b: dict) -> bool:
    """Bit for bit: the fp64 sum compared as int64."""
    for k in STATE_ARRAYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            return False
        if k == "motp_sum":
            x, y = x.view(np.int64), y.view(np.int64)
        if not np.array_equal(x, y):
            return False
    return True


def check_thr(thr) -> float:
    thr = float(thr)
    if not 0.0 < thr <= 1.0:
        raise ValueError(f"the evaluation IoU must be in (0, 1], got {thr}")
    return thr


def _rows(gt, trk, NG, NT):
    """The frame's five arrays, checked (the rule's preconditions)."""
    gb = np.ascontiguousarray(np.asarray(gt[0], dtype=np.float32)).reshape(-1, 4)
    gi = np.asarray(gt[1]).reshape(-1).astype(np.int64)
    gf = np.asarray(gt[2]).reshape(-1).astype(np.int32)
    tb = np.ascontiguousarray(np.asarray(trk[0], dtype=np.float32)).reshape(-1, 4)
    ti = np.asarray(trk[1]).reshape(-1).astype(np.int64)
    if not (len(gb) == len(gi) == len(gf)) or len(tb) != len(ti):
        raise ValueError("a frame's boxes, indices and flags must have one length per side")
    for name, idx, n in (("ground-truth", gi, NG), ("tracker", ti, NT)):
        if len(idx) and (idx.min() < 0 or idx.max() >= n):
            raise ValueError(f"{name} index outside [0, {n})")
        if len(np.unique(idx)) != len(idx):
            raise ValueError(f"a {name} index appears twice in one frame")
    if not (np.isfinite(gb).all() and np.isfinite(tb).all()):
        raise ValueError("box coordinates must be finite")
    return gb, gi, gf, tb, ti


def _assign(cost):
    """linear_sum_assignment of cost fp32 [nt, ng] in the rule's orientation -> (tracker rows, ground-truth rows)."""
    from scipy.optimize import linear_sum_assignment

    nt, ng = cost.shape
    if nt == 0 or ng == 0:
        z = np.zeros(0, np.int64)
        return z, z
    if nt >= ng:
        r, c = linear_sum_assignment(cost.astype(np.float64))
        return r, c
    r, c = linear_sum_assignment(np.ascontiguousarray(cost.T).astype(np.float64))
    return c, r


def frame_scores(prev_step, gi, ti, iou, thr):
    """Step 3's score fp32 [nt, ng] of tracker rows ``ti`` against scored rows ``gi``; ``iou`` fp32 [nt, ng]."""
    f32 = np.float32
    same = prev_step[gi][None, :] == ti[:, None]
    score = np.where(same, f32(1000) + iou, iou).astype(f32)
    return np.where(iou < f32(thr), f32(0), score).astype(f32)


def mot_reference(state, gt, trk, thr=0.5):
    """One frame of one sequence.  ``gt``: (boxes fp32 [m, 4] xyxy, index [m],
    flag [m]); ``trk``: (boxes fp32 [k, 4] xyxy, index [k]).  Updates ``state``
    (new_state) in place -> the frame's matches [(g, t)] in ground-truth row
    order."""
    f32 = np.float32
    thr32 = f32(check_thr(thr))
    NG, NT = state["pmc"].shape
    gb, gi, gf, tb, ti = _rows(gt, trk, NG, NT)
    prev, last, per_gt, counts = state["prev_step"], state["last_ever"], state["per_gt"], state["counts"]
    iou = _iou(tb, gb)  # 1. [nt, ng]
    keep = np.ones(len(ti), bool)
    scored = gf != 0
    if not scored.all():  # 2. ignore regions
        ts, gs = _assign(np.where(iou >= thr32, -iou, f32(0)).astype(f32))
        for t, g in zip(ts, gs):
            if not scored[g] and iou[t, g] >= thr32:
                keep[t] = False
    tl, gl = np.nonzero(keep)[0], np.nonzero(scored)[0]
    sub = iou[np.ix_(tl, gl)]
    score = frame_scores(prev, gi[gl], ti[tl], sub, thr32)  # 3.
    ts, gs = _assign(-score)
    match = np.full(len(gl), -1, np.int64)  # per scored row: its row of tl
    for t, g in zip(ts, gs):
        if score[t, g] > 0:
            match[g] = t
    # 7. everything that is not matched now is cleared
    before = prev.copy()
    held = (prev >= 0) | (prev == -2)
    prev[held], prev[~held] = -2, -1
    out = []
    for j, g in enumerate(gi[gl]):  # ground-truth row order
        per_gt[g, 0] += 1
        state["gt_count"][g] += 1
        if match[j] < 0:
            prev[g] = -1
            continue
        t = int(ti[tl[match[j]]])
        per_gt[g, 1] += 1
        if before[g] == -1:  # 5. not matched in its previous present frame
            per_gt[g, 2] += 1
        if last[g] >= 0 and last[g] != t:
            counts[3] += 1
        prev[g], last[g] = t, t
        state["motp_sum"][0] = state["motp_sum"][0] + np.float64(sub[match[j], j])  # 6.
        out.append((int(g), t))
    n = len(out)
    counts[0] += n
    counts[1] += len(gl) - n
    counts[2] += len(tl) - n
    counts[4] += len(ti) - len(tl)
    counts[5] += 1
    # 8. the identity table
    state["trk_count"][ti[tl]] += 1
    ts, gs = np.nonzero(sub >= thr32)
    state["pmc"][gi[gl][gs], ti[tl][ts]] += 1
    return out


def _ratio(a, b) -> float:
    return float(a) / float(b) if b else 0.0


def _derive(m: dict) -> dict:
    """The ratios from the integer counts and motp_sum (an empty denominator gives 0.0)."""
    m["MOTA"] = _ratio(m["TP"] - m["FP"] - m["IDSW"], m["TP"] + m["FN"])
    m["MOTP"] = _ratio(m["motp_sum"], m["TP"])
    m["Recall"] = _ratio(m["TP"], m["TP"] + m["FN"])
    m["Precision"] = _ratio(m["TP"], m["TP"] + m["FP"])
    m["IDF1"] = _ratio(2 * m["IDTP"], 2 * m["IDTP"] + m["IDFP"] + m["IDFN"])
    m["IDP"] = _ratio(m["IDTP"], m["IDTP"] + m["IDFP"])
    m["IDR"] = _ratio(m["IDTP"], m["IDTP"] + m["IDFN"])
    return m


def idtp(pmc) -> int:
    """The largest sum of pmc over one-to-one assignments of ground-truth to tracker indices."""
    from scipy.optimize import linear_sum_assignment

    pmc = np.asarray(pmc)
    if pmc.size == 0:
        return 0
    r, c = linear_sum_assignment(-pmc.astype(np.float32))
    return int(pmc[r, c].astype(np.int64).sum())


def mot_metrics(state) -> dict:
    """The metrics of one sequence's state after its last frame: the counts
    (INT_METRICS; GT = the ground-truth indices seen; MT / ML: matched / present
    above 0.8 / below 0.2, compared in integers, PT the rest), motp_sum, and
    MOTA = (TP - FP - IDSW) / (TP + FN), MOTP = motp_sum / TP, Recall,
    Precision, IDF1 = 2 IDTP / (2 IDTP + IDFP + IDFN), IDP, IDR; an empty
    denominator gives 0.0.  IDTP is the maximum over one-to-one assignments of
    ground-truth to tracker indices of sum pmc (an assignment on -pmc in fp32,
    exact up to 2^24 frames: more are refused), IDFN = sum gt_count - IDTP, IDFP
    = sum trk_count - IDTP.  This is the standard identity-metric formulation
    (Ristani et al.) with its constant terms taken out: there an index left
    without a partner costs its own count, which is what pairing it with pmc =
    0 costs here, so IDFN + IDFP = sum gt_count + sum trk_count - 2 IDTP in
    both and the optimum is the same."""
    counts = np.asarray(state["counts"]).astype(np.int64)
    if int(counts[5]) > MOT_MAX_FRAMES:
        raise ValueError(f"mot_metrics: {int(counts[5])} frames; the identity table is exact up to 2^24")
    m = {k: int(counts[i]) for i, k in enumerate(COUNTS)}
    per_gt = np.asarray(state["per_gt"]).astype(np.int64)
    present, matched = per_gt[:, 0], per_gt[:, 1]
    seen = present > 0
    mt = seen & (5 * matched > 4 * present)
    ml = seen & (5 * matched < present)
    m["GT"], m["MT"], m["ML"] = int(seen.sum()), int(mt.sum()), int(ml.sum())
    m["PT"] = m["GT"] - m["MT"] - m["ML"]
    m["Frag"] = int(np.maximum(per_gt[:, 2] - 1, 0).sum())
    m["IDTP"] = idtp(state["pmc"])
    m["IDFN"] = int(np.asarray(state["gt_count"]).astype(np.int64).sum()) - m["IDTP"]
    m["IDFP"] = int(np.asarray(state["trk_count"]).astype(np.int64).sum()) - m["IDTP"]
    m["motp_sum"] = float(np.asarray(state["motp_sum"]).reshape(-1)[0])
    return _derive(m)


def combine(metrics) -> dict:
    """The combined row of several sequences' metrics, in the order given: the
    integer counts and motp_sum are summed and the ratios derived from the sums
    (an empty denominator, no sequence at all included, gives 0.0)."""
    m = {k: 0 for k in INT_METRICS}
    m["motp_sum"] = 0.0
    for x in metrics:
        for k in INT_METRICS:
            m[k] += int(x[k])
        m["motp_sum"] += float(x["motp_sum"])
    return _derive(m)


# ---------------------------------------------------------------------------
# the device state
# ---------------------------------------------------------------------------
class MotEvalState:
    """S sequences' evaluation state on the device, between launches of
    rtdetr_mot_eval (the layout include/moe_hip.h documents):
      prev_step int32 [S, NG]      last_ever int32 [S, NG]     per_gt int32 [S, NG, 3]
      counts    int64 [S, 8]       motp_sum  fp64  [S]         pmc    int32 [S, NG, NT]
      gt_count  int32 [S, NG]      trk_count int32 [S, NT]
    and one status word for all launches (0: fine).
    """

    def __init__(self, S: int, NG: int, NT: int, device):
        import torch

        self.S, self.NG, self.NT = int(S), int(NG), int(NT)
        if not (1 <= self.S <= MOT_MAX_S and 1 <= self.NG <= MOT_MAX_NG and 1 <= self.NT <= MOT_MAX_NT):
            raise ValueError(f"MotEvalState: need 1 <= S <= {MOT_MAX_S}, 1 <= NG <= {MOT_MAX_NG} and "
                             f"1 <= NT <= {MOT_MAX_NT}, got {self.S}, {self.NG}, {self.NT}")
        S, NG, NT = self.S, self.NG, self.NT
        i32 = dict(dtype=torch.int32, device=device)
        self.prev_step = torch.full((S, NG), -1, **i32)
        self.last_ever = torch.full((S, NG), -1, **i32)
        self.per_gt = torch.zeros((S, NG, 3), **i32)
        self.counts = torch.zeros((S, 8), dtype=torch.int64, device=device)
        self.motp_sum = torch.zeros((S,), dtype=torch.float64, device=device)
        self.pmc = torch.zeros((S, NG, NT), **i32)
        self.gt_count = torch.zeros((S, NG), **i32)
        self.trk_count = torch.zeros((S, NT), **i32)
        self.status = torch.zeros((1,), **i32)

    def tensors(self):
        return (self.prev_step, self.last_ever, self.per_gt, self.counts, self.motp_sum, self.pmc, self.gt_count,
                self.trk_count)

    def export(self, s: int) -> dict:
        """Slot s as the reference's named arrays (new_state's layout)."""
        out = {k: t[s].cpu().numpy().copy() for k, t in zip(STATE_ARRAYS, self.tensors())}
        out["motp_sum"] = out["motp_sum"].reshape(1)
        return out

    def load(self, s: int, state: dict):
        """Slot s from the reference's named arrays."""
        import torch

        for k, t in zip(STATE_ARRAYS, self.tensors()):
            t[s].copy_(torch.from_numpy(np.ascontiguousarray(state[k]).reshape(tuple(t[s].shape))))


# ---------------------------------------------------------------------------
# MOTChallenge files
# ---------------------------------------------------------------------------
def _xyxy(x, y, w, h):
    """MOTChallenge x, y, w, h -> fp32 xyxy: the four values rounded to fp32, then x + w and y + h in fp32."""
    x, y, w, h = (np.asarray(v, dtype=np.float64).astype(np.float32) for v in (x, y, w, h))
    return np.stack([x, y, x + w, y + h], axis=-1).astype(np.float32).reshape(-1, 4)


def _parse(text, what, defaults):
    """The numeric rows of MOTChallenge text, missing trailing columns filled in from ``defaults`` (columns 6..)."""
    rows = []
    for no, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if not line:
            continue
        parts = [p for p in line.replace(" ", ",").split(",") if p != ""]
        if len(parts) < 6:
            raise ValueError(f"{what}, line {no}: need at least frame,id,x,y,w,h")
        try:
            v = [float(p) for p in parts[:9]]
        except ValueError:
            raise ValueError(f"{what}, line {no}: not numeric: {line!r}") from None
        v += list(defaults[len(v) - 6:])
        if v[0] < 1 or v[0] != int(v[0]) or v[1] != int(v[1]):
            raise ValueError(f"{what}, line {no}: the frame must be an integer >= 1 and the id an integer")
        rows.append(v)
    return np.asarray(rows, dtype=np.float64).reshape(-1, 9)


def _frames(rows, flags, what):
    """{frame: (boxes fp32 [m, 4], ids int64 [m], flags int32 [m])}, a frame's rows in file order."""
    out = {}
    order = np.argsort(rows[:, 0], kind="stable")
    rows, flags = rows[order], flags[order]
    frames = rows[:, 0].astype(np.int64)
    for f in np.unique(frames):
        sel = frames == f
        ids = rows[sel, 1].astype(np.int64)
        if len(np.unique(ids)) != len(ids):
            raise ValueError(f"{what}: an id appears twice in frame {int(f)}")
        boxes = _xyxy(rows[sel, 2], rows[sel, 3], rows[sel, 4], rows[sel, 5])
        if not np.isfinite(boxes).all():
            raise ValueError(f"{what}: a box of frame {int(f)} is not finite")
        out[int(f)] = (boxes, ids, flags[sel].astype(np.int32))
    return out


def parse_gt(text, classes=None, ignore_classes=(), what="ground truth") -> dict:
    """MOTChallenge ground-truth text -> {frame: (boxes, ids, flags)} (load_gt's rules)."""
    rows = _parse(text, what, (1.0, 1.0, 1.0))
    cls = rows[:, 7].astype(np.int64)
    ignore = np.isin(cls, np.asarray(list(ignore_classes), dtype=np.int64))
    keep = rows[:, 6] != 0
    if classes is not None:
        keep &= np.isin(cls, np.asarray(list(classes), dtype=np.int64))
    keep |= ignore
    flags = np.where(ignore, 0, 1).astype(np.int32)
    return _frames(rows[keep], flags[keep], what)


def parse_mot(text, what="results") -> dict:
    """A tracker's MOTChallenge text (predictor.mot_lines) -> {frame: (boxes fp32 [k, 4] xyxy, ids int64 [k])}."""
    rows = _parse(text, what, (1.0, -1.0, -1.0))
    return {f: (b, i) for f, (b, i, _) in _frames(rows, np.ones(len(rows), np.int32), what).items()}


def load_gt(root, keys, classes=None, ignore_classes=()) -> dict:
    """MOTChallenge ground truth of the sequences ``keys`` under ``root``:
    ``<root>/<key>/gt/gt.txt``, or else ``<root>/<key>.txt``.  A line is
    frame,id,x,y,w,h,conf,class,visibility (frame 1-based; missing trailing
    columns are 1,1,1).  Rows of ``ignore_classes`` become ignore regions (flag
    0); other rows with conf == 0 or a class not in ``classes`` (None: every
    class) are dropped.  -> {key: {frame: (boxes fp32 [m, 4] xyxy, ids int64
    [m], flags int32 [m])}}; a frame without lines has no entry and no truths.
    A missing file is a FileNotFoundError naming both paths; an id twice in one
    frame is a ValueError."""
    root = Path(root)
    out = {}
    for key in keys:
        a, b = root / key / "gt" / "gt.txt", root / (key + ".txt")
        path = a if a.is_file() else b
        if not path.is_file():
            raise FileNotFoundError(f"no ground truth for sequence {key!r}: neither {a} nor {b} exists")
        out[key] = parse_gt(path.read_text(), classes, ignore_classes, what=str(path))
    return out


def load_results(results, keys) -> dict:
    """{key: parse_mot(...)} from {key: MOT text} or a directory of <key>.txt files."""
    out = {}
    for key in keys:
        if isinstance(results, dict):
            if key not in results:
                raise ValueError(f"no results for sequence {key!r}")
            text, what = results[key], f"results of {key}"
        else:
            path = Path(results) / (key + ".txt")
            if not path.is_file():
                raise FileNotFoundError(f"no results for sequence {key!r}: {path} does not exist")
            text, what = path.read_text(), str(path)
        out[key] = parse_mot(text, what)
    return out


# ---------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------
def eval_on_gpu(dev) -> bool:
    """The evaluator runs in the HIP kernel on a GPU device unless MOE_TRACK_EVAL=0 asks for the reference."""
    return dev is not None and dev.type == "cuda" and os.environ.get("MOE_TRACK_EVAL", "1") != "0"


def dense_sequence(gt_frames: dict, trk_frames: dict) -> dict:
    """One sequence with its ids mapped to dense indices (ascending raw id):
    {"NG", "NT", "frames": [(gt boxes, g, flags, trk boxes, t)] for frame 1 ..
    the last frame either side has rows in}."""
    gids = sorted({int(i) for _, ids, _ in gt_frames.values() for i in ids})
    tids = sorted({int(i) for _, ids in trk_frames.values() for i in ids})
    gmap, tmap = {v: j for j, v in enumerate(gids)}, {v: j for j, v in enumerate(tids)}
    n = max([0, *gt_frames, *trk_frames])
    e4, e1 = np.zeros((0, 4), np.float32), np.zeros(0, np.int32)
    frames = []
    for f in range(1, n + 1):
        gb, gi, gf = gt_frames.get(f, (e4, e1, e1))
        tb, ti = trk_frames.get(f, (e4, e1))
        frames.append((gb, np.asarray([gmap[int(i)] for i in gi], np.int32), np.asarray(gf, np.int32),
                       tb, np.asarray([tmap[int(i)] for i in ti], np.int32)))
    return {"NG": len(gids), "NT": len(tids), "frames": frames}


def run_reference(seqs, thr) -> list:
    """Every sequence's final state by mot_reference."""
    states = []
    for sq in seqs:
        st = new_state(sq["NG"], sq["NT"])
        for gb, gi, gf, tb, ti in sq["frames"]:
            mot_reference(st, (gb, gi, gf), (tb, ti), thr)
        states.append(st)
    return states


def pack_chunks(seqs, max_frames=MOT_MAX_F):
    """The launches of ``seqs`` (at most MOT_MAX_S of them, slot j for sequence
    j): host arrays per chunk of at most ``max_frames`` frames.  A chunk
    holds the next frames of every sequence that has frames left, the same
    number of each, a sequence's frames in order, so that the launch's
    workgroups -- one per sequence -- all have work."""
    M = max([1, *(len(fr[1]) for sq in seqs for fr in sq["frames"])])
    K = max([1, *(len(fr[4]) for sq in seqs for fr in sq["frames"])])
    done = [0] * len(seqs)
    chunks = []
    while True:
        live = [j for j, sq in enumerate(seqs) if done[j] < len(sq["frames"])]
        if not live:
            return chunks, M, K
        per = max(1, max_frames // len(live))
        picks = [(j, f) for j in live for f in range(done[j], min(done[j] + per, len(seqs[j]["frames"])))]
        F = len(picks)
        c = {"gt_boxes": np.zeros((F, M, 4), np.float32), "gt_idx": np.zeros((F, M), np.int32),
             "gt_flag": np.zeros((F, M), np.int32), "n_gt": np.zeros(F, np.int32),
             "trk_boxes": np.zeros((F, K, 4), np.float32), "trk_idx": np.zeros((F, K), np.int32),
             "n_trk": np.zeros(F, np.int32), "frame_slot": np.zeros(F, np.int32),
             "frame_reset": np.zeros(F, np.int32)}
        for i, (j, f) in enumerate(picks):
            gb, gi, gf, tb, ti = seqs[j]["frames"][f]
            m, k = len(gi), len(ti)
            c["gt_boxes"][i, :m], c["gt_idx"][i, :m], c["gt_flag"][i, :m], c["n_gt"][i] = gb, gi, gf, m
            c["trk_boxes"][i, :k], c["trk_idx"][i, :k], c["n_trk"][i] = tb, ti, k
            c["frame_slot"][i] = j
            done[j] = f + 1
        chunks.append(c)


def run_device(seqs, thr, device) -> list:
    """Every sequence's final state by rtdetr_mot_eval: one launch per chunk
    (pack_chunks), groups of at most MOT_MAX_S sequences."""
    import torch

    from ..moe import _lib

    states = []
    for g0 in range(0, len(seqs), MOT_MAX_S):
        group = seqs[g0:g0 + MOT_MAX_S]
        st = MotEvalState(len(group), max(1, *(sq["NG"] for sq in group)), max(1, *(sq["NT"] for sq in group)),
                          device)
        chunks, _, _ = pack_chunks(group)
        for c in chunks:
            t = {k: torch.from_numpy(v).to(device) for k, v in c.items()}
            _lib.mot_eval(st, t["gt_boxes"], t["gt_idx"], t["gt_flag"], t["n_gt"], t["trk_boxes"], t["trk_idx"],
                          t["n_trk"], t["frame_slot"], t["frame_reset"], thr)
        _lib.mot_eval_check(st)
        for j, sq in enumerate(group):
            full = st.export(j)
            NG, NT = sq["NG"], sq["NT"]
            states.append({"prev_step": full["prev_step"][:NG], "last_ever": full["last_ever"][:NG],
                           "per_gt": full["per_gt"][:NG], "counts": full["counts"], "motp_sum": full["motp_sum"],
                           "pmc": full["pmc"][:NG, :NT], "gt_count": full["gt_count"][:NG],
                           "trk_count": full["trk_count"][:NT]})
    return states


def evaluate(gt, results, thr=0.5, device=None, hota=False) -> dict:
    """Score tracker output against ground truth.  ``gt``: load_gt's dict;
    ``results``: {key: MOT text} as predictor.mot_lines returns it, or a
    directory of <key>.txt files; every key of ``gt`` must have results.  The
    frames of a sequence are 1 .. the last frame either side has a row in.  ->
    {key: mot_metrics' dict, "COMBINED": combine's over the keys in sorted
    order, whatever order gt has them in}.  On a GPU ``device`` (a torch.device or anything torch.device
    takes) all sequences are packed, padded to the largest M and K, and every
    chunk of at most 1024 frames is ONE HIP launch (rtdetr_mot_eval); with
    ``device`` None or the CPU, or MOE_TRACK_EVAL=0, mot_reference runs
    instead and gives the same dict.  ``hota``: every sequence's dict and
    COMBINED gain one key "HOTA" holding hota.hota_metrics' / combine_hota's
    dict (hota.py: the frame-parallel kernels rtdetr_hota_* on a GPU device,
    hota_reference otherwise, the same dict either way)."""
    thr = check_thr(thr)
    keys = list(gt)
    if "COMBINED" in keys:
        raise ValueError('a sequence may not be called "COMBINED"')
    res = load_results(results, keys)
    seqs = [dense_sequence(gt[k], res[k]) for k in keys]
    for k, sq in zip(keys, seqs):
        if len(sq["frames"]) > MOT_MAX_FRAMES:
            raise ValueError(f"sequence {k!r} has more than 2^24 frames")
    dev = None
    if device is not None:
        import torch

        dev = torch.device(device)
    states = run_device(seqs, thr, dev) if eval_on_gpu(dev) and seqs else run_reference(seqs, thr)
    out = {k: mot_metrics(st) for k, st in zip(keys, states)}
    out["COMBINED"] = combine([out[k] for k in sorted(keys)])
    if hota:
        from . import hota as H

        hs = H.run_device_hota(seqs, thr, dev) if eval_on_gpu(dev) and seqs else H.run_reference_hota(seqs, thr)
        for k, st in zip(keys, hs):
            out[k]["HOTA"] = H.hota_metrics(st)
        out["COMBINED"]["HOTA"] = H.combine_hota([out[k]["HOTA"] for k in sorted(keys)])
    return out
