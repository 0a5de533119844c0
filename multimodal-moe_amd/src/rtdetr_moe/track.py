"""Tracking by detection (engine.track / engine.predict(track=...)): the rule
that links a sequence's detections from frame to frame, stated once.

* ``TrackArgs``: the tracker's arguments.  The defaults are ByteTrack's where it
  has them (track_high, track_low, new_thr, max_age) and are NOT tuned here:
  this tree has no trained weights and no sequence ground truth (with ground
  truth of your own, engine.track(..., gt=...) scores a run: moteval.py).
* ``track_reference``: one frame of one sequence, plain numpy.  The HIP kernel
  rtdetr_track_update / rtdetr_track_update_shift (_lib.track_update) takes the
  same decisions and computes
  the same boxes bit for bit and is tested against this function; it is also
  the tracker of the CPU device and of MOE_PREDICT_TRACK=0.
* ``TrackState``: the device buffers the kernel keeps its tracks in between
  launches, with an export to (and an import from) the reference's arrays.
* ``SweepState``: the same for G configurations at once (tune.py's parameter
  sweep, rtdetr_track_sweep).

The rule.  A sequence owns T track slots: box (xyxy), vel (one fp32 per side),
score, label, id, age, hits (0: the slot is free), and per sequence next_id
(starts at 1) and dropped.  The candidates are the frame's rows in the order
given (best first, as postprocess_batched and the merges deliver them); nothing
is sorted.  All arithmetic is fp32, every operation rounded on its own, no FMA.
 1. Predict: every live slot, coasting ones included, box = box + vel, per
    coordinate; with a camera shift (sx, sy) of the frame (TrackArgs.cmc:
    motion.py) box = (box + vel) + (sx, sy, sx, sy), each operation rounded on
    its own.  vel is untouched, so the filter learns the residual motion.
    Without a shift nothing is added (adding zero would turn -0.0 into +0.0).
 2. Bands: row d takes part if d < n_valid, its score is finite and score >=
    track_low; it is high if score >= track_high, else low.  Coordinates must
    be finite.
 3. IoU: area = max(x2 - x1, 0) * max(y2 - y1, 0); iw, ih as in merge.py; inter
    = iw * ih; den = (area_t + area_d) - inter; iou = inter / den if den > 0
    else 0 (the one correctly rounded division).  A pair is admissible if the
    labels are equal (or class_agnostic) and iou > thr.
 4. Greedy association of a set of slots with a set of rows: repeatedly match
    the admissible pair of a still-unmatched slot and row with the largest iou
    (equal iou: the lower row, then the lower slot) until none is left.  A
    deliberate simplification of ByteTrack's linear assignment.  This is
    assoc = "greedy", the default; assoc = "lsap" replaces the step (below).
 5. Stage 1: all live slots against the high rows, thr = match_iou.
 6. Stage 2 (BYTE): the slots still unmatched with age == 0 and hits >=
    min_hits against the low rows, thr = second_iou.
 7. A matched slot: r = det - box; box = box + alpha * r; vel = vel + beta * r;
    score the row's; age = 0; hits = min(hits + 1, 2^30).
 8. An unmatched live slot: hits < min_hits frees it; otherwise age += 1 and it
    is freed once age > max_age.  A freed slot is all zeros.
 9. Births, after step 8: every unmatched high row with score >= new_thr, in
    row order, takes the lowest free slot (box the row's, vel 0, hits 1, age 0,
    id = next_id++); without a free slot dropped += 1.
10. Report: out_id[d] is the id of the slot that row d updated or founded if
    that slot now has hits >= min_hits, else -1; out_box[d] is that slot's box
    after the update, else zeros.

Step 4 with assoc = "lsap", for one stage's slots and rows (both in ascending
index order); steps 1-3 and 5-10 are as above.
 4a. Admissible pairs: adm[t, d] as in step 3 (labels equal or class_agnostic,
     fp32 iou > thr); score[t, d] is the fp32 iou where admissible, else 0.
 4b. Pruning (part of the rule): only the slots with at least one admissible
     row and the rows with at least one admissible slot are kept.  If either
     side is then empty the stage matches nothing and no problem is solved.
     This keeps filler rows and false positives out of the problem and bounds
     the solver's work by the real candidates, not by K.
 4c. Solve scipy.optimize.linear_sum_assignment on cost = -(float64) score of
     the pruned sets, in moteval._assign's orientation: the side with more
     members is the matrix's rows (equal sizes: the slots).  The costs lie in
     [-1, 0] and are finite: a NaN iou is simply inadmissible.
 4d. A returned pair is a match if and only if it is admissible.
It maximises the total IoU over the one-to-one admissible matchings.  It is NOT
ByteTrack's lapjv with cost_limit: that prices leaving a pair unmatched and can
prefer fewer matches; here a match is never traded away for a price.  Events:
"ties" is a greedy notion and is not counted; solves (problems solved),
solve_n_max (the largest smaller side) and solve_q_max (the largest larger side)
are added instead (LSAP_EVENTS), under "lsap" only.
"""
from __future__ import annotations

from dataclasses import asdict, dataclass, fields

import numpy as np

TRACK_MAX_K, TRACK_MAX_T, TRACK_MAX_F, TRACK_MAX_S = 1024, 256, 1024, 1024  # rtdetr_track_update's limits
TRACK_MAX_G = 1024  # rtdetr_track_sweep: configurations per launch
HITS_CAP = 1 << 30
STATE_FIELDS = ("box", "vel", "score", "label", "id", "age", "hits")
EVENTS = ("stage1", "stage2", "refound", "tentative_freed", "expired", "births", "dropped", "ties", "reported")
LSAP_EVENTS = ("solves", "solve_n_max", "solve_q_max")  # added to the events under assoc = "lsap" only
ASSOC = ("greedy", "lsap")  # TrackArgs.assoc; the index is the kernel's ``assoc`` argument


@dataclass
class TrackArgs:
    track_high: float = 0.5     # high-score band starts here
    track_low: float = 0.1      # low-score band starts here
    new_thr: float = 0.6        # minimum score to start a track
    match_iou: float = 0.2      # stage 1: IoU must exceed this
    second_iou: float = 0.5     # stage 2: IoU must exceed this
    max_age: int = 30           # frames a confirmed track may coast unmatched
    min_hits: int = 2           # hits needed before a track is reported
    alpha: float = 0.5          # filter gain on the box
    beta: float = 0.25          # filter gain on the velocity
    class_agnostic: bool = False  # ignore labels when matching
    max_tracks: int = 64        # track slots T per sequence, at most 256
    # camera-motion compensation (motion.py): the tracks' predicted boxes move by the frame's global shift
    cmc: bool = False
    cmc_radius: int = 48        # search radius in pixels of the model's input, a multiple of 4 in [4, 64]; not tuned
    cmc_gate: float = 0.1       # a non-zero shift must beat SAD(0, 0) by this share; not tuned
    cmc_rows: tuple = (0.0, 1.0)  # the (top, bottom) fractions of the height the estimator looks at
    assoc: str = "greedy"       # step 4: "greedy", or "lsap" (the assignment with the largest total IoU)

    def __post_init__(self):
        from .motion import check_rows, check_search

        if not isinstance(self.assoc, str) or self.assoc not in ASSOC:
            raise ValueError(f'TrackArgs.assoc must be "greedy" or "lsap", got {self.assoc!r}')
        if not isinstance(self.cmc, (bool, np.bool_)):
            raise ValueError(f"TrackArgs.cmc must be a bool, got {self.cmc!r}")
        self.cmc = bool(self.cmc)
        try:
            self.cmc_radius, _ = check_search(self.cmc_radius, self.cmc_gate)
            self.cmc_gate = float(self.cmc_gate)
            self.cmc_rows = check_rows(self.cmc_rows)
        except ValueError as e:
            raise ValueError(f"TrackArgs.cmc_*: {e}") from None
        for name in ("track_high", "track_low", "new_thr", "match_iou", "second_iou", "alpha", "beta"):
            v = float(getattr(self, name))
            if v != v:
                raise ValueError(f"TrackArgs.{name} must not be NaN")
            setattr(self, name, v)
        self.max_age, self.min_hits, self.max_tracks = int(self.max_age), int(self.min_hits), int(self.max_tracks)
        self.class_agnostic = bool(self.class_agnostic)
        if not 0 <= self.max_age <= HITS_CAP:
            raise ValueError(f"TrackArgs.max_age must be in [0, 2^30], got {self.max_age}")
        if not 1 <= self.min_hits <= HITS_CAP:
            raise ValueError(f"TrackArgs.min_hits must be in [1, 2^30], got {self.min_hits}")
        if not 1 <= self.max_tracks <= TRACK_MAX_T:
            raise ValueError(f"TrackArgs.max_tracks must be in [1, {TRACK_MAX_T}], got {self.max_tracks}")

    @classmethod
    def parse(cls, v) -> "TrackArgs":
        """A TrackArgs, a dict of its fields, or True (the defaults)."""
        if isinstance(v, cls):
            return v
        if v is True:
            return cls()
        if isinstance(v, dict):
            unknown = set(v) - {f.name for f in fields(cls)}
            if unknown:
                raise ValueError(f"unknown tracker arguments {sorted(unknown)}")
            return cls(**v)
        raise ValueError(f"track must be a TrackArgs or a dict of its fields, got {type(v).__name__}")

    def as_dict(self) -> dict:
        return asdict(self)


def new_state(T: int) -> dict:
    """An empty sequence state of T slots (the rule's named arrays)."""
    T = int(T)
    return {"box": np.zeros((T, 4), np.float32), "vel": np.zeros((T, 4), np.float32),
            "score": np.zeros(T, np.float32), "label": np.zeros(T, np.int32), "id": np.zeros(T, np.int32),
            "age": np.zeros(T, np.int32), "hits": np.zeros(T, np.int32), "next_id": 1, "dropped": 0}


def copy_state(state: dict) -> dict:
    return {k: (v.copy() if isinstance(v, np.ndarray) else int(v)) for k, v in state.items()}


def states_equal(a: dict, b: dict) -> bool:
    """Bit for bit: the fp32 arrays compared as int32."""
    if int(a["next_id"]) != int(b["next_id"]) or int(a["dropped"]) != int(b["dropped"]):
        return False
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.int32), np.ascontiguousarray(b[k]).view(np.int32))
               for k in STATE_FIELDS)


def _iou(tb, db):
    """tb [n, 4] against db [m, 4] -> fp32 [n, m], the rule's step 3."""
    zero = np.float32(0)
    ta = np.maximum(tb[:, 2] - tb[:, 0], zero) * np.maximum(tb[:, 3] - tb[:, 1], zero)
    da = np.maximum(db[:, 2] - db[:, 0], zero) * np.maximum(db[:, 3] - db[:, 1], zero)
    iw = np.maximum(np.minimum(tb[:, None, 2], db[None, :, 2]) - np.maximum(tb[:, None, 0], db[None, :, 0]), zero)
    ih = np.maximum(np.minimum(tb[:, None, 3], db[None, :, 3]) - np.maximum(tb[:, None, 1], db[None, :, 1]), zero)
    inter = iw * ih
    den = (ta[:, None] + da[None, :]) - inter
    ok = den > zero
    return np.where(ok, inter / np.where(ok, den, np.float32(1)), zero).astype(np.float32)


def _associate(slots, rows, box, label, b, lab, thr, agnostic, events):
    """The greedy step 4 over the given slot and row indices -> [(slot, row)] in the order matched."""
    if len(slots) == 0 or len(rows) == 0:
        return []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        iou = _iou(box[slots], b[rows])
        adm = iou > np.float32(thr)
    if not agnostic:
        adm &= label[slots][:, None] == lab[rows][None, :]
    out = []
    while adm.any():
        best = iou[adm].max()
        ts, ds = np.nonzero(adm & (iou == best))
        if events is not None and len(ts) > 1:
            events["ties"] += 1
        j = np.lexsort((ts, ds))[0]  # the lower row, then the lower slot (both index lists ascend)
        t, d = int(ts[j]), int(ds[j])
        out.append((int(slots[t]), int(rows[d])))
        adm[t, :] = False
        adm[:, d] = False
    return out


def _associate_lsap(slots, rows, box, label, b, lab, thr, agnostic, events):
    """Step 4 with assoc = "lsap" (4a-4d) over the given slot and row indices -> [(slot, row)]."""
    if len(slots) == 0 or len(rows) == 0:
        return []
    from scipy.optimize import linear_sum_assignment

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        iou = _iou(box[slots], b[rows])
        adm = iou > np.float32(thr)
    if not agnostic:
        adm &= label[slots][:, None] == lab[rows][None, :]
    ks, kr = np.nonzero(adm.any(1))[0], np.nonzero(adm.any(0))[0]
    if len(ks) == 0:
        return []
    adm = adm[np.ix_(ks, kr)]
    score = np.where(adm, iou[np.ix_(ks, kr)], np.float32(0)).astype(np.float32)
    cost = -score.astype(np.float64)
    if len(ks) >= len(kr):  # the larger side is the matrix's rows; equal: the slots
        ts, ds = linear_sum_assignment(cost)
    else:
        ds, ts = linear_sum_assignment(np.ascontiguousarray(cost.T))
    if events is not None:
        events["solves"] += 1
        events["solve_n_max"] = max(events["solve_n_max"], min(len(ks), len(kr)))
        events["solve_q_max"] = max(events["solve_q_max"], max(len(ks), len(kr)))
        if "solve_shapes" in events:  # a list the caller put there: every problem's (slots, rows)
            events["solve_shapes"].append((len(ks), len(kr)))
    return [(int(slots[ks[t]]), int(rows[kr[d]])) for t, d in zip(ts, ds) if adm[t, d]]


def track_reference(state, boxes, scores, labels, n_valid, args, events=None, shift=None):
    """One frame of one sequence: boxes fp32 [K, 4] xyxy, scores fp32 [K], labels
    [K] (tensors or arrays), ``n_valid`` None (= K) or the number of leading
    rows that count.  Updates ``state`` (new_state) in place -> (out_id int32
    [K], out_box fp32 [K, 4], count: the reported rows).  ``events``: a dict the
    frame's event counts (EVENTS; with assoc = "lsap" LSAP_EVENTS too) are added to.  ``shift``: the frame's camera
    shift (sx, sy) in the boxes' pixels, or None: nothing is added."""
    a = TrackArgs.parse(args)
    f32 = np.float32
    b = np.ascontiguousarray(np.asarray(boxes, dtype=f32)).reshape(-1, 4)
    s = np.asarray(scores, dtype=f32).reshape(-1)
    lab = np.asarray(labels).reshape(-1).astype(np.int32)
    K = s.shape[0]
    n = K if n_valid is None else min(max(int(n_valid), 0), K)
    box, vel, hits, age = state["box"], state["vel"], state["hits"], state["age"]
    T = hits.shape[0]
    if events is not None:
        for k in EVENTS + (LSAP_EVENTS if a.assoc == "lsap" else ()):
            events.setdefault(k, 0)
    associate = _associate_lsap if a.assoc == "lsap" else _associate
    # 1. predict
    live = hits > 0
    box[live] = box[live] + vel[live]
    if shift is not None:
        sx, sy = f32(shift[0]), f32(shift[1])
        box[live] = box[live] + np.array([sx, sy, sx, sy], dtype=f32)
    # 2. bands
    with np.errstate(invalid="ignore"):
        part = (np.arange(K) < n) & np.isfinite(s) & (s >= f32(a.track_low))
        high = part & (s >= f32(a.track_high))
    low = part & ~high
    # 5. stage 1, 6. stage 2
    row_slot = np.full(K, -1, dtype=np.int64)
    slot_row = np.full(T, -1, dtype=np.int64)
    m1 = associate(np.nonzero(live)[0], np.nonzero(high)[0], box, state["label"], b, lab, a.match_iou,
                    a.class_agnostic, events)
    for t, d in m1:
        slot_row[t], row_slot[d] = d, t
    second = live & (slot_row < 0) & (age == 0) & (hits >= a.min_hits)
    m2 = associate(np.nonzero(second)[0], np.nonzero(low)[0], box, state["label"], b, lab, a.second_iou,
                    a.class_agnostic, events)
    for t, d in m2:
        slot_row[t], row_slot[d] = d, t
    if events is not None:
        events["stage1"] += len(m1)
        events["stage2"] += len(m2)
    # 7. update, 8. unmatched
    alpha, beta = f32(a.alpha), f32(a.beta)
    for t in np.nonzero(live)[0]:
        d = slot_row[t]
        if d >= 0:
            if events is not None and age[t] > 0:
                events["refound"] += 1
            r = b[d] - box[t]
            box[t] = box[t] + alpha * r
            vel[t] = vel[t] + beta * r
            state["score"][t] = s[d]
            age[t] = 0
            hits[t] = min(int(hits[t]) + 1, HITS_CAP)
            continue
        if hits[t] < a.min_hits:
            free, what = True, "tentative_freed"
        else:
            age[t] += 1
            free, what = age[t] > a.max_age, "expired"
        if free:
            for k in STATE_FIELDS:
                state[k][t] = 0
            if events is not None:
                events[what] += 1
    # 9. births
    with np.errstate(invalid="ignore"):
        born = high & (row_slot < 0) & (s >= f32(a.new_thr))
    free_slots = np.nonzero(hits == 0)[0]
    for j, d in enumerate(np.nonzero(born)[0]):
        if j >= len(free_slots):
            state["dropped"] = int(state["dropped"]) + 1
            if events is not None:
                events["dropped"] += 1
            continue
        t = free_slots[j]
        box[t], vel[t] = b[d], 0
        state["score"][t], state["label"][t] = s[d], lab[d]
        state["id"][t] = state["next_id"]
        state["next_id"] = int(state["next_id"]) + 1
        age[t], hits[t] = 0, 1
        row_slot[d] = t
        if events is not None:
            events["births"] += 1
    # 10. report
    out_id = np.full(K, -1, dtype=np.int32)
    out_box = np.zeros((K, 4), dtype=f32)
    rep = row_slot >= 0
    rep[rep] = hits[row_slot[rep]] >= a.min_hits
    out_id[rep] = state["id"][row_slot[rep]]
    out_box[rep] = box[row_slot[rep]]
    count = int(rep.sum())
    if events is not None:
        events["reported"] += count
    return out_id, out_box, count


class TrackState:
    """S sequences' track slots on the device, between launches of
    rtdetr_track_update (the layout include/moe_hip.h documents):
      box   fp32  [S, T, 8]  x1 y1 x2 y2, then the four sides' velocities
      score fp32  [S, T]
      meta  int32 [S, T, 4]  label, id, age, hits (0: free)
      seq   int32 [S, 2]     next_id, dropped
    """

    def __init__(self, S: int, T: int, device):
        import torch

        self.S, self.T = int(S), int(T)
        if not 1 <= self.S <= TRACK_MAX_S or not 1 <= self.T <= TRACK_MAX_T:
            raise ValueError(f"TrackState: need 1 <= S <= {TRACK_MAX_S} and 1 <= T <= {TRACK_MAX_T}")
        self.box = torch.zeros((self.S, self.T, 8), dtype=torch.float32, device=device)
        self.score = torch.zeros((self.S, self.T), dtype=torch.float32, device=device)
        self.meta = torch.zeros((self.S, self.T, 4), dtype=torch.int32, device=device)
        self.seq = torch.zeros((self.S, 2), dtype=torch.int32, device=device)
        self.seq[:, 0] = 1

    def tensors(self):
        return self.box, self.score, self.meta, self.seq

    def snapshot(self):
        """Copies of the four buffers (restore() puts them back)."""
        return tuple(t.clone() for t in self.tensors())

    def restore(self, snap):
        for t, s in zip(self.tensors(), snap):
            t.copy_(s)

    def export(self, s: int) -> dict:
        """Slot s as the reference's named arrays (new_state's layout)."""
        box, score, meta, seq = (t[s].cpu().numpy() for t in self.tensors())
        return {"box": box[:, :4].copy(), "vel": box[:, 4:].copy(), "score": score.copy(),
                "label": meta[:, 0].copy(), "id": meta[:, 1].copy(), "age": meta[:, 2].copy(),
                "hits": meta[:, 3].copy(), "next_id": int(seq[0]), "dropped": int(seq[1])}

    def load(self, s: int, state: dict):
        """Slot s from the reference's named arrays."""
        import torch

        box = np.concatenate([state["box"], state["vel"]], 1).astype(np.float32)
        meta = np.stack([state["label"], state["id"], state["age"], state["hits"]], 1).astype(np.int32)
        self.box[s].copy_(torch.from_numpy(box))
        self.score[s].copy_(torch.from_numpy(np.asarray(state["score"], np.float32)))
        self.meta[s].copy_(torch.from_numpy(meta))
        self.seq[s].copy_(torch.tensor([int(state["next_id"]), int(state["dropped"])], dtype=torch.int32))


class SweepState(TrackState):
    """G configurations' TrackStates in one set of buffers, between launches of
    rtdetr_track_sweep (tune.py): TrackState's layout per (g, s),
      box fp32 [G, S, T, 8]   score fp32 [G, S, T]   meta int32 [G, S, T, 4]   seq int32 [G, S, 2]
    """

    def __init__(self, G: int, S: int, T: int, device):
        import torch

        self.G, self.S, self.T = int(G), int(S), int(T)
        if not 1 <= self.G <= TRACK_MAX_G or not 1 <= self.S <= TRACK_MAX_S or not 1 <= self.T <= TRACK_MAX_T:
            raise ValueError(f"SweepState: need 1 <= G <= {TRACK_MAX_G}, 1 <= S <= {TRACK_MAX_S} and "
                             f"1 <= T <= {TRACK_MAX_T}")
        G, S, T = self.G, self.S, self.T
        self.box = torch.zeros((G, S, T, 8), dtype=torch.float32, device=device)
        self.score = torch.zeros((G, S, T), dtype=torch.float32, device=device)
        self.meta = torch.zeros((G, S, T, 4), dtype=torch.int32, device=device)
        self.seq = torch.zeros((G, S, 2), dtype=torch.int32, device=device)
        self.seq[..., 0] = 1

    def _slot(self, g: int, s: int) -> TrackState:
        """Configuration g's slots as a TrackState over the same memory."""
        view = TrackState.__new__(TrackState)
        view.S, view.T = self.S, self.T
        view.box, view.score, view.meta, view.seq = (t[g] for t in self.tensors())
        return view

    def export(self, g: int, s: int) -> dict:
        """Slot s of configuration g as the reference's named arrays."""
        return self._slot(g, s).export(s)

    def export_all(self) -> list:
        """[g][s] -> the reference's named arrays, with one copy per buffer."""
        box, score, meta, seq = (t.cpu().numpy() for t in self.tensors())
        return [[{"box": box[g, s, :, :4].copy(), "vel": box[g, s, :, 4:].copy(), "score": score[g, s].copy(),
                  "label": meta[g, s, :, 0].copy(), "id": meta[g, s, :, 1].copy(), "age": meta[g, s, :, 2].copy(),
                  "hits": meta[g, s, :, 3].copy(), "next_id": int(seq[g, s, 0]), "dropped": int(seq[g, s, 1])}
                 for s in range(self.S)] for g in range(self.G)]

    def load(self, g: int, s: int, state: dict):
        """Slot s of configuration g from the reference's named arrays."""
        self._slot(g, s).load(s, state)
