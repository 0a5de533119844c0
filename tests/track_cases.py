"""Shared inputs of the tracker's tests (track.track_reference on the CPU,
rtdetr_track_update on the GPU): a generator of synthetic pedestrian sequences,
hand-made cases, and a runner that steps the reference over a sequence and
returns its outputs, its final state and its event counts.  Not a test."""
from __future__ import annotations

import numpy as np

W, H = 1248, 704


def draw_sequence(n_obj, n_frames, K, seed=0, jitter=0.0, miss=0.0, low_share=0.0, fp=0, gaps=None, n_labels=1,
                  leave=None):
    """Constant-velocity pedestrians as a detector would report them.
    -> dict(boxes fp32 [F, K, 4], scores fp32 [F, K], labels int32 [F, K],
    n_valid int32 [F], truth int64 [F, K]: the object of each row, -1 for a
    false positive or a filler row).
    Object i starts on a grid (110 px apart, two rows), 30..50 px wide, 80..120
    high, |vx| <= 0.8, |vy| <= 0.3 px per frame.  Per frame and visible object:
    box + N(0, jitter) per side; with probability ``miss`` no row; with
    probability ``low_share`` a score in [0.15, 0.45], else in [0.65, 0.95].
    ``fp`` false positives per frame: random boxes, scores in [0.1, 0.9].
    ``gaps`` {object: (first, last + 1)}: frames without that object; ``leave``
    {object: frame}: gone from that frame on.  The rows are ordered best first
    and cut at K; the rest are fillers with scores below 0.05 (n_valid counts
    the rows with score >= 0.1, a prefix)."""
    rng = np.random.default_rng(seed)
    gaps, leave = gaps or {}, leave or {}
    i = np.arange(n_obj)
    w, h = rng.uniform(30, 50, n_obj), rng.uniform(80, 120, n_obj)
    x0, y0 = 40.0 + (i % 10) * 110.0, 60.0 + (i // 10) * 260.0
    vx, vy = rng.uniform(-0.8, 0.8, n_obj), rng.uniform(-0.3, 0.3, n_obj)
    lab = rng.integers(0, n_labels, n_obj)
    out = dict(boxes=np.zeros((n_frames, K, 4), np.float32), scores=np.zeros((n_frames, K), np.float32),
               labels=np.zeros((n_frames, K), np.int32), n_valid=np.zeros(n_frames, np.int32),
               truth=np.full((n_frames, K), -1, np.int64))
    for f in range(n_frames):
        rows = []
        for o in range(n_obj):
            g = gaps.get(o)
            if (g and g[0] <= f < g[1]) or (o in leave and f >= leave[o]):
                continue
            if f > 0 and rng.random() < miss:
                continue
            low = f > 1 and rng.random() < low_share
            s = rng.uniform(0.15, 0.45) if low else rng.uniform(0.65, 0.95)
            x, y = x0[o] + vx[o] * f, y0[o] + vy[o] * f
            b = np.array([x, y, x + w[o], y + h[o]]) + (rng.normal(0, jitter, 4) if jitter else 0.0)
            rows.append((s, b, lab[o], o))
        for _ in range(fp):
            x, y, ww = rng.uniform(0, W - 60), rng.uniform(0, H - 130), rng.uniform(25, 55)
            rows.append((rng.uniform(0.1, 0.9), np.array([x, y, x + ww, y + 2.4 * ww]), rng.integers(0, n_labels), -1))
        rows.sort(key=lambda r: -r[0])
        rows = rows[:K]
        n = len(rows)
        for d, (s, b, c, o) in enumerate(rows):
            out["boxes"][f, d], out["scores"][f, d], out["labels"][f, d], out["truth"][f, d] = b, s, c, o
        m = K - n  # fillers: what a detector's remaining queries look like
        fx, fy = rng.uniform(0, W - 60, m), rng.uniform(0, H - 130, m)
        out["boxes"][f, n:] = np.stack([fx, fy, fx + 40, fy + 100], 1)
        out["scores"][f, n:] = np.sort(rng.uniform(0.001, 0.05, m))[::-1]
        out["n_valid"][f] = n
    return out


def run_reference(seq, args, T, n_valid="given", state=None, chunks=None):
    """Step track_reference over seq's frames (``chunks``: lists of frame
    indices, stepped one after the other -- the result cannot depend on it).
    ``n_valid``: "given" (seq's), None, or an int array [F].
    -> dict(out_id int32 [F, K], out_box fp32 [F, K, 4], count int32 [F],
    state, events)."""
    from src.rtdetr_moe.track import new_state, track_reference

    F, K = seq["scores"].shape
    nv = seq["n_valid"] if isinstance(n_valid, str) else n_valid
    state = new_state(T) if state is None else state
    events = {}
    out_id = np.zeros((F, K), np.int32)
    out_box = np.zeros((F, K, 4), np.float32)
    count = np.zeros(F, np.int32)
    for chunk in (chunks or [range(F)]):
        for f in chunk:
            out_id[f], out_box[f], count[f] = track_reference(state, seq["boxes"][f], seq["scores"][f],
                                                              seq["labels"][f], None if nv is None else nv[f], args,
                                                              events)
    return dict(out_id=out_id, out_box=out_box, count=count, state=state, events=events)


def identities(seq, out_id):
    """{object: the ids its reported rows got, in frame order} and the number of
    switches: reported rows of one object whose id differs from the object's
    previous reported id."""
    ids, switches = {}, 0
    F, K = out_id.shape
    for f in range(F):
        for d in range(K):
            o, t = int(seq["truth"][f, d]), int(out_id[f, d])
            if o < 0 or t < 0:
                continue
            seen = ids.setdefault(o, [])
            if seen and seen[-1] != t:
                switches += 1
            if not seen or seen[-1] != t:
                seen.append(t)
    return ids, switches


def _frames(rows_per_frame, K):
    """[(box, score, label)] per frame -> a seq dict padded to K rows with zeros (n_valid the given rows)."""
    F = len(rows_per_frame)
    seq = dict(boxes=np.zeros((F, K, 4), np.float32), scores=np.zeros((F, K), np.float32),
               labels=np.zeros((F, K), np.int32), n_valid=np.zeros(F, np.int32), truth=np.full((F, K), -1, np.int64))
    for f, rows in enumerate(rows_per_frame):
        for d, (b, s, c) in enumerate(rows):
            seq["boxes"][f, d], seq["scores"][f, d], seq["labels"][f, d] = b, s, c
        seq["n_valid"][f] = len(rows)
    return seq


A = (100.0, 50.0, 140.0, 150.0)
B = (300.0, 50.0, 340.0, 150.0)


def hand_cases():
    """[dict(name, seq, args, T, ids: the expected out_id rows of every frame (the given rows only))]."""
    nan, inf = float("nan"), float("inf")
    return [
        # two rows identical to one track: the lower row takes it, the other founds a track
        dict(name="two_rows_one_track", T=4, args=dict(min_hits=1), ties=1,
             seq=_frames([[(A, 0.9, 0)], [(A, 0.9, 0), (A, 0.8, 0)]], 4), ids=[[1], [1, 2]]),
        # two tracks identical to one row: the lower slot takes it; the other, tentative, is freed
        dict(name="two_tracks_one_row", T=4, args=dict(min_hits=2), ties=1,
             seq=_frames([[(A, 0.9, 0), (A, 0.8, 0)], [(A, 0.9, 0)], [(A, 0.9, 0)]], 4), ids=[[-1, -1], [1], [1]]),
        # the same with confirmed tracks: slot 1 coasts and takes the second row one frame later
        dict(name="two_tracks_one_row_confirmed", T=4, args=dict(min_hits=1), ties=1,
             seq=_frames([[(A, 0.9, 0), (A, 0.8, 0)], [(A, 0.9, 0)], [(A, 0.9, 0), (A, 0.7, 0)]], 4),
             ids=[[1, 2], [1], [1, 2]]),
        # labels separate what overlaps; class_agnostic joins it
        dict(name="labels_separate", T=4, args=dict(min_hits=1), ties=0,
             seq=_frames([[(A, 0.9, 0)], [(A, 0.9, 1)]], 4), ids=[[1], [2]]),
        dict(name="class_agnostic_joins", T=4, args=dict(min_hits=1, class_agnostic=True), ties=0,
             seq=_frames([[(A, 0.9, 0)], [(A, 0.9, 1)]], 4), ids=[[1], [1]]),
        # NaN, -inf and +inf scores never take part; a low row founds nothing
        dict(name="bad_scores", T=4, args=dict(min_hits=1, track_low=-inf), ties=0,
             seq=_frames([[(A, nan, 0), (B, -inf, 0), (A, inf, 0), (B, 0.9, 0), (A, 0.3, 0)]], 8),
             ids=[[-1, -1, -1, 1, -1]]),
        # a low row keeps a confirmed track alive (stage 2) and a second identical low row changes nothing
        dict(name="stage_two", T=4, args=dict(min_hits=2), ties=1,
             seq=_frames([[(A, 0.9, 0)], [(A, 0.9, 0)], [(A, 0.3, 0), (A, 0.3, 0)], [(A, 0.9, 0)]], 4),
             ids=[[-1], [1], [1, -1], [1]]),
        # no free slot: the birth is dropped
        dict(name="dropped", T=1, args=dict(min_hits=1), ties=0, dropped=2,
             seq=_frames([[(A, 0.9, 0), (B, 0.8, 0)], [(A, 0.9, 0), (B, 0.8, 0)]], 4), ids=[[1, -1], [1, -1]]),
    ]


def check_hand_case(case, res):
    """res: run_reference's (or the kernel's) out_id against the case's expected ids."""
    for f, want in enumerate(case["ids"]):
        got = res["out_id"][f].tolist()
        assert got[:len(want)] == want and all(v == -1 for v in got[len(want):]), (case["name"], f, got, want)
