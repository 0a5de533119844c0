"""Shared inputs of the tracking evaluator's tests (moteval.mot_reference on
the CPU, rtdetr_mot_eval on the GPU): a generator of random frames with dense
indices, a generator of tracked pedestrians that also emits the clean truth
boxes, builders for hand-made sequences and MOTChallenge text, and a runner
that steps the reference.  Not a test."""
from __future__ import annotations

import numpy as np

A = (100.0, 50.0, 140.0, 150.0)
B = (300.0, 50.0, 340.0, 150.0)
C = (500.0, 50.0, 540.0, 150.0)


def shifted(box, dx):
    """``box`` moved right by dx: IoU with the original is (40 - dx) / (40 + dx) for the 40-wide boxes above."""
    return (box[0] + dx, box[1], box[2] + dx, box[3])


def frame(gt_rows, trk_rows):
    """[(g, box, flag)], [(t, box)] -> mot_reference's (gt boxes, g, flags, trk boxes, t)."""
    gb = np.asarray([r[1] for r in gt_rows], np.float32).reshape(-1, 4)
    tb = np.asarray([r[1] for r in trk_rows], np.float32).reshape(-1, 4)
    return (gb, np.asarray([r[0] for r in gt_rows], np.int32), np.asarray([r[2] for r in gt_rows], np.int32),
            tb, np.asarray([r[0] for r in trk_rows], np.int32))


def run_reference(frames, NG, NT, thr=0.5, state=None, chunks=None):
    """Step mot_reference over ``frames`` (``chunks``: lists of frame indices stepped one after the other) -> state."""
    from src.rtdetr_moe.moteval import mot_reference, new_state

    state = new_state(NG, NT) if state is None else state
    for chunk in (chunks or [range(len(frames))]):
        for f in chunk:
            gb, gi, gf, tb, ti = frames[f]
            mot_reference(state, (gb, gi, gf), (tb, ti), thr)
    return state


def metrics_of(frames, NG, NT, thr=0.5):
    from src.rtdetr_moe.moteval import mot_metrics

    return mot_metrics(run_reference(frames, NG, NT, thr))


def draw_frames(seed, F, NG, NT, m, k, ignore=0.0, tie=0.0, jitter=3.0, drift=0.1):
    """F random frames for NG ground-truth and NT tracker indices.  Objects of
    30..50 x 80..120 px move at constant velocity in a field sized so that
    neighbours overlap now and then.  Tracker index t follows object t (t >= NG:
    nothing, a random box per frame); per frame, with probability ``drift``, two
    tracker indices swap what they follow (identity switches).  A frame shows
    ``m`` = (lo, hi) random ground-truth indices and ``k`` = (lo, hi) random
    tracker indices, each side in random row order.  A shown ground-truth row
    is an ignore region with probability ``ignore``.  A tracker row's box is
    its object's plus N(0, jitter) per side, or, with probability ``tie``, an
    exact copy of it -- and a tracker row that follows nothing copies a shown
    ground-truth box exactly with probability ``tie`` (identical boxes: exact
    IoU ties).  -> [(gt boxes fp32, g int32, flags int32, trk boxes fp32, t int32)]."""
    rng = np.random.default_rng(seed)
    side = 70.0 * np.sqrt(max(NG, NT)) + 100.0
    pos = rng.uniform(0, side, (NG, 2))
    vel = rng.uniform(-2, 2, (NG, 2))
    wh = np.stack([rng.uniform(30, 50, NG), rng.uniform(80, 120, NG)], 1)
    follows = np.where(np.arange(NT) < NG, np.arange(NT), -1)
    frames = []
    for f in range(F):
        if NT > 1 and rng.random() < drift:
            a, b = rng.choice(NT, 2, replace=False)
            follows[a], follows[b] = follows[b], follows[a]
        xy = pos + vel * f
        box = np.concatenate([xy, xy + wh], 1)
        nm = int(rng.integers(m[0], min(m[1], NG) + 1))
        nk = int(rng.integers(k[0], min(k[1], NT) + 1))
        gi = rng.permutation(NG)[:nm]
        ti = rng.permutation(NT)[:nk]
        gb = box[gi].astype(np.float32)
        gf = (rng.random(nm) >= ignore).astype(np.int32)
        tb = np.zeros((nk, 4), np.float32)
        for r, t in enumerate(ti):
            o = follows[t]
            if o >= 0:
                tb[r] = box[o] + (0.0 if rng.random() < tie else rng.normal(0, jitter, 4))
            elif nm and rng.random() < tie:
                tb[r] = gb[rng.integers(nm)]
            else:
                x, y = rng.uniform(0, side, 2)
                tb[r] = (x, y, x + 40, y + 100)
        frames.append((gb, gi.astype(np.int32), gf, tb.astype(np.float32), ti.astype(np.int32)))
    return frames


def draw_tracked(n_obj, n_frames, seed=0, jitter=1.5, jumps=None):
    """Pedestrians on a grid, far enough apart never to overlap, with the clean
    truth boxes AND a detector's rows of them: no false positives, no misses.
    ``jumps`` {object: frame}: from that frame on the object stands 55 px further
    right (its track is lost and a new one founded: an identity switch).  ->
    (seq: tests/track_cases.py's dict with ``truth`` = the object of each row, K
    = n_obj; truth_boxes fp32 [F, n_obj, 4])."""
    rng = np.random.default_rng(seed)
    jumps = jumps or {}
    i = np.arange(n_obj)
    w, h = rng.uniform(30, 50, n_obj), rng.uniform(80, 120, n_obj)
    x0, y0 = 40.0 + (i % 8) * 150.0, 60.0 + (i // 8) * 260.0
    vx, vy = rng.uniform(-0.5, 0.5, n_obj), rng.uniform(-0.3, 0.3, n_obj)
    K = n_obj
    seq = dict(boxes=np.zeros((n_frames, K, 4), np.float32), scores=np.zeros((n_frames, K), np.float32),
               labels=np.zeros((n_frames, K), np.int32), n_valid=np.full(n_frames, K, np.int32),
               truth=np.full((n_frames, K), -1, np.int64))
    truth_boxes = np.zeros((n_frames, n_obj, 4), np.float32)
    for f in range(n_frames):
        s = rng.uniform(0.65, 0.95, n_obj)
        order = np.argsort(-s)
        for o in range(n_obj):
            x = x0[o] + vx[o] * f + (55.0 if o in jumps and f >= jumps[o] else 0.0)
            y = y0[o] + vy[o] * f
            truth_boxes[f, o] = (x, y, x + w[o], y + h[o])
        for d, o in enumerate(order):
            seq["boxes"][f, d] = truth_boxes[f, o] + rng.normal(0, jitter, 4)
            seq["scores"][f, d], seq["truth"][f, d] = s[o], o
    return seq, truth_boxes


def mot_text(rows) -> str:
    """[(frame, id, x1, y1, x2, y2, *rest)] -> MOTChallenge text (x, y, w, h; ``rest`` appended as given)."""
    out = []
    for fr, i, x1, y1, x2, y2, *rest in rows:
        out.append(",".join(str(v) for v in (fr, i, x1, y1, x2 - x1, y2 - y1, *rest)))
    return "".join(line + "\n" for line in out)
