"""Shared inputs of the tests of TrackArgs.assoc = "lsap" (track.track_reference
on the CPU, rtdetr_track_update_assoc / rtdetr_track_sweep_assoc on the GPU): a
crowd generator (neighbours that overlap above match_iou and cross), hand cases
with the tracks set directly, a runner, and the drawn shapes of the GPU tests
with the preconditions that keep the comparison from passing on nothing.  Not a
test."""
from __future__ import annotations

import numpy as np

from track_cases import W, H, _frames, draw_sequence, hand_cases

_CACHE = {}


def draw_crowd(n_obj, n_frames, K, seed=0, spacing=18.0, speed=3.0, jitter=1.5, miss=0.1, low_share=0.2, fp=2, dup=0,
               n_labels=1):
    """draw_sequence's dict for a crowd: object i stands at x = 30 + spacing * (i % per_row), 40 px wide and 100 high
    (spacing < width: neighbours overlap, IoU about 0.38 at 18 px), in rows 120 px apart, and walks at +-speed px a
    frame, the sign alternating with i, so that neighbours cross.  ``miss``, ``low_share``, ``jitter`` and ``fp`` as
    draw_sequence's; ``dup``: the first ``dup`` rows of a frame appear a second time with the same box and a score
    0.001 lower (a tile's copy: exact cost ties for the solver).  Rows best first, cut at K, fillers after."""
    rng = np.random.default_rng(seed)
    per_row = int((W - 100) // spacing)
    i = np.arange(n_obj)
    x0, y0 = 30.0 + spacing * (i % per_row), 20.0 + 120.0 * (i // per_row)
    vx = np.where(i % 2 == 0, speed, -speed) * rng.uniform(0.6, 1.0, n_obj)
    lab = rng.integers(0, n_labels, n_obj)
    out = dict(boxes=np.zeros((n_frames, K, 4), np.float32), scores=np.zeros((n_frames, K), np.float32),
               labels=np.zeros((n_frames, K), np.int32), n_valid=np.zeros(n_frames, np.int32),
               truth=np.full((n_frames, K), -1, np.int64))
    for f in range(n_frames):
        rows = []
        for o in range(n_obj):
            if f > 0 and rng.random() < miss:
                continue
            low = f > 1 and rng.random() < low_share
            s = rng.uniform(0.15, 0.45) if low else rng.uniform(0.65, 0.95)
            x = x0[o] + vx[o] * f
            b = np.array([x, y0[o], x + 40.0, y0[o] + 100.0]) + (rng.normal(0, jitter, 4) if jitter else 0.0)
            rows.append((s, b, lab[o], o))
        for _ in range(fp):
            x, y = rng.uniform(0, W - 60), rng.uniform(0, H - 130)
            rows.append((rng.uniform(0.1, 0.9), np.array([x, y, x + 40.0, y + 100.0]), rng.integers(0, n_labels), -1))
        rows.sort(key=lambda r: -r[0])
        rows += [(s - 0.001, b.copy(), c, o) for s, b, c, o in rows[:dup]]
        rows.sort(key=lambda r: -r[0])
        rows = rows[:K]
        n = len(rows)
        for d, (s, b, c, o) in enumerate(rows):
            out["boxes"][f, d], out["scores"][f, d], out["labels"][f, d], out["truth"][f, d] = b, s, c, o
        m = K - n
        fx, fy = rng.uniform(0, W - 60, m), rng.uniform(0, H - 130, m)
        out["boxes"][f, n:] = np.stack([fx, fy, fx + 40, fy + 100], 1)
        out["scores"][f, n:] = np.sort(rng.uniform(0.001, 0.05, m))[::-1]
        out["n_valid"][f] = n
    return out


def run(seq, args, T, n_valid="given", state=None, frames=None, shift=None):
    """track_cases.run_reference with the frames' camera shifts (``shift`` fp32 [F, 2] or None) and, under lsap, every
    solve's (slots, rows) in events["solve_shapes"]."""
    from src.rtdetr_moe.track import TrackArgs, new_state, track_reference

    args = TrackArgs.parse(args)
    F, K = seq["scores"].shape
    nv = seq["n_valid"] if isinstance(n_valid, str) else n_valid
    state = new_state(T) if state is None else state
    events = {"solve_shapes": []} if args.assoc == "lsap" else {}
    out_id = np.zeros((F, K), np.int32)
    out_box = np.zeros((F, K, 4), np.float32)
    count = np.zeros(F, np.int32)
    for f in (range(F) if frames is None else frames):
        out_id[f], out_box[f], count[f] = track_reference(state, seq["boxes"][f], seq["scores"][f], seq["labels"][f],
                                                          None if nv is None else nv[f], args, events,
                                                          shift=None if shift is None else shift[f])
    return dict(out_id=out_id, out_box=out_box, count=count, state=state, events=events)


def n_valid_mode(seq, mode):
    """tests/test_gpu_track.py's n_valid modes."""
    if mode == "null":
        return None
    if mode == "zero":
        return np.zeros_like(seq["n_valid"])
    nv = seq["n_valid"].copy()
    if mode == "partial":
        nv[1::3] = nv[1::3] * 3 // 4  # every third frame loses its weakest quarter
        nv[2::7] = 10 ** 6            # clamped to K
        nv[5::11] = -4                # clamped to 0
    return nv


# (K, T, F, objects, n_valid mode, seed, dup, crowd): K on both sides of a wave and at the limit (1024 with T = 256
# needs more than 64 KiB of LDS); T = 1, 4, one wave, 65 (two waves, one thread in the second), 256 (four waves: the
# idle waves' barriers); F = 1, 2, 16.  ``crowd``: draw_crowd and the crowd preconditions; else draw_sequence.  Seeds
# tuned on the CPU reference for the preconditions (check_preconditions, check_coverage).
SHAPES = [
    (1, 1, 16, 1, "null", 0, 0, False),
    (5, 4, 16, 8, "given", 1, 0, False),
    (65, 64, 1, 20, "given", 5, 0, False),
    (1024, 1, 2, 3, "null", 10, 0, False),
    (300, 4, 16, 8, "partial", 8, 0, False),
    (300, 256, 2, 120, "null", 7, 0, True),
    (63, 64, 16, 30, "given", 2, 0, True),
    (65, 65, 16, 40, "partial", 4, 6, True),
    (65, 64, 16, 40, "zero", 5, 0, True),
    (300, 64, 16, 50, "given", 6, 8, True),
    (300, 256, 16, 120, "given", 3, 0, True),
    (1024, 256, 16, 150, "given", 9, 10, True),
]


def shape_args(T, **kw):
    from src.rtdetr_moe.track import TrackArgs

    return TrackArgs(**{"max_age": 3, "max_tracks": T, "assoc": "lsap", **kw})


def drawn(shape):
    """-> dict(seq, nv, args, ref: run() under lsap, greedy: run() under greedy).  Cached: read-only."""
    if shape not in _CACHE:
        K, T, F, objects, mode, seed, dup, crowd = shape
        if crowd:
            seq = draw_crowd(objects, F, K, seed=seed, dup=dup)
        else:
            seq = draw_sequence(objects, F, K, seed=seed, jitter=2.0, miss=0.12, low_share=0.2,
                                fp=min(3, max(K // 8, 0)))
        nv = n_valid_mode(seq, mode)
        args = shape_args(T)
        _CACHE[shape] = dict(seq=seq, nv=nv, args=args, ref=run(seq, args, T, n_valid=nv),
                             greedy=run(seq, shape_args(T, assoc="greedy"), T, n_valid=nv))
    return _CACHE[shape]


def check_preconditions(shape):
    """Asserted on the reference before the GPU is touched."""
    K, T, F, objects, mode, seed, dup, crowd = shape
    c = drawn(shape)
    e = c["ref"]["events"]
    print(shape, {k: v for k, v in e.items() if k != "solve_shapes"})
    if mode == "zero":
        assert e["reported"] == 0 and e["births"] == 0 and e["solves"] == 0
        return
    assert e["births"] >= 1
    if F >= 2:
        assert e["solves"] >= 1
    if crowd and F >= 16:
        assert e["solves"] >= 1 and e["solve_n_max"] >= 8 and e["stage2"] >= 1
        differs = [f for f in range(F) if not np.array_equal(c["ref"]["out_id"][f], c["greedy"]["out_id"][f])]
        assert differs, "the lsap reference equals the greedy one: the test would pass on the old rule"
    if T == 4:
        assert e["dropped"] >= 1


def check_coverage():
    """Across SHAPES: a solve of each orientation, and one whose smaller side crosses a wave."""
    shapes = [sr for s in SHAPES for sr in drawn(s)["ref"]["events"].get("solve_shapes", [])]
    assert any(ns > nr for ns, nr in shapes) and any(ns < nr for ns, nr in shapes)
    assert any(ns == nr for ns, nr in shapes)
    big = drawn((300, 256, 16, 120, "given", 3, 0, True))["ref"]["events"]
    assert big["solve_n_max"] >= 65


# ---------------------------------------------------------------------------
# hand cases: the tracks set directly
# ---------------------------------------------------------------------------
def _bx(x, y=50.0, w=40.0, h=100.0):
    return (float(x), float(y), float(x + w), float(y + h))


def state_of(T, tracks):
    """new_state(T) with slot t holding tracks[t] = (box, label) as a confirmed track (hits 2, age 0, vel 0, id t + 1)."""
    from src.rtdetr_moe.track import new_state

    st = new_state(T)
    for t, (box, label) in enumerate(tracks):
        st["box"][t], st["label"][t], st["id"][t], st["hits"][t], st["score"][t] = box, label, t + 1, 2, 0.9
    st["next_id"] = len(tracks) + 1
    return st


def lsap_hand_cases():
    """[dict(name, T, args, tracks: state_of's list, seq: one frame, ids: the expected out_id under lsap, greedy: under
    greedy, solves: the (slots, rows) of the solves)], worked out by hand:
    * two_people: the issue's example.  IoU A-108 0.667, B-108 0.538, A-80 0.333, B-80 0: greedy takes A-108 and row 80
      founds id 3; the largest total is A-80 + B-108.
    * labels_separate: the same boxes, but row 80 has another label: A-80 is inadmissible, A takes 108 (0.667 against
      B's 0.538), row 80 founds id 3 -- the greedy answer, by the solver.
    * stage_two: the same pairs in the low band: stage 1 has no rows, stage 2 solves (second_iou 0.3).
    * negative_thr: thr < 0 makes the zero-IoU pair B-80 admissible too; the answer stays A-80 + B-108, and a far row
      (IoU 0 with both) is kept by the pruning: 2 slots x 3 rows, the rows the larger side.
    * more_slots: a third track C at 140, whose only pair is C-108 at 0.111 (match_iou 0.1 keeps it): 3 slots x 2
      rows, the slots the larger side; the answer is still A-80 + B-108 and C coasts.
    * equal_three: tracks at 100, 120, 140 against rows at 128, 108, 88.  IoU by offset: 8 px 0.667, 12 px 0.538, 20 px
      0.333, 28 px 0.176 (inadmissible).  C-128 + B-108 + A-88 (three times 0.538 = 1.615) beats B-128 + A-108 (1.333),
      which is what greedy takes before it strands C."""
    m1 = dict(min_hits=1)
    two = [(_bx(100), 0), (_bx(120), 0)]
    cases = [
        dict(name="two_people", T=4, args=m1, tracks=two, seq=_frames([[(_bx(108), 0.9, 0), (_bx(80), 0.8, 0)]], 4),
             ids=[2, 1], greedy=[1, 3], solves=[(2, 2)]),
        dict(name="labels_separate", T=4, args=m1, tracks=two,
             seq=_frames([[(_bx(108), 0.9, 0), (_bx(80), 0.8, 1)]], 4), ids=[1, 3], greedy=[1, 3], solves=[(2, 1)]),
        dict(name="stage_two", T=4, args=dict(min_hits=1, second_iou=0.3), tracks=two,
             seq=_frames([[(_bx(108), 0.4, 0), (_bx(80), 0.3, 0)]], 4), ids=[2, 1], greedy=[1, -1], solves=[(2, 2)]),
        dict(name="negative_thr", T=4, args=dict(min_hits=1, match_iou=-1.0), tracks=two,
             seq=_frames([[(_bx(108), 0.9, 0), (_bx(80), 0.8, 0), (_bx(600), 0.7, 0)]], 4), ids=[2, 1, 3],
             greedy=[1, 2, 3], solves=[(2, 3)]),
        dict(name="more_slots", T=4, args=dict(min_hits=1, match_iou=0.1), tracks=two + [(_bx(140), 0)],
             seq=_frames([[(_bx(108), 0.9, 0), (_bx(80), 0.8, 0)]], 4), ids=[2, 1], greedy=[1, 4], solves=[(3, 2)]),
        dict(name="equal_three", T=4, args=m1, tracks=two + [(_bx(140), 0)],
             seq=_frames([[(_bx(128), 0.9, 0), (_bx(108), 0.8, 0), (_bx(88), 0.7, 0)]], 4), ids=[3, 2, 1],
             greedy=[2, 1, 4], solves=[(3, 3)]),
    ]
    return cases


def tie_cases():
    """track_cases.hand_cases()'s tie cases (and the rest), to be run under lsap: the expected ids are the same, because
    in each a tie's two candidates are interchangeable up to the row or slot order the solver keeps (checked on the
    CPU against the reference, not assumed)."""
    return hand_cases()
