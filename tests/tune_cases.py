"""Shared inputs of the tracker sweep's tests (tune.py on the CPU,
rtdetr_track_sweep on the GPU): a noisy detector's rows of one synthetic
sequence, the clean ground truth of the same objects, and the 16-configuration
grid.  Not a test."""
from __future__ import annotations

import numpy as np

from track_cases import draw_sequence

KEY = "seq"
GRID16 = {"match_iou": [0.2, 0.8], "max_age": [0, 3], "min_hits": [1, 2], "track_high": [0.5, 0.7]}
# (K, T, seed): the shapes the reference was checked at, and what its least-reporting configuration still reports
SHAPES = [(65, 64, 2), (300, 256, 6), (40, 8, 3), (5, 4, 1)]
MIN_REPORTED = {(65, 64, 2): 215, (300, 256, 6): 230, (40, 8, 3): 113}

_CACHE = {}


def case(K, seed, F=24):
    """-> dict(seq: draw_sequence's noisy rows, dets: {KEY: {frame: (boxes, scores, labels)}} with all K rows of
    every frame (the fillers score below every track_low used), gt: {KEY: {frame: (boxes, ids, flags)}}, the clean
    boxes of the same objects, id = object + 1).  Cached: treat it as read-only."""
    if (K, seed, F) in _CACHE:
        return _CACHE[(K, seed, F)]
    seq = draw_sequence(20, F, K, seed, jitter=2.0, miss=0.12, low_share=0.2, fp=min(3, K // 8), leave={0: 12})
    clean = draw_sequence(20, F, max(K, 20), seed, leave={0: 12})
    dets = {KEY: {f + 1: (seq["boxes"][f].copy(), seq["scores"][f].copy(), seq["labels"][f].copy())
                  for f in range(F)}}
    gt = {KEY: {}}
    for f in range(F):
        rows = np.nonzero(clean["truth"][f] >= 0)[0]
        gt[KEY][f + 1] = (clean["boxes"][f][rows].copy(), clean["truth"][f][rows] + 1,
                          np.ones(len(rows), np.int32))
    _CACHE[(K, seed, F)] = dict(seq=seq, dets=dets, gt=gt)
    return _CACHE[(K, seed, F)]


_REFS = {}


def reference(K, T, seed, grid=None, shifts=None, tag=None):
    """track_sweep_reference of case(K, seed) under the grid (GRID16), computed once per (K, T, seed, tag) -> (configs,
    per configuration the KEY's dict).  Read-only."""
    from src.rtdetr_moe import tune
    from src.rtdetr_moe.track import TrackArgs

    name = (K, T, seed, tag)
    if name not in _REFS:
        configs = tune.expand_grid(grid or GRID16, TrackArgs(max_tracks=T))
        ref = tune.track_sweep_reference(case(K, seed)["dets"], configs, T,
                                         shifts=None if shifts is None else {KEY: shifts})
        _REFS[name] = (configs, [r[KEY] for r in ref])
    return _REFS[name]


def reports_equal(a, b) -> bool:
    """Two (configuration, sequence) results bit for bit: the compact report and the state."""
    from src.rtdetr_moe.track import states_equal

    return (np.array_equal(a["count"], b["count"]) and np.array_equal(a["ids"], b["ids"])
            and np.array_equal(a["rows"], b["rows"])
            and np.array_equal(np.ascontiguousarray(a["boxes"]).view(np.int32),
                               np.ascontiguousarray(b["boxes"]).view(np.int32))
            and states_equal(a["state"], b["state"]))


def check_distinct(K, T, seed, ref):
    """The conditions that stop a kernel which ignores its configuration from passing, asserted on the reference."""
    distinct = sum(1 for i in range(len(ref)) if not any(reports_equal(ref[i], ref[j]) for j in range(i)))
    if (K, T, seed) in MIN_REPORTED:
        assert distinct == len(ref), distinct
        assert min(int(r["count"].sum()) for r in ref) >= MIN_REPORTED[(K, T, seed)]
    else:
        assert distinct >= 2, distinct
    return distinct
