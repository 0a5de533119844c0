"""Inputs shared by the size-report tests (test_size_report_cpu.py,
test_gpu_eval_match_bands.py): the seeded batches of
test_gpu_eval_match.py::test_random_batches with their banded reference codes
(computed once per process), and the constructed ignore-region cases."""
from __future__ import annotations

import functools

import numpy as np

from eval_match_cases import random_image

INF = float("inf")
KM_CASES = [(300, 1), (300, 20), (300, 65), (300, 130), (1, 20), (63, 20), (65, 20)]
BANDS3 = [(0.0, 40.0), (40.0, 80.0), (80.0, INF)]
# eight bands, overlapping: the three above, the whole axis, a band inside another, one that
# straddles two, a narrow one with fractional edges and an open one
BANDS8 = BANDS3 + [(0.0, INF), (50.0, 70.0), (30.0, 60.0), (59.5, 60.25), (110.0, INF)]
SCALES = [1.0, 3848 / 1248, 0.5, 1.0, 2168 / 704, 0.75]  # per image of a batch


def batch(K, M):
    """The six images of test_random_batches(K, M): boxes, scores, labels stacked
    and [(gt, gt_labels)] with truth counts [0, 1, M, M // 2, min(5, M), M]."""
    rng = np.random.default_rng(1000 * K + M)
    imgs = [random_image(rng, K, n) for n in [0, 1, M, M // 2, min(5, M), M]]
    boxes, scores, labels = (np.stack([im[i] for im in imgs]) for i in range(3))
    return boxes, scores, labels, [(im[3], im[4]) for im in imgs]


def reference(boxes, scores, labels, gts, bands, scales=None, iouv=None):
    """uint8 [B, R, K, T]: match_predictions_banded per image."""
    from src.rtdetr_moe.metrics import IOU_THRESHOLDS, match_predictions_banded

    iouv = IOU_THRESHOLDS if iouv is None else iouv
    scales = [1.0] * len(gts) if scales is None else scales
    return np.stack([match_predictions_banded(boxes[b], scores[b], labels[b],
                                              np.asarray(g, np.float64).reshape(-1, 4), np.asarray(gl, np.int64),
                                              bands, scales[b], iouv) for b, (g, gl) in enumerate(gts)])


@functools.lru_cache(maxsize=None)
def seeded(K, M):
    """(batch(K, M), codes uint8 [6, 4, K, 10]) at scale 1 for the bands
    [(0, inf)] + BANDS3 -- read-only, shared by the tests."""
    b = batch(K, M)
    code = reference(*b, [(0.0, INF)] + BANDS3)
    code.setflags(write=False)
    return b, code


def constructed():
    """[(name, boxes f32 [K,4], scores f32 [K], gt f64 [n,4], bands, scale, want)]:
    one class; want[r][k] is the code at IoU 0.5 (None: not stated).  Each case
    is explained where it is built."""
    f32 = lambda rows: np.asarray(rows, np.float32).reshape(-1, 4)  # noqa: E731
    f64 = lambda rows: np.asarray(rows, np.float64).reshape(-1, 4)  # noqa: E731
    desc = lambda k: np.linspace(0.9, 0.1, k).astype(np.float32)  # noqa: E731
    cases = []
    # preference: P has IoU 0.6 on the in-band truth A (height 48) and 0.8 on the out-of-band B
    # (height 100); it takes A (code 1), so Q, sitting on B, still finds B (code 2).  The plain
    # matcher gives B to P and leaves Q a false positive.
    cases.append(("preference", f32([[0, 0, 100, 80], [0, 0, 100, 100]]), desc(2),
                  f64([[0, 0, 100, 48], [0, 0, 100, 100]]), [(0.0, 50.0)], 1.0, [[1, 2]]))
    # consumed ignore region: two in-band predictions (height 49) on one out-of-band truth
    # (height 50 = hi, exclusive): the first is ignored and consumes it, the second is a false positive
    cases.append(("consumed", f32([[0, 0, 100, 49], [0, 1, 100, 50]]), desc(2), f64([[0, 0, 100, 50]]),
                  [(0.0, 50.0)], 1.0, [[2, 0]]))
    # unmatched predictions far from the truth: in-band -> 0, out-of-band -> 2, per band
    cases.append(("unmatched", f32([[300, 300, 320, 330], [400, 300, 420, 360]]), desc(2), f64([[0, 0, 10, 30]]),
                  [(0.0, 50.0), (50.0, INF)], 1.0, [[0, 2], [2, 0]]))
    # edges: heights exactly lo (40: in) and exactly hi (100: out), truths and predictions alike
    cases.append(("edges", f32([[0, 0, 20, 40], [100, 0, 120, 100], [300, 0, 320, 40], [400, 0, 420, 100]]), desc(4),
                  f64([[0, 0, 20, 40], [100, 0, 120, 100]]), [(40.0, 100.0)], 1.0, [[1, 2, 0, 2]]))
    # a scale moves boxes across the edges: 39 px is out at scale 1 and in at scale 2 (78), 60 px in and then out (120)
    boxes = f32([[0, 0, 20, 39], [100, 0, 120, 60], [300, 0, 320, 39], [400, 0, 420, 60]])
    gt = f64([[0, 0, 20, 39], [100, 0, 120, 60]])
    cases.append(("scale 1", boxes, desc(4), gt, [(40.0, 100.0)], 1.0, [[2, 1, 2, 0]]))
    cases.append(("scale 2", boxes, desc(4), gt, [(40.0, 100.0)], 2.0, [[1, 2, 0, 2]]))
    # the prediction height is the float32 difference: 40.0 exactly (in [40, 100)), where the
    # float64 difference of the same coordinates is 39.9999986 (out)
    y1, y2 = float.fromhex("0x1.47fbbp-1"), float.fromhex("0x1.451feep+5")
    cases.append(("fp32 height", f32([[300, y1, 320, y2]]), desc(1), f64([[0, 0, 10, 50]]), [(40.0, 100.0)], 1.0,
                  [[0]]))
    # a truth with negative height is in no band, (0, inf) included; it overlaps nothing
    cases.append(("negative truth", f32([[0, 0, 20, 50], [100, 20, 120, 50]]), desc(2),
                  f64([[0, 0, 20, 50], [100, 50, 120, 20]]), [(0.0, INF)], 1.0, [[1, 0]]))
    return cases
