"""Tiled prediction's two host-side definitions (engine.predict(tiles=...)).

* ``tile_windows``: the overlapping grid of crops of a frame.
* ``merge_reference``: the greedy, score-ordered merge of the detections of a
  frame's passes (full frame + tiles), stated once.  The HIP kernel
  rtdetr_nms_merge (_lib.nms_merge) takes the same decisions bit for bit and is
  tested against this function; it is also the merge of the CPU device and of
  MOE_PREDICT_MERGE=0.

The rule.  Candidate i takes part if i < n_valid and scores[i] >= conf (a NaN
score never does).  The candidates are visited in argsort(-scores, stable)
order: descending score, equal scores by lower index.  A visited candidate is
suppressed if some already kept j has the same label (or ``class_agnostic``)
and inter > thr * den; otherwise it is kept; the walk stops after ``max_det``
kept.  All arithmetic is fp32, every operation rounded on its own, no division:
    area  = max(x2 - x1, 0) * max(y2 - y1, 0)
    iw    = max(min(x2_i, x2_j) - max(x1_i, x1_j), 0), ih likewise
    inter = iw * ih
    den   = (area_i + area_j) - inter    metric "iou"
    den   = min(area_i, area_j)          metric "ios" (intersection over the smaller box)
so a zero-area box never suppresses anything and is never suppressed.
Coordinates must be finite.
"""
from __future__ import annotations

import numpy as np

METRICS = {"iou": 0, "ios": 1}  # the kernel's metric argument
MERGE_MAX_N, MERGE_MAX_DET, MERGE_MAX_B = 4096, 1024, 1024  # rtdetr_nms_merge's limits


def _axis_windows(L: int, n: int, o: float):
    """[(start, length)] of the n tiles of an axis of length L at overlap fraction o."""
    L, n = int(L), int(n)
    if n < 1 or n > L:
        raise ValueError(f"tiles per axis must be in [1, {L}] for an axis of {L} pixels, got {n}")
    if n == 1:
        return [(0, L)]
    t = min(L, int(np.ceil(L / (n - (n - 1) * o))))
    return [((i * (L - t) + (n - 1) // 2) // (n - 1), t) for i in range(n)]


def tile_windows(w: int, h: int, tiles=(2, 2), overlap: float = 0.2):
    """The (rows, cols) grid of windows over a w x h frame, row-major:
    [(x0, y0, tw, th)] in integer pixels.  Per axis of length L with n tiles
    and overlap fraction o in [0, 0.5]: tile length t = min(L, ceil(L / (n -
    (n - 1) o))), start of tile i s_i = (i (L - t) + (n - 1) // 2) // (n - 1)
    (s_0 = 0 for n = 1): the first window starts at 0, the last ends at L and
    neighbours overlap by at least floor(o t) - 1 pixels."""
    rows, cols = (int(v) for v in tiles)
    o = float(overlap)
    if not 0.0 <= o <= 0.5:
        raise ValueError(f"tile overlap must be in [0, 0.5], got {overlap}")
    ys = _axis_windows(h, rows, o)
    xs = _axis_windows(w, cols, o)
    return [(x0, y0, tw, th) for y0, th in ys for x0, tw in xs]


def parse_tiles(tiles):
    """None / "" -> None; "2x3" or (2, 3) -> (rows, cols)."""
    if tiles is None or tiles == "":
        return None
    if isinstance(tiles, str):
        parts = tiles.lower().split("x")
        if len(parts) != 2:
            raise ValueError(f"tiles must be ROWSxCOLS, got {tiles!r}")
        tiles = parts
    rows, cols = (int(v) for v in tiles)
    if rows < 1 or cols < 1:
        raise ValueError(f"tiles must be >= 1 per axis, got {rows}x{cols}")
    return rows, cols


def merge_reference(boxes, scores, labels, n_valid, conf, thr, metric="ios", max_det=300, class_agnostic=False):
    """One image: boxes fp32 [N, 4] xyxy, scores fp32 [N], labels [N] (tensors
    or arrays) -> int64 array of the kept candidate indices, best first (the
    rule in the module's docstring).  ``n_valid`` None means N."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float32)).reshape(-1, 4)
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    N = s.shape[0]
    n = N if n_valid is None else min(max(int(n_valid), 0), N)
    conf32, thr32, zero = np.float32(conf), np.float32(thr), np.float32(0)
    with np.errstate(invalid="ignore"):
        part = (np.arange(N) < n) & (s >= conf32)
    order = np.argsort(-s, kind="stable")
    order = order[part[order]]
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    area = np.maximum(x2 - x1, zero) * np.maximum(y2 - y1, zero)
    max_det = int(max_det)
    kept = np.empty(min(max_det, len(order)), dtype=np.int64)
    nk = 0
    for i in order:
        if nk >= max_det:
            break
        k = kept[:nk]
        iw = np.maximum(np.minimum(x2[i], x2[k]) - np.maximum(x1[i], x1[k]), zero)
        ih = np.maximum(np.minimum(y2[i], y2[k]) - np.maximum(y1[i], y1[k]), zero)
        inter = iw * ih
        den = (area[i] + area[k]) - inter if metric == "iou" else np.minimum(area[i], area[k])
        hit = inter > thr32 * den
        if not class_agnostic:
            hit &= lab[k] == lab[i]
        if not hit.any():
            kept[nk] = i
            nk += 1
    return kept[:nk].copy()
