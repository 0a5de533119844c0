"""Candidates for the merge tests (tests/test_gpu_nms_merge.py): drawn on the
CPU from a seed, clustered like the detections of a frame's passes -- each
object several times, slightly displaced -- with scores on a 1/64 grid, so that
equal scores are common, and two labels."""
from __future__ import annotations

import numpy as np
import torch

FRAME_W, FRAME_H = 3848.0, 2168.0


def draw(N: int, seed: int, clusters: int | None = None):
    """(boxes fp32 [N, 4] xyxy, scores fp32 [N], labels int32 [N]) of one image:
    ``clusters`` (default max(2, N // 6)) cluster centres, boxes of pedestrian
    aspect ratio (w = 0.4 h, h in [40, 200]) jittered around them by a few
    pixels."""
    rng = np.random.default_rng(seed)
    M = max(2, N // 6) if clusters is None else int(clusters)
    cx = rng.uniform(100, FRAME_W - 100, M)
    cy = rng.uniform(120, FRAME_H - 120, M)
    h = rng.uniform(40, 200, M)
    which = rng.integers(0, M, N)
    jit = rng.normal(0.0, 3.0, (N, 4))
    hh = h[which] * rng.uniform(0.6, 1.0, N)  # some copies truncated, as a tile's box of a person it cuts
    x1 = cx[which] - 0.2 * h[which] + jit[:, 0]
    y1 = cy[which] - 0.5 * h[which] + jit[:, 1]
    x2 = cx[which] + 0.2 * h[which] + jit[:, 2]
    y2 = y1 + hh + jit[:, 3]
    boxes = torch.from_numpy(np.stack([x1, y1, x2, y2], 1).astype(np.float32))
    scores = torch.from_numpy((rng.integers(0, 64, N) / 64.0).astype(np.float32))
    labels = torch.from_numpy(rng.integers(0, 2, N).astype(np.int32))
    return boxes, scores, labels


def draw_batch(B: int, N: int, seed: int, clusters: int | None = None):
    parts = [draw(N, seed * 100 + b, clusters) for b in range(B)]
    return tuple(torch.stack([p[j] for p in parts]) for j in range(3))


def reference_batch(boxes, scores, labels, n_valid, conf, thr, metric, max_det, class_agnostic):
    """merge_reference per image -> (kept index lists, visited-and-suppressed
    counts): a candidate that takes part and stands before the last kept one in
    the visit order (before the end, if the max_det cut was not reached) was
    visited; it was suppressed if it is not kept."""
    from src.rtdetr_moe.merge import merge_reference

    kept, suppressed = [], []
    for b in range(boxes.shape[0]):
        nv = None if n_valid is None else int(n_valid[b])
        k = merge_reference(boxes[b], scores[b], labels[b], nv, conf, thr, metric, max_det, class_agnostic)
        s = scores[b].numpy()
        n = s.shape[0] if nv is None else min(max(nv, 0), s.shape[0])
        with np.errstate(invalid="ignore"):
            part = (np.arange(s.shape[0]) < n) & (s >= np.float32(conf))
        order = np.argsort(-s, kind="stable")
        order = order[part[order]]
        if len(k) >= max_det:  # the walk stopped at the cut
            visited = int(np.nonzero(order == k[-1])[0][0]) + 1
        else:
            visited = len(order)
        kept.append(k.tolist())
        suppressed.append(visited - len(k))
    return kept, suppressed
