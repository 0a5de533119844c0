"""Inputs shared by the validation-matching tests (test_gpu_eval_match*.py,
test_eval_match_host.py): seeded detection batches and the float64-area
variant of the reference IoU."""
from __future__ import annotations

import numpy as np


def random_image(rng, K, n, classes=3, size=640.0):
    """(boxes f32 [K,4], scores f32 [K], labels i64 [K], gt f64 [n,4], gt_labels i64 [n]):
    jittered copies of the truths (IoUs spread over 0.5..0.95, several per
    truth so they compete, some with a wrong label) and pure noise boxes, all
    with fractional coordinates."""
    xy = rng.uniform(0, size - 130, (n, 2))
    wh = rng.uniform(15, 120, (n, 2))
    gt = np.concatenate([xy, xy + wh], 1).astype(np.float64)
    gl = rng.integers(0, classes, n).astype(np.int64)
    boxes = np.empty((K, 4), np.float64)
    labels = rng.integers(0, classes, K).astype(np.int64)
    for k in range(K):
        if n and rng.random() < 0.6:
            j = int(rng.integers(n))
            w, h = gt[j, 2] - gt[j, 0], gt[j, 3] - gt[j, 1]
            boxes[k] = gt[j] + rng.uniform(-0.08, 0.08, 4) * np.array([w, h, w, h])
            if rng.random() < 0.85:
                labels[k] = gl[j]
        else:
            p = rng.uniform(0, size - 130, 2)
            boxes[k] = np.concatenate([p, p + rng.uniform(5, 120, 2)])
    scores = rng.random(K).astype(np.float32)
    return boxes.astype(np.float32), scores, labels, gt, gl


def to_targets(gts, W, H):
    """Per-image (gt xyxy pixels f64, labels) -> the loader's target dicts
    (normalised cxcywh float32 boxes, int64 labels, CPU tensors)."""
    import torch

    out = []
    for g, gl in gts:
        g = np.asarray(g, np.float64).reshape(-1, 4)
        c = np.stack([(g[:, 0] + g[:, 2]) / 2 / W, (g[:, 1] + g[:, 3]) / 2 / H,
                      (g[:, 2] - g[:, 0]) / W, (g[:, 3] - g[:, 1]) / H], 1).astype(np.float32)
        out.append({"boxes": torch.from_numpy(c).reshape(-1, 4), "labels": torch.as_tensor(gl, dtype=torch.int64)})
    return out


def box_iou_f64_area(a, b):
    """metrics.box_iou_np with the prediction area in float64 (NOT what the
    reference computes on float32 predictions)."""
    lt = np.maximum(a[:, None, :2], b[None, :, :2])
    rb = np.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = np.clip(rb - lt, 0, None)
    inter = wh[..., 0] * wh[..., 1]
    a64 = a.astype(np.float64)
    area_a = np.prod(np.clip(a64[:, 2:] - a64[:, :2], 0, None), 1)
    area_b = np.prod(np.clip(b[:, 2:] - b[:, :2], 0, None), 1)
    return inter / np.maximum(area_a[:, None] + area_b[None] - inter, 1e-9)
