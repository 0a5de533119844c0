"""Shared inputs of the camera-motion tests (motion.shift_reference on the CPU,
rtdetr_frame_shift on the GPU): a block scene to cut shifted views from, the
noise-only frames that the gate is for, and the pan case of the tracker.  Not a
test."""
from __future__ import annotations

import numpy as np

SHIFTS = [(0, 0), (1, 0), (-3, 2), (5, -7), (11, 9), (-12, -12), (13, 3), (-9, 14)]  # found at radius 12 (and 16)
PAN = [0, 40, 40, 40, -35, -35, 30, 30, 0, 0, 45, -45, 40, 40, 40, 40, -30, -30, 20, 20]  # px per frame


def scene(h, w, seed=0, block=8):
    """Random values on ``block`` x ``block`` blocks, fp32 RGB [h, w, 3] in [0, 1]."""
    rng = np.random.default_rng(seed)
    small = rng.random(((h + block - 1) // block, (w + block - 1) // block, 3)).astype(np.float32)
    return np.repeat(np.repeat(small, block, 0), block, 1)[:h, :w]


def view(sc, h, w, ox, oy, seed=None, sigma=0.02, margin=80):
    """The h x w view of ``sc`` whose content stands (ox, oy) further right / down than at offset (0, 0), plus
    independent N(0, sigma) noise (``seed`` None: none)."""
    y, x = margin - oy, margin - ox
    v = sc[y:y + h, x:x + w].copy()
    if seed is not None:
        v = v + np.random.default_rng(seed).normal(0, sigma, v.shape).astype(np.float32)
    return v.astype(np.float32)


def views(h, w, offsets, seed=0, margin=80):
    """One noisy view per cumulative offset -> fp32 [F, h, w, 3]; frame f's content stands offsets[f] from frame
    0's, so the shift of frame f against f - 1 is offsets[f] - offsets[f - 1]."""
    sc = scene(h + 2 * margin, w + 2 * margin, seed)
    return np.stack([view(sc, h, w, ox, oy, seed=1000 * seed + f + 1, margin=margin)
                     for f, (ox, oy) in enumerate(offsets)])


def cumulative(steps):
    """[(dx, dy)] per frame -> the cumulative offsets, frame 0 at its own step."""
    out, x, y = [], 0, 0
    for dx, dy in steps:
        x, y = x + dx, y + dy
        out.append((x, y))
    return out


def noise_frames(h, w, kind, seed=0):
    """Two independent frames without structure: "uniform" noise, or "dark" (0.05 + N(0, 0.02), clipped)."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((2, h, w, 3)).astype(np.float32)
    return np.clip(0.05 + rng.normal(0, 0.02, (2, h, w, 3)), 0, 1).astype(np.float32)


def pan_sequence():
    """draw_sequence(8, 20, 32, seed=1) with the camera pan PAN added to every valid box's x -> (seq, shifts fp32
    [20, 2]: each frame's pan)."""
    from track_cases import draw_sequence

    seq = draw_sequence(8, 20, 32, seed=1)
    cum = np.cumsum(np.asarray(PAN, np.float32))
    for f in range(20):
        n = int(seq["n_valid"][f])
        seq["boxes"][f, :n, 0] += cum[f]
        seq["boxes"][f, :n, 2] += cum[f]
    return seq, np.stack([np.asarray(PAN, np.float32), np.zeros(20, np.float32)], 1)


def run_reference_shift(seq, args, T, shifts, state=None):
    """track_cases.run_reference with a shift per frame (None: none)."""
    from src.rtdetr_moe.track import new_state, track_reference

    F, K = seq["scores"].shape
    state = new_state(T) if state is None else state
    out_id, out_box, count = np.zeros((F, K), np.int32), np.zeros((F, K, 4), np.float32), np.zeros(F, np.int32)
    for f in range(F):
        out_id[f], out_box[f], count[f] = track_reference(state, seq["boxes"][f], seq["scores"][f], seq["labels"][f],
                                                          seq["n_valid"][f], args,
                                                          shift=None if shifts is None else shifts[f])
    return dict(out_id=out_id, out_box=out_box, count=count, state=state)


def draw_frames(root, layout, out_hw, scale=2, seed=11, margin=64):
    """PNG sequences for engine.track: ``layout`` = ((name, [(dx, dy) per frame, in pixels of the model's input]),
    ...).  Every frame is ``scale`` x out_hw and cut from one scene of blocks that are 8 x 8 at the model's input,
    at offsets that are whole input pixels; the scene's values are multiples of 1 / 255, so the PNG holds them."""
    from PIL import Image

    h, w = out_hw[0] * scale, out_hw[1] * scale
    m = margin * scale
    for q, (name, steps) in enumerate(layout):
        sc = np.round(scene(h + 2 * m, w + 2 * m, seed + q, block=8 * scale) * 255).astype(np.uint8)
        (root / name).mkdir()
        for f, (ox, oy) in enumerate(cumulative(steps)):
            y, x = m - oy * scale, m - ox * scale
            Image.fromarray(sc[y:y + h, x:x + w]).save(root / name / f"{f:03d}.png")
