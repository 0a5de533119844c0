"""Multi-pass prediction's host-side definitions (engine.predict(tiles=..., flip=...)).

* ``tile_windows``: the overlapping grid of crops of a frame.
* ``unmirror_boxes``: the boxes of a mirrored pass back in their window
  (predict / validate with ``flip``).
* ``merge_reference``: the greedy, score-ordered merge of the detections of a
  frame's passes (full frame + tiles), stated once.  The HIP kernel
  rtdetr_nms_merge (_lib.nms_merge) takes the same decisions bit for bit and is
  tested against this function; it is also the merge of the CPU device and of
  MOE_PREDICT_MERGE=0.
* ``fuse_reference``: the same walk, after which every kept box is averaged
  with the copies it suppressed that agree with it (predict(merge="fuse"));
  the HIP kernel rtdetr_box_fuse (_lib.box_fuse) is tested against it.

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
FUSE_MAX_N, FUSE_MAX_DET, FUSE_MAX_B, FUSE_MAX_P = 4096, 1024, 1024, 64  # rtdetr_box_fuse's limits


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


def unmirror_boxes(boxes, width):
    """The boxes of a mirrored pass (predict / validate with ``flip``) back in
    the unmirrored window: boxes fp32 [..., 4] xyxy (a tensor on any device, or
    an array) -> the same kind and shape with x1' = width - x2 and x2' = width
    - x1, y unchanged; fp32, each subtraction rounded on its own.  ``width``:
    the window's width in the boxes' units, a number or anything that
    broadcasts against boxes[..., 0] (one width per slot: [S, 1] for [S, k, 4]
    boxes); it is rounded to fp32 first.  Applied to a mirrored pass's boxes as
    postprocess_batched returns them, ahead of the shift by the window's origin
    and the clip.  On coordinates and widths that fp32 subtracts exactly it is
    its own inverse."""
    import torch

    if isinstance(boxes, torch.Tensor):
        if boxes.dtype != torch.float32:
            raise ValueError(f"unmirror_boxes: boxes must be fp32, got {boxes.dtype}")
        w = torch.as_tensor(width, dtype=torch.float32, device=boxes.device)
        return torch.stack([w - boxes[..., 2], boxes[..., 1], w - boxes[..., 0], boxes[..., 3]], -1)
    b = np.asarray(boxes)
    if b.dtype != np.float32:
        raise ValueError(f"unmirror_boxes: boxes must be fp32, got {b.dtype}")
    w = np.asarray(width, dtype=np.float32)
    return np.stack([w - b[..., 2], b[..., 1], w - b[..., 0], b[..., 3]], -1).astype(np.float32)


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


def fuse_reference(boxes, scores, labels, n_valid, conf, thr, metric="ios", max_det=300, class_agnostic=False,
                   fuse_thr=0.55, windows=None, return_clusters=False):
    """One image: merge_reference's walk, then every kept box (a leader) fused
    with the copies of its object -> (kept int64 [n_kept], identical to
    merge_reference's; fused boxes fp32 [n_kept, 4]; members int32 [n_kept]).
    ``windows`` fp32 [P, 4] (x0, y0, x1, y1) or None: row 0 the frame, rows
    1..P-1 the tile windows; N must be P k, candidate i belongs to pass i // k.

    1. A candidate that was visited and suppressed joins the first leader, in
       kept order, that suppresses it.  Candidates past the max_det-th kept one
       are not visited and join nothing.
    2. It fuses if the two boxes agree on what both passes could see: both
       clamped, coordinate by coordinate, into V, the intersection of the two
       passes' windows (no clamp without ``windows``), then inter > fuse_thr *
       ((area_i + area_j) - inter), always the "iou" form.  The truncated and
       the full copy of one person pass; a child's box inside an adult's, which
       "ios" suppresses, does not: it stays suppressed and is not averaged in.
       The leader always fuses.
    3. Side s of candidate i of pass p > 0 is cut if it lies on an edge of W_p
       that is not an edge of the frame W_0: x1 if x1_i <= W_p.x0 and W_p.x0 >
       W_0.x0, x2 if x2_i >= W_p.x1 and W_p.x1 < W_0.x1, y likewise.
    4. Per leader and side, over the fusing candidates in visit order (leader
       first): one contributes if that side is not cut and its score is finite
       and > 0; num = num + (score * coord), den = den + score in fp32; the
       fused coordinate is num / den if den > 0, else the leader's own; with
       ``windows`` it is clamped into W_0; an axis that comes out unordered
       keeps both of the leader's coordinates.
    Score and label stay the leader's.  fp32, every operation rounded on its
    own, no FMA; the only division is the last one.
    ``return_clusters``: also return rank int64 [N] (the kept rank whose average
    candidate i went into, a leader its own; -1 for every other candidate) and
    the number of visited, suppressed candidates."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    f32 = np.float32
    b = np.ascontiguousarray(np.asarray(boxes, dtype=f32)).reshape(-1, 4)
    s = np.asarray(scores, dtype=f32).reshape(-1)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    N = s.shape[0]
    W, k = None, 0
    if windows is not None:
        W = np.ascontiguousarray(np.asarray(windows, dtype=f32)).reshape(-1, 4)
        P = W.shape[0]
        if P < 1 or P > FUSE_MAX_P or N % P != 0:
            raise ValueError(f"windows must be [P, 4] with 1 <= P <= {FUSE_MAX_P} and N = P k, got P {P}, N {N}")
        k = max(N // P, 1)
    n = N if n_valid is None else min(max(int(n_valid), 0), N)
    conf32, thr32, fthr32, zero = f32(conf), f32(thr), f32(fuse_thr), f32(0)
    with np.errstate(invalid="ignore"):
        part = (np.arange(N) < n) & (s >= conf32)
    order = np.argsort(-s, kind="stable")
    order = order[part[order]]
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    area = np.maximum(x2 - x1, zero) * np.maximum(y2 - y1, zero)
    max_det = int(max_det)
    kept = np.empty(min(max_det, len(order)), dtype=np.int64)
    nk = 0
    joined = []  # (candidate, kept rank of its leader), in visit order
    for i in order:
        if nk >= max_det:
            break
        kk = kept[:nk]
        iw = np.maximum(np.minimum(x2[i], x2[kk]) - np.maximum(x1[i], x1[kk]), zero)
        ih = np.maximum(np.minimum(y2[i], y2[kk]) - np.maximum(y1[i], y1[kk]), zero)
        inter = iw * ih
        den = (area[i] + area[kk]) - inter if metric == "iou" else np.minimum(area[i], area[kk])
        hit = inter > thr32 * den
        if not class_agnostic:
            hit &= lab[kk] == lab[i]
        if hit.any():
            joined.append((int(i), int(np.argmax(hit))))
        else:
            kept[nk] = i
            nk += 1
    kept = kept[:nk].copy()

    def fuses(i, j):
        bi, bj = b[i], b[j]
        if W is not None:
            wi, wj = W[i // k], W[j // k]
            lo = np.maximum(wi[[0, 1, 0, 1]], wj[[0, 1, 0, 1]])
            hi = np.minimum(wi[[2, 3, 2, 3]], wj[[2, 3, 2, 3]])
            bi = np.minimum(np.maximum(bi, lo), hi)
            bj = np.minimum(np.maximum(bj, lo), hi)
        ai = np.maximum(bi[2] - bi[0], zero) * np.maximum(bi[3] - bi[1], zero)
        aj = np.maximum(bj[2] - bj[0], zero) * np.maximum(bj[3] - bj[1], zero)
        iw = np.maximum(np.minimum(bi[2], bj[2]) - np.maximum(bi[0], bj[0]), zero)
        ih = np.maximum(np.minimum(bi[3], bj[3]) - np.maximum(bi[1], bj[1]), zero)
        inter = iw * ih
        return bool(inter > fthr32 * ((ai + aj) - inter))

    def uncut(i):
        """Which of the four sides of candidate i may be averaged."""
        if W is None or i // k == 0:
            return (True, True, True, True)
        w, w0 = W[i // k], W[0]
        return (not (b[i, 0] <= w[0] and w[0] > w0[0]), not (b[i, 1] <= w[1] and w[1] > w0[1]),
                not (b[i, 2] >= w[2] and w[2] < w0[2]), not (b[i, 3] >= w[3] and w[3] < w0[3]))

    num = np.zeros((nk, 4), dtype=f32)
    den = np.zeros((nk, 4), dtype=f32)
    members = np.ones(nk, dtype=np.int32)

    def add(i, q):
        if np.isfinite(s[i]) and s[i] > zero:
            for side, ok in enumerate(uncut(i)):
                if ok:
                    num[q, side] = num[q, side] + (s[i] * b[i, side])
                    den[q, side] = den[q, side] + s[i]

    # visit order with the leader first: a leader precedes every candidate it suppresses
    for q in range(nk):
        add(int(kept[q]), q)
    rank = np.full(N, -1, dtype=np.int64)
    rank[kept] = np.arange(nk)
    for i, q in joined:
        if fuses(i, int(kept[q])):
            members[q] += 1
            rank[i] = q
            add(i, q)
    fused = b[kept].copy() if nk else np.zeros((0, 4), dtype=f32)
    for q in range(nk):
        lead = b[kept[q]]
        out = lead.copy()
        for side in range(4):
            if den[q, side] > zero:
                out[side] = num[q, side] / den[q, side]
        if W is not None:
            out = np.minimum(np.maximum(out, W[0][[0, 1, 0, 1]]), W[0][[2, 3, 2, 3]])
        if out[0] > out[2]:
            out[0], out[2] = lead[0], lead[2]
        if out[1] > out[3]:
            out[1], out[3] = lead[1], lead[3]
        fused[q] = out
    if return_clusters:
        return kept, fused, members, rank, len(joined)
    return kept, fused, members
