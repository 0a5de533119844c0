"""Candidates for the box-fusion tests (tests/test_box_fuse_cpu.py,
tests/test_gpu_box_fuse.py), drawn on the CPU from a seed, per pass and not from
one pool: pedestrian-shaped objects on a 3848 x 2168 frame, one jittered copy in
every pass (the full frame, then the tiles of merge.tile_windows) whose window
sees at least 4 px of the object, each copy clipped to its window, scores on the
1/64 grid and two labels; and the hand-made cases both files run."""
from __future__ import annotations

import numpy as np
import torch

FRAME_W, FRAME_H = 3848, 2168
GRIDS = {5: (2, 2), 4: (1, 3), 3: (2, 1), 1: (1, 1)}  # passes -> the tile grid (rows, cols)
SIGMA_FRAME, SIGMA_TILE = 0.06, 0.02       # jitter of a copy's sides, as a fraction of the object's height


def windows_of(P: int, w: int = FRAME_W, h: int = FRAME_H) -> np.ndarray:
    """fp32 [P, 4] (x0, y0, x1, y1): the frame, then the tiles' windows."""
    from src.rtdetr_moe.merge import tile_windows

    rows = [(0, 0, w, h)]
    if P > 1:
        rows += [(x0, y0, x0 + tw, y0 + th) for x0, y0, tw, th in tile_windows(w, h, GRIDS[P], 0.2)]
    return np.asarray(rows, dtype=np.float32)


def draw(P: int, k: int, seed: int, objects: int | None = None):
    """One image: (boxes fp32 [P k, 4], scores fp32 [P k], labels int32 [P k],
    windows fp32 [P, 4], truth fp32 [objects, 4], obj int64 [P k]: the object a
    candidate copies, -1 for a filler).  ``objects`` (default about 0.8 k, at
    least 1): a fifth of them stand on a tile edge, so that tiles cut them; one
    in eight is a child inside the previous object's box.  A pass holds its
    copies (the first k) and then fillers: small low-score boxes in its window."""
    rng = np.random.default_rng(seed)
    W = windows_of(P)
    M = max(1, (4 * k) // 5) if objects is None else int(objects)
    h = rng.uniform(40.0, 300.0, M)
    cx = rng.uniform(60.0, FRAME_W - 60.0, M)
    cy = rng.uniform(160.0, FRAME_H - 160.0, M)
    edges_x = sorted({float(v) for v in W[1:, [0, 2]].reshape(-1)} - {0.0, float(FRAME_W)})
    edges_y = sorted({float(v) for v in W[1:, [1, 3]].reshape(-1)} - {0.0, float(FRAME_H)})
    for m in range(0, M, 5):  # on a tile's inner edge
        if edges_x and m % 2 == 0:
            cx[m] = edges_x[(m // 10) % len(edges_x)] + rng.uniform(-0.1, 0.1) * h[m]
        elif edges_y:
            cy[m] = edges_y[(m // 10) % len(edges_y)] + rng.uniform(-0.3, 0.3) * h[m]
    truth = np.stack([cx - 0.2 * h, cy - 0.5 * h, cx + 0.2 * h, cy + 0.5 * h], 1)
    for m in range(7, M, 8):  # a child in front of the adult m - 1: inside its box, a third of its height
        x1, y1, x2, y2 = truth[m - 1]
        hh = (y2 - y1) / 3.0
        truth[m] = [x1 + 0.1 * (x2 - x1), y2 - hh, x1 + 0.1 * (x2 - x1) + 0.4 * hh, y2]
    truth[:, [0, 2]] = truth[:, [0, 2]].clip(0, FRAME_W)
    truth[:, [1, 3]] = truth[:, [1, 3]].clip(0, FRAME_H)
    label = rng.integers(0, 2, M)
    boxes = np.zeros((P, k, 4))
    scores = np.zeros((P, k))
    labels = np.zeros((P, k), dtype=np.int32)
    obj = np.full((P, k), -1, dtype=np.int64)
    for p in range(P):
        x0, y0, x1, y1 = (float(v) for v in W[p])
        sigma = SIGMA_FRAME if p == 0 else SIGMA_TILE
        n = 0
        for m in range(M):
            t = truth[m]
            if min(t[2], x1) - max(t[0], x0) < 4.0 or min(t[3], y1) - max(t[1], y0) < 4.0 or n >= k:
                continue
            c = t + rng.normal(0.0, sigma * (t[3] - t[1]), 4)
            boxes[p, n] = [min(max(c[0], x0), x1), min(max(c[1], y0), y1), min(max(c[2], x0), x1),
                           min(max(c[3], y0), y1)]
            scores[p, n] = rng.integers(16, 64) / 64.0
            labels[p, n] = label[m] if rng.uniform() < 0.9 else 1 - label[m]
            obj[p, n] = m
            n += 1
        for j in range(n, k):  # fillers
            fx, fy = rng.uniform(x0, x1 - 30.0), rng.uniform(y0, y1 - 60.0)
            boxes[p, j] = [fx, fy, fx + rng.uniform(8.0, 30.0), fy + rng.uniform(20.0, 60.0)]
            scores[p, j] = rng.integers(0, 24) / 64.0
            labels[p, j] = rng.integers(0, 2)
    return (torch.from_numpy(boxes.reshape(P * k, 4).astype(np.float32)),
            torch.from_numpy(scores.reshape(-1).astype(np.float32)), torch.from_numpy(labels.reshape(-1)),
            torch.from_numpy(W), torch.from_numpy(truth.astype(np.float32)), torch.from_numpy(obj.reshape(-1)))


def draw_batch(B: int, P: int, k: int, seed: int, objects: int | None = None):
    """(boxes [B, N, 4], scores [B, N], labels [B, N], windows [B, P, 4])."""
    parts = [draw(P, k, seed * 100 + b, objects) for b in range(B)]
    return tuple(torch.stack([p[j] for p in parts]) for j in range(4))


def cut_sides(boxes: np.ndarray, windows: np.ndarray | None) -> np.ndarray:
    """bool [N, 4]: the sides the rule calls cut (fuse_reference's step 3, restated on arrays)."""
    N = boxes.shape[0]
    cut = np.zeros((N, 4), dtype=bool)
    if windows is None:
        return cut
    P = windows.shape[0]
    k = max(N // P, 1)
    w = windows[np.arange(N) // k]
    w0 = windows[0]
    tile = (np.arange(N) // k > 0)
    cut[:, 0] = tile & (boxes[:, 0] <= w[:, 0]) & (w[:, 0] > w0[0])
    cut[:, 1] = tile & (boxes[:, 1] <= w[:, 1]) & (w[:, 1] > w0[1])
    cut[:, 2] = tile & (boxes[:, 2] >= w[:, 2]) & (w[:, 2] < w0[2])
    cut[:, 3] = tile & (boxes[:, 3] >= w[:, 3]) & (w[:, 3] < w0[3])
    return cut


def reference_batch(boxes, scores, labels, windows, n_valid, conf, thr, metric, max_det, class_agnostic, fuse_thr):
    """fuse_reference per image -> a list of dicts: kept (list), fused fp32
    [n, 4], members int32 [n], rank int64 [N], and the counts ``clusters``
    (leaders with at least 2 fusing members), ``unfused`` (visited, suppressed,
    not fused), ``cut`` (cut sides of fusing candidates with a positive score:
    left out of an average) and ``repaired`` (leaders with a cut side whose
    fused coordinate on that side differs from their own)."""
    from src.rtdetr_moe.merge import fuse_reference

    out = []
    for b in range(boxes.shape[0]):
        nv = None if n_valid is None else int(n_valid[b])
        W = None if windows is None else windows[b].numpy()
        kept, fused, members, rank, suppressed = fuse_reference(
            boxes[b], scores[b], labels[b], nv, conf, thr, metric, max_det, class_agnostic, fuse_thr, W,
            return_clusters=True)
        bx, sc = boxes[b].numpy(), scores[b].numpy()
        cut = cut_sides(bx, W)
        fusing = rank >= 0
        lead_cut = cut[kept] if len(kept) else np.zeros((0, 4), dtype=bool)
        out.append(dict(kept=kept.tolist(), fused=torch.from_numpy(fused).reshape(-1, 4),
                        members=torch.from_numpy(members), rank=rank,
                        clusters=int((members >= 2).sum()),
                        unfused=int(suppressed - (int(members.sum()) - len(kept))),
                        cut=int((cut[fusing] & (sc[fusing] > 0)[:, None]).sum()),
                        repaired=int((lead_cut & (fused != bx[kept])).any(1).sum()) if len(kept) else 0))
    return out


# ---------------------------------------------------------------------------
# hand-made cases: (name, boxes, scores, labels, windows or None, options, expected kept, fused boxes, members)
# every expected number is worked out in the comment above its case
# ---------------------------------------------------------------------------
def hand_cases():
    cases = []
    frame = [0, 0, 400, 100]
    # two equal-score copies average: x1 = (0.5 * 0 + 0.5 * 2) / 1 = 1, x2 = (5 + 6) / 1 = 11
    cases.append(dict(name="equal scores average", boxes=[[0, 0, 10, 20], [2, 0, 12, 20]], scores=[0.5, 0.5],
                      labels=[0, 0], windows=None, opts={}, kept=[0], fused=[[1, 0, 11, 20]], members=[2]))
    # three passes of one candidate each: the frame, tile 1 = x in [0, 223], tile 2 = x in [180, 400].
    # the leader (frame, 0.75) and tile 1's copy (0.25) whose x2 = 223 lies on tile 1's inner edge: x2 is cut and
    # stays the leader's 240 ((0.75 * 240) / 0.75); x1 = (0.75 * 200 + 0.25 * 204) / 1 = 201; y1 = (0.75 * 10 +
    # 0.25 * 14) / 1 = 11; y2 = 90.  The fuse test clamps both into V = tile 1: 23 x 80 against 19 x 76 inside
    # it, IoU = 1444 / 1840 = 0.78.  Tile 2's candidate is far away and is kept on its own.
    cases.append(dict(name="cut side left out", boxes=[[200, 10, 240, 90], [204, 14, 223, 90], [300, 0, 310, 20]],
                      scores=[0.75, 0.25, 0.125], labels=[0, 0, 0],
                      windows=[frame, [0, 0, 223, 100], [180, 0, 400, 100]], opts={}, kept=[0, 2],
                      fused=[[201, 11, 240, 90], [300, 0, 310, 20]], members=[2, 1]))
    # the truncated copy wins (0.75 against the frame's 0.25): x2 = 223 is cut, so x2 comes from the frame's copy
    # alone, (0.25 * 240) / 0.25 = 240: repaired; x1 = (0.75 * 200 + 0.25 * 200) / 1 = 200
    cases.append(dict(name="truncated leader repaired", boxes=[[200, 10, 240, 90], [200, 10, 223, 90],
                                                             [300, 0, 310, 20]],
                      scores=[0.25, 0.75, 0.125], labels=[0, 0, 0],
                      windows=[frame, [0, 0, 223, 100], [180, 0, 400, 100]], opts={}, kept=[1, 2],
                      fused=[[200, 10, 240, 90], [300, 0, 310, 20]], members=[2, 1]))
    # a child inside an adult: "ios" suppresses it (inter 40 = its area > 0.5 * 40) but IoU = 40 / 200 < 0.55:
    # not fused, the adult's box stays; under "iou" it is not suppressed at all
    cases.append(dict(name="child inside adult (ios)", boxes=[[0, 0, 10, 20], [2, 12, 7, 20]], scores=[0.75, 0.5],
                      labels=[0, 0], windows=None, opts=dict(metric="ios"), kept=[0], fused=[[0, 0, 10, 20]],
                      members=[1]))
    cases.append(dict(name="child inside adult (iou)", boxes=[[0, 0, 10, 20], [2, 12, 7, 20]], scores=[0.75, 0.5],
                      labels=[0, 0], windows=None, opts=dict(metric="iou"), kept=[0, 1],
                      fused=[[0, 0, 10, 20], [2, 12, 7, 20]], members=[1, 1]))
    # scores 0 and -0.0 at conf 0 take part and fuse (members 2) but weigh nothing: den = 0, the leader's box stays
    cases.append(dict(name="zero scores fall back", boxes=[[0, 0, 10, 20], [2, 0, 12, 20]], scores=[0.0, -0.0],
                      labels=[0, 0], windows=None, opts={}, kept=[0], fused=[[0, 0, 10, 20]], members=[2]))
    # the unordered axis: tile 1 = x in [0, 10], tile 2 = x in [5, 100].  The leader (tile 1, 0.75) is [6, 10] in
    # x, x2 cut; the copy (tile 2, 0.25) is [5, 8.5], x1 cut.  V = [5, 10]: inter 2.5 * 10 = 25, union 40 + 35 -
    # 25 = 50, IoU 0.5 > 0.3.  x1 = (0.75 * 6) / 0.75 = 6 from the leader alone, x2 = (0.25 * 8.5) / 0.25 = 8.5
    # from the copy alone: ordered.  (The frame's candidate has score -1 < conf and takes no part.)
    cases.append(dict(name="axis still ordered", boxes=[[0, 0, 0, 0], [6, 0, 10, 10], [5, 0, 8.5, 10]],
                      scores=[-1.0, 0.75, 0.25], labels=[0, 0, 0],
                      windows=[[0, 0, 100, 10], [0, 0, 10, 10], [5, 0, 100, 10]], opts=dict(fuse_thr=0.3), kept=[1],
                      fused=[[6, 0, 8.5, 10]], members=[2]))
    # unordered: a third tile, x in [0, 9.5], at thr = fuse_thr = 0.1.  Leader (tile 1, 0.5) [6, 10], x2 cut; B
    # (tile 3, 0.5) [9, 9.5], x2 cut: "ios" inter 5 = its area > 0.5, in V = [0, 9.5] IoU = 5 / 35 > 0.1; A (tile
    # 2, 0.25) [5, 7] x [0, 8], x1 cut: inter 8 > 0.1 * 16, in V = [5, 10] IoU = 8 / 48 > 0.1.  x1 = (0.5 * 6 + 0.5
    # * 9) / 1 = 7.5 (leader, B), x2 = (0.25 * 7) / 0.25 = 7 (A alone) < x1: the x axis keeps the leader's 6 and
    # 10, while y fuses: y1 = 0, y2 = (0.5 * 10 + 0.5 * 10 + 0.25 * 8) / 1.25 = 12 / 1.25 = 9.6 (rounded once)
    cases.append(dict(name="unordered axis falls back",
                      boxes=[[0, 0, 0, 0], [6, 0, 10, 10], [5, 0, 7, 8], [9, 0, 9.5, 10]],
                      scores=[-1.0, 0.5, 0.25, 0.5], labels=[0, 0, 0, 0],
                      windows=[[0, 0, 100, 10], [0, 0, 10, 10], [5, 0, 100, 10], [0, 0, 9.5, 10]],
                      opts=dict(fuse_thr=0.1, thr=0.1), kept=[1], fused=[[6, 0, 10, 9.6]], members=[3]))
    # the clamp to the frame: the windows say the frame ends at x = 11, the average x2 = (6 + 5) / 1 = 11.5 -> 11;
    # one pass (P = 1) of two candidates
    cases.append(dict(name="clamp to the frame", boxes=[[0, 0, 12, 20], [2, 0, 11, 20]], scores=[0.5, 0.5],
                      labels=[0, 0], windows=[[0, 0, 11, 20]], opts={}, kept=[0], fused=[[1, 0, 11, 20]],
                      members=[2]))
    # max_det cuts the walk: candidate 1 (a copy of 0) is visited before the second keep and fuses; candidate 3 (a
    # copy of 2) comes after the max_det-th kept one, is not visited and joins nothing
    cases.append(dict(name="max_det cuts the walk", boxes=[[0, 0, 10, 20], [2, 0, 12, 20], [50, 0, 60, 20],
                                                           [52, 0, 62, 20], [0, 0, 10, 20]],
                      scores=[0.5, 0.5, 0.25, 0.25, 0.125], labels=[0, 0, 0, 0, 0], windows=None,
                      opts=dict(max_det=2), kept=[0, 2], fused=[[1, 0, 11, 20], [50, 0, 60, 20]], members=[2, 1]))
    return cases


def run_hand_case(case, fuse):
    """``fuse(boxes [1, N, 4], scores, labels int32, windows [1, P, 4] or None, conf, thr, metric, max_det,
    class_agnostic, fuse_thr)`` -> (kept list, fused tensor [n, 4], members list) of the one image; asserts the
    case's expected answer exactly (the expected numbers are exact in fp32)."""
    o = dict(conf=0.0, thr=0.5, metric="ios", max_det=300, class_agnostic=False, fuse_thr=0.55)
    o.update(case["opts"])
    boxes = torch.tensor(case["boxes"], dtype=torch.float32).reshape(1, -1, 4)
    scores = torch.tensor(case["scores"], dtype=torch.float32).reshape(1, -1)
    labels = torch.tensor(case["labels"], dtype=torch.int32).reshape(1, -1)
    windows = None if case["windows"] is None else torch.tensor(case["windows"], dtype=torch.float32)[None]
    kept, fused, members = fuse(boxes, scores, labels, windows, o["conf"], o["thr"], o["metric"], o["max_det"],
                                o["class_agnostic"], o["fuse_thr"])
    assert kept == case["kept"], (case["name"], kept)
    assert members == case["members"], (case["name"], members)
    want = torch.tensor(case["fused"], dtype=torch.float32).reshape(-1, 4)
    assert torch.equal(fused, want), (case["name"], fused.tolist())
