"""Tiled prediction on the host: merge.tile_windows, merge.merge_reference
against hand-worked answers, and engine.predict(device="cpu", tiles=...) against
the same pipeline built by hand."""
from __future__ import annotations

import math
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
FRAMES = ROOT / "tests" / "golden" / "zod_mini" / "frames"
SPEC = "rtdetr-r18-moe4-top1"
IMGSZ = (320, 640)


# ---------------------------------------------------------------------------
# tile_windows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("L", [7, 64, 271, 483, 2168, 3848])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("o", [0.0, 0.2, 0.5])
def test_tile_windows_cover_the_axis_and_overlap(L, n, o):
    from src.rtdetr_moe.merge import tile_windows

    # the same axis as columns (one row) and as rows (one column)
    cols = tile_windows(L, 11, tiles=(1, n), overlap=o)
    rows = tile_windows(11, L, tiles=(n, 1), overlap=o)
    assert [(x0, tw) for x0, _, tw, _ in cols] == [(y0, th) for _, y0, _, th in rows]
    assert all((y0, th) == (0, 11) for _, y0, _, th in cols) and all((x0, tw) == (0, 11) for x0, _, tw, _ in rows)
    starts = [x0 for x0, _, _, _ in cols]
    t = cols[0][2]
    assert len(cols) == n and all(tw == t for _, _, tw, _ in cols)
    assert t == (L if n == 1 else min(L, math.ceil(L / (n - (n - 1) * o))))
    assert starts[0] == 0 and starts[-1] + t == L
    assert all(isinstance(v, int) for w in cols for v in w)
    for a, b in zip(starts, starts[1:]):
        assert b > a or t == L
        assert a + t - b >= math.floor(o * t) - 1  # neighbours overlap (so the union covers the axis)


def test_tile_windows_of_a_zod_frame():
    from src.rtdetr_moe.merge import tile_windows

    assert tile_windows(3848, 2168, tiles=(2, 2), overlap=0.2) == [
        (0, 0, 2138, 1205), (1710, 0, 2138, 1205), (0, 963, 2138, 1205), (1710, 963, 2138, 1205)]
    # row-major: 2 rows x 3 columns
    w = tile_windows(300, 200, tiles=(2, 3), overlap=0.0)
    assert [(x0, y0) for x0, y0, _, _ in w] == [(0, 0), (100, 0), (200, 0), (0, 100), (100, 100), (200, 100)]
    assert tile_windows(640, 320, tiles=(1, 1), overlap=0.5) == [(0, 0, 640, 320)]


def test_tile_windows_bad_arguments():
    from src.rtdetr_moe.merge import parse_tiles, tile_windows

    for kw in (dict(tiles=(0, 1)), dict(tiles=(1, 0)), dict(tiles=(1, 8)), dict(tiles=(6, 1)),
               dict(overlap=-0.01), dict(overlap=0.51), dict(overlap=float("nan"))):
        with pytest.raises(ValueError):
            tile_windows(7, 5, **{"tiles": (1, 1), "overlap": 0.2, **kw})
    assert len(tile_windows(7, 5, tiles=(5, 7), overlap=0.5)) == 35
    assert parse_tiles("2x3") == (2, 3) and parse_tiles((3, 4)) == (3, 4) and parse_tiles(None) is None
    for bad in ("2", "2x", "0x2", "2x2x2"):
        with pytest.raises(ValueError):
            parse_tiles(bad)


# ---------------------------------------------------------------------------
# merge_reference by hand
# ---------------------------------------------------------------------------
def _merge(boxes, scores, labels, n_valid=None, conf=0.0, thr=0.5, metric="ios", max_det=300, **kw):
    from src.rtdetr_moe.merge import merge_reference

    out = merge_reference(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4),
                          torch.tensor(scores, dtype=torch.float32), torch.tensor(labels), n_valid, conf, thr,
                          metric, max_det, **kw)
    assert out.dtype == np.int64
    return out.tolist()


def test_contained_truncated_box_goes_under_ios_and_stays_under_iou():
    # a person's full-frame box 10 x 20 and a tile's truncated box of the same person, 10 x 8, inside it:
    # inter 80; "ios": den = min(200, 80) = 80 and 80 > 0.5 x 80; "iou": den = 200 + 80 - 80 and 80 < 100
    boxes = [[0, 0, 10, 20], [0, 0, 10, 8]]
    assert _merge(boxes, [0.9, 0.8], [0, 0], metric="ios") == [0]
    assert _merge(boxes, [0.9, 0.8], [0, 0], metric="iou") == [0, 1]
    assert _merge(boxes, [0.8, 0.9], [0, 0], metric="ios") == [1]  # the better score is kept, whichever box it is
    # inter == thr x den exactly is not a suppression (strict >): 10 x 10 against its 10 x 5 half at thr 1 / 0.5
    assert _merge([[0, 0, 10, 10], [0, 0, 10, 5]], [0.9, 0.8], [0, 0], metric="ios", thr=1.0) == [0, 1]
    assert _merge([[0, 0, 10, 10], [0, 0, 10, 5]], [0.9, 0.8], [0, 0], metric="iou", thr=0.5) == [0, 1]
    assert _merge([[0, 0, 10, 10], [0, 0, 10, 6]], [0.9, 0.8], [0, 0], metric="iou", thr=0.5) == [0]
    with pytest.raises(ValueError):
        _merge(boxes, [0.9, 0.8], [0, 0], metric="giou")


def test_labels_separate_unless_class_agnostic():
    boxes = [[0, 0, 10, 20], [1, 1, 10, 20], [0, 0, 10, 19]]
    assert _merge(boxes, [0.9, 0.8, 0.7], [0, 1, 1]) == [0, 1]  # 2 goes to 1 (its label), 1 survives 0
    assert _merge(boxes, [0.9, 0.8, 0.7], [0, 1, 1], class_agnostic=True) == [0]
    assert _merge(boxes, [0.9, 0.8, 0.7], [0, 1, 2]) == [0, 1, 2]


def test_equal_scores_go_by_the_lower_index():
    same = [[0, 0, 10, 20]] * 3
    assert _merge(same, [0.5, 0.5, 0.5], [0, 0, 0]) == [0]
    assert _merge(same + [[50, 50, 60, 60]], [0.5, 0.75, 0.75, 0.75], [0, 0, 0, 0]) == [1, 3]
    # -0.0 and +0.0 are one score
    assert _merge([[0, 0, 1, 1], [5, 5, 6, 6]], [-0.0, 0.0], [0, 0], conf=-1.0) == [0, 1]
    far = [[20 * i, 0, 20 * i + 10, 10] for i in range(4)]
    assert _merge(far, [0.25, 0.5, 0.25, 0.5], [0] * 4) == [1, 3, 0, 2]


def test_who_takes_part():
    far = [[20 * i, 0, 20 * i + 10, 10] for i in range(6)]
    scores = [0.9, float("nan"), 0.2, 0.25, 0.8, 0.7]
    assert _merge(far, scores, [0] * 6, conf=0.25) == [0, 4, 5, 3]  # NaN and 0.2 < conf are out; == conf is in
    assert _merge(far, scores, [0] * 6, conf=0.25, n_valid=5) == [0, 4, 3]
    assert _merge(far, scores, [0] * 6, conf=0.25, n_valid=0) == []
    assert _merge(far, scores, [0] * 6, conf=0.25, n_valid=99) == [0, 4, 5, 3]  # clamped to N
    assert _merge(far, scores, [0] * 6, conf=-float("inf")) == [0, 4, 5, 3, 2]  # NaN never takes part
    # an excluded candidate suppresses nothing
    assert _merge([[0, 0, 10, 20]] * 2, [float("nan"), 0.5], [0, 0]) == [1]
    assert _merge([[0, 0, 10, 20]] * 2, [0.9, 0.5], [0, 0], n_valid=0) == []
    assert _merge([], [], []) == []


def test_max_det_cuts_the_kept_list():
    far = [[20 * i, 0, 20 * i + 10, 10] for i in range(5)]
    assert _merge(far, [0.1, 0.5, 0.3, 0.4, 0.2], [0] * 5, max_det=3) == [1, 3, 2]
    # suppressed candidates do not count towards the cut
    boxes = [[0, 0, 10, 10], [0, 0, 10, 10], [20, 0, 30, 10], [40, 0, 50, 10]]
    assert _merge(boxes, [0.9, 0.8, 0.7, 0.6], [0] * 4, max_det=2) == [0, 2]


def test_zero_area_boxes_are_kept_and_suppress_nothing():
    # a degenerate box inside a big one, at any threshold: inter = 0 is never > thr x den
    boxes = [[0, 0, 10, 20], [5, 5, 5, 9], [5, 5, 5, 9], [3, 7, 8, 7], [6, 6, 2, 2]]  # the last: x2 < x1, area 0
    for metric in ("ios", "iou"):
        for thr in (0.0, 0.5):
            assert _merge(boxes, [0.9, 0.8, 0.7, 0.6, 0.5], [0] * 5, metric=metric, thr=thr) == [0, 1, 2, 3, 4]
            assert _merge(boxes, [0.5, 0.6, 0.7, 0.8, 0.9], [0] * 5, metric=metric, thr=thr) == [4, 3, 2, 1, 0]
    # thr 0: any overlap suppresses; touching boxes do not overlap
    assert _merge([[0, 0, 10, 10], [9, 9, 20, 20], [10, 0, 20, 9]], [0.9, 0.8, 0.7], [0] * 3, thr=0.0) == [0, 2]


# ---------------------------------------------------------------------------
# engine.predict(device="cpu", tiles=...)
# ---------------------------------------------------------------------------
def test_predict_cpu_tiles_equal_the_pipeline_built_by_hand():
    from PIL import Image

    from src.rtdetr_moe import engine
    from src.rtdetr_moe.merge import merge_reference, tile_windows
    from src.rtdetr_moe.preprocess import FrameSource, host_resize, mapped_sizes, padded_hw

    path = sorted(FRAMES.glob("*.jpg"))[0]
    torch.manual_seed(0)
    res = engine.predict(SPEC, [path], imgsz=IMGSZ, batch=1, device="cpu", conf=0.0, workers=0, tiles=(2, 1))
    assert res.speed["passes"] == 3 and set(res.speed) == {"preprocess", "inference", "postprocess", "passes"}
    (p,) = res.predictions
    frame = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
    H, W = frame.shape[:2]
    assert p.size == (W, H) == (1248, 704)
    wins = tile_windows(W, H, tiles=(2, 1), overlap=0.2)
    assert wins == [(0, 0, 1248, 392), (0, 312, 1248, 392)]
    model = res.model.model
    model.eval()
    out_hw, pad_hw = padded_hw(IMGSZ)
    ctx = torch.tensor([FrameSource([path]).context_id(path)], dtype=torch.int32)
    cand = []
    for x0, y0, tw, th in [(0, 0, W, H)] + wins:
        x = host_resize(np.ascontiguousarray(frame[y0:y0 + th, x0:x0 + tw]), out_hw, pad_hw)[None]
        with torch.no_grad():
            out = model(x, ctx)
        b, sc, lb = model.postprocess_batched(out, mapped_sizes([(tw, th)], out_hw, pad_hw), num_top=300)
        lo = torch.tensor([x0, y0, x0, y0], dtype=b.dtype)
        hi = torch.tensor([x0 + tw, y0 + th, x0 + tw, y0 + th], dtype=b.dtype)
        cand.append((torch.minimum(torch.maximum(b[0] + lo, lo), hi), sc[0], lb[0]))
    k = cand[0][0].shape[0]
    assert k == 300
    cb, cs, cl = (torch.cat([c[j] for c in cand]) for j in range(3))
    keep = torch.from_numpy(merge_reference(cb, cs, cl, None, 0.0, 0.5, "ios", 300))
    assert 2 <= len(keep) <= 300 and len(keep) < 3 * k  # something was kept, something went
    assert torch.equal(p.boxes, cb[keep]) and torch.equal(p.scores, cs[keep]) and torch.equal(p.labels, cl[keep])
    assert p.source.dtype == torch.int64 and torch.equal(p.source, keep // k)
    assert p.boxes.dtype == torch.float32 and p.labels.dtype == torch.int64
    assert bool((p.scores[:-1] >= p.scores[1:]).all())
    # a row of tile t lies inside window t
    for t, (x0, y0, tw, th) in enumerate(wins, start=1):
        b = p.boxes[p.source == t]
        assert bool((b[:, [0, 2]] >= x0).all() and (b[:, [0, 2]] <= x0 + tw).all())
        assert bool((b[:, [1, 3]] >= y0).all() and (b[:, [1, 3]] <= y0 + th).all())
    # without tiles: what predict returned before the feature, and no source
    torch.manual_seed(0)
    plain = engine.predict(SPEC, [path], imgsz=IMGSZ, batch=1, device="cpu", conf=0.0, workers=0)
    (q,) = plain.predictions
    assert q.source is None and set(plain.speed) == {"preprocess", "inference", "postprocess"}
    assert torch.equal(q.boxes, cand[0][0]) and torch.equal(q.scores, cand[0][1]) and torch.equal(q.labels, cand[0][2])


def test_predict_rejects_too_many_candidates_and_bad_options():
    from src.rtdetr_moe import engine

    path = sorted(FRAMES.glob("*.jpg"))[0]
    kw = dict(imgsz=(128, 256), batch=1, device="cpu", conf=0.0, workers=0)
    with pytest.raises(ValueError, match="candidates"):
        engine.predict(SPEC, [path], tiles=(4, 4), **kw)  # 17 x 300 = 5100 > 4096
    with pytest.raises(ValueError):
        engine.predict(SPEC, [path], tiles=(2, 2), tile_overlap=0.6, **kw)
    with pytest.raises(ValueError):
        engine.predict(SPEC, [path], tiles=(2, 2), merge_metric="giou", **kw)
    with pytest.raises(ValueError):
        engine.predict(SPEC, [path], tiles=(0, 2), **kw)


def test_boundary_passes_the_tile_options(tmp_path):
    from src.models.vision import rtdetr as B

    torch.manual_seed(0)
    res = B.predict_rtdetr_detector(SPEC, str(FRAMES / "000101.jpg"), imgsz=(128, 256), batch=2, device="cpu",
                                    conf=0.0, tiles=(1, 2), tile_overlap=0.1, merge_iou=0.6, merge_metric="iou",
                                    class_agnostic=True)
    (p,) = res.predictions
    assert res.speed["passes"] == 3 and p.source is not None and set(p.source.tolist()) <= {0, 1, 2}
