"""Flip test-time augmentation on the CPU: merge.unmirror_boxes, the argument
checks, the pass order and window table, engine.predict(device="cpu",
flip=True) and engine.validate(device="cpu", flip=True), with stand-in forwards
in place of engine.EvalForward (the model's answer is a small function of its
input, so that every expected row can be written down)."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
FRAMES = ROOT / "tests" / "golden" / "zod_mini" / "frames"
SPEC = "rtdetr-r18-moe4-top1"
IMGSZ = (64, 128)


# ---------------------------------------------------------------------------
# unmirror_boxes
# ---------------------------------------------------------------------------
def test_unmirror_boxes_by_hand():
    from src.rtdetr_moe.merge import unmirror_boxes

    b = torch.tensor([[0.0, 1.0, 10.0, 5.0], [3.5, 2.0, 100.0, 9.0], [-2.0, 0.0, 0.25, 1.0]], dtype=torch.float32)
    got = unmirror_boxes(b, 100)
    assert got.dtype == torch.float32
    assert got.tolist() == [[90.0, 1.0, 100.0, 5.0], [0.0, 2.0, 96.5, 9.0], [99.75, 0.0, 102.0, 1.0]]
    # each subtraction is one fp32 operation on the fp32-rounded width: the stated bits
    w = 1248 * (3848 / 1248) / 3  # a float width, as a window of a frame that pack_frames reduced has
    x = torch.tensor([[0.1, 0.0, 1000.7, 1.0]], dtype=torch.float32)
    want = np.array([[np.float32(w) - np.float32(1000.7), 0.0, np.float32(w) - np.float32(0.1), 1.0]], np.float32)
    assert np.array_equal(unmirror_boxes(x, w).numpy(), want)
    assert np.array_equal(unmirror_boxes(x.numpy(), w), want)  # arrays as tensors
    # one width per slot broadcasts over [S, k, 4]
    s = torch.stack([b, b])
    got = unmirror_boxes(s, torch.tensor([[100.0], [50.0]]))
    assert torch.equal(got[0], unmirror_boxes(b, 100)) and torch.equal(got[1], unmirror_boxes(b, 50))
    with pytest.raises(ValueError, match="fp32"):
        unmirror_boxes(b.double(), 100)


def test_unmirror_boxes_is_an_involution_on_exact_inputs():
    from src.rtdetr_moe.merge import unmirror_boxes

    rng = np.random.default_rng(0)
    # quarter pixels below 4096 and an integer width: every difference is exact in fp32
    b = torch.from_numpy((rng.integers(0, 4 * 4096, (500, 4)) / 4).astype(np.float32))
    for width in (1, 1248, 3848):
        once = unmirror_boxes(b, width)
        assert torch.equal(unmirror_boxes(once, width), b)
        assert torch.equal(once[:, [1, 3]], b[:, [1, 3]])
        assert torch.equal(once[:, 2] - once[:, 0], b[:, 2] - b[:, 0])  # the width of a box is kept


# ---------------------------------------------------------------------------
# arguments, limits, pass order
# ---------------------------------------------------------------------------
def test_check_args_and_candidates_with_flip():
    from types import SimpleNamespace

    from src.rtdetr_moe.predictor import _check_args, _check_candidates

    base = (0.2, "fuse", 0.5, "ios", 0.55, None)
    with pytest.raises(ValueError, match="give tiles"):  # the existing message, with neither
        _check_args(None, *base)
    assert _check_args(None, *base, True) == (None, None, True)  # fuse with flip and no tiles
    assert _check_args((2, 2), *base, True) == (None, (2, 2), True)
    with pytest.raises(ValueError, match="merge_metric"):  # the merge's arguments are checked for the two-pass run
        _check_args(None, 0.2, "nms", 0.5, "giou", 0.55, None, True)
    with pytest.raises(ValueError, match="merge_iou"):
        _check_args(None, 0.2, "nms", 1.5, "ios", 0.55, None, True)
    _check_args(None, 0.2, "nms", 1.5, "giou", 0.55, None)  # without tiles and flip they are not looked at

    model = SimpleNamespace(decoder=SimpleNamespace(num_queries=300), num_classes=1)
    assert _check_candidates(None, False, 300, model) == 0
    assert _check_candidates(None, False, 300, model, True) == 0  # two passes, 600 candidates
    assert _check_candidates((2, 2), True, 300, model, True) == 4  # 10 passes, 3000 candidates
    with pytest.raises(ValueError, match=r"3x3 with flip.*6000 candidates"):
        _check_candidates((3, 3), False, 300, model, True)
    assert _check_candidates((3, 3), False, 300, model) == 9  # 3000 without flip
    # 2 x 37 passes of 50 candidates fit the merge (3700) but not the fusion's 64 windows
    assert _check_candidates((6, 6), False, 50, model, True) == 36
    with pytest.raises(ValueError, match=r"flip.*74 passes"):
        _check_candidates((6, 6), True, 50, model, True)
    with pytest.raises(ValueError, match="flip"):
        _check_candidates(None, False, 2000, model, True)  # max_det above the merge's


def test_predict_refuses_before_any_work(monkeypatch):
    from src.rtdetr_moe import engine, preprocess

    made = []
    monkeypatch.setattr(preprocess, "FrameSource", lambda *a, **k: made.append(1))
    monkeypatch.setattr(engine, "EvalForward", lambda *a, **k: made.append(1))
    with pytest.raises(ValueError, match="flip"):
        engine.predict(SPEC, [FRAMES / "000101.jpg"], imgsz=IMGSZ, batch=1, device="cpu", tiles=(3, 3), flip=True)
    with pytest.raises(ValueError, match="fuse_iou"):
        engine.predict(SPEC, [FRAMES / "000101.jpg"], imgsz=IMGSZ, batch=1, device="cpu", merge="fuse", fuse_iou=2,
                       flip=True)
    assert not made


def test_window_table_and_pass_order_for_1x2_tiles():
    from src.rtdetr_moe.merge import tile_windows
    from src.rtdetr_moe.predictor import _pass_windows

    wins = tile_windows(100, 40, (1, 2), 0.2)
    assert wins == [(0, 0, 56, 40), (44, 0, 56, 40)]
    plain = _pass_windows([(100, 40)], [wins])
    assert plain.tolist() == [[[0, 0, 100, 40], [0, 0, 56, 40], [44, 0, 100, 40]]]
    both = _pass_windows([(100, 40)], [wins], True)
    assert both.dtype == torch.float32 and tuple(both.shape) == (1, 6, 4)
    assert torch.equal(both[:, :3], plain) and torch.equal(both[:, 3:], plain)  # pass 3 + p has pass p's window
    assert _pass_windows([(100, 40), (7, 9)], None, True).tolist() == [[[0, 0, 100, 40]] * 2, [[0, 0, 7, 9]] * 2]


# ---------------------------------------------------------------------------
# predict(device="cpu", flip=True)
# ---------------------------------------------------------------------------
Q = 6
# cx, cy, w, h of the stand-in's queries, normalised: not symmetric about the middle column
TABLE = torch.tensor([[0.20, 0.30, 0.10, 0.20], [0.70, 0.40, 0.20, 0.30], [0.45, 0.60, 0.30, 0.20],
                      [0.10, 0.80, 0.10, 0.10], [0.90, 0.20, 0.15, 0.25], [0.55, 0.50, 0.05, 0.60]])


class StandIn:
    """In place of engine.EvalForward: query q's box is TABLE[q] and its logit the mean of a column band of the
    input's left half, so that an image and its mirror get different answers."""
    calls = []

    def __init__(self, model=None):
        self.graphs = {}

    def prepare(self, images, ctx):
        pass

    def __call__(self, images, ctx):
        StandIn.calls.append(images.clone())
        B, W = images.shape[0], images.shape[-1]
        band = W // (2 * Q)
        logits = torch.stack([images[..., q * band:(q + 1) * band].mean(dim=(1, 2, 3)) for q in range(Q)], 1) * 6 - 3
        return {"pred_logits": logits[..., None], "pred_boxes": TABLE[None].expand(B, Q, 4).clone()}


def _frame(h, w, seed, palindrome=False):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if palindrome:
        a[:, w - w // 2:] = a[:, :w // 2][:, ::-1]
    return a


def _save(tmp_path, name, a):
    from PIL import Image

    p = tmp_path / name
    Image.fromarray(a).save(p)
    return p


@pytest.fixture
def recorded(monkeypatch):
    """predict with the stand-in forward; the candidates every merge is handed, as (boxes, scores, labels, windows)."""
    from src.rtdetr_moe import engine, predictor

    seen = []
    merge = predictor._merge_rows

    def spy(cb, cs, cl, rule, fuse_iou, win, *a, **kw):
        seen.append((cb.clone(), cs.clone(), cl.clone(), None if win is None else win.clone()))
        return merge(cb, cs, cl, rule, fuse_iou, win, *a, **kw)

    monkeypatch.setattr(engine, "EvalForward", StandIn)
    monkeypatch.setattr(predictor, "_merge_rows", spy)
    StandIn.calls = []
    return seen


def _hand_pass(crop, x0, y0, mirror):
    """One pass built by hand: host_resize of the crop (mirrored: of its mirrored bytes), the stand-in,
    postprocess_batched with the mapped size, un-mirroring, shift and clip."""
    from src.rtdetr_moe.merge import unmirror_boxes
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.preprocess import host_resize, mapped_sizes

    th, tw = crop.shape[:2]
    x = host_resize(np.ascontiguousarray(crop[:, ::-1]) if mirror else crop, IMGSZ, IMGSZ)[None]
    out = StandIn()(x, None)
    b, sc, lb = RTDETRMoE.postprocess_batched(None, out, mapped_sizes([(tw, th)], IMGSZ, IMGSZ), num_top=300)
    b = b[0]
    if mirror:
        b = unmirror_boxes(b, tw)
    lo = torch.tensor([x0, y0, x0, y0], dtype=b.dtype)
    hi = torch.tensor([x0 + tw, y0 + th, x0 + tw, y0 + th], dtype=b.dtype)
    return torch.minimum(torch.maximum(b + lo, lo), hi), sc[0], lb[0]


def test_predict_cpu_flip_candidates_are_the_passes_built_by_hand(tmp_path, recorded):
    from src.rtdetr_moe import engine
    from src.rtdetr_moe.merge import merge_reference, tile_windows

    a = _frame(48, 100, 1)
    path = _save(tmp_path, "a.png", a)
    res = engine.predict(SPEC, [path], imgsz=IMGSZ, batch=2, device="cpu", conf=0.0, workers=0, tiles=(1, 2),
                         flip=True)
    assert res.speed["passes"] == 6 and len(recorded) == 1
    cb, cs, cl, win = recorded[0]
    assert tuple(cb.shape) == (1, 6 * Q, 4) and win is None
    wins = [(0, 0, 100, 48)] + tile_windows(100, 48, (1, 2), 0.2)
    order = [(w, False) for w in wins] + [(w, True) for w in wins]  # today's passes, then their mirrored copies
    for p, ((x0, y0, tw, th), mirror) in enumerate(order):
        b, sc, lb = _hand_pass(a[y0:y0 + th, x0:x0 + tw], x0, y0, mirror)
        rows = slice(p * Q, (p + 1) * Q)
        assert torch.equal(cb[0, rows], b) and torch.equal(cs[0, rows], sc) and torch.equal(cl[0, rows], lb), p
    # a mirrored pass really saw other pixels
    assert not torch.equal(cs[0, :Q], cs[0, 3 * Q:4 * Q])
    (p,) = res.predictions
    keep = torch.from_numpy(merge_reference(cb[0], cs[0], cl[0], None, 0.0, 0.5, "ios", 300))
    assert torch.equal(p.boxes, cb[0][keep]) and torch.equal(p.scores, cs[0][keep])
    assert torch.equal(p.source, keep // Q) and int(p.source.max()) < 6 and p.members is None
    # the unmirrored prefix of the table is the table of the run without flip
    recorded.clear()
    off = engine.predict(SPEC, [path], imgsz=IMGSZ, batch=2, device="cpu", conf=0.0, workers=0, tiles=(1, 2))
    assert off.speed["passes"] == 3
    assert torch.equal(recorded[0][0], cb[:, :3 * Q]) and torch.equal(recorded[0][1], cs[:, :3 * Q])


def test_predict_cpu_flip_on_a_self_mirror_frame(tmp_path, recorded):
    from src.rtdetr_moe import engine
    from src.rtdetr_moe.merge import unmirror_boxes
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.preprocess import mapped_sizes

    a = _frame(40, 64, 2, palindrome=True)
    assert np.array_equal(a, a[:, ::-1])
    path = _save(tmp_path, "p.png", a)
    res = engine.predict(SPEC, [path], imgsz=IMGSZ, batch=1, device="cpu", conf=0.0, workers=0, flip=True,
                         merge="fuse")
    assert res.speed["passes"] == 2 and set(res.speed) == {"preprocess", "inference", "postprocess", "passes"}
    first, second = StandIn.calls
    assert torch.equal(first, second)  # the mirrored pass's input is the unmirrored pass's, bit for bit
    cb, cs, cl, win = recorded[0]
    assert tuple(cb.shape) == (1, 2 * Q, 4) and win.tolist() == [[[0, 0, 64, 40]] * 2]
    # its candidates are the unmirrored pass's, un-mirrored (the clip to the frame commutes with it: the frame's
    # own edges map onto each other)
    lim = torch.tensor([64.0, 40.0, 64.0, 40.0])
    raw, _, _ = _hand_pass(a, 0, 0, False)
    b, sc, lb = RTDETRMoE.postprocess_batched(None, StandIn()(first, None), mapped_sizes([(64, 40)], IMGSZ, IMGSZ))
    assert torch.equal(cb[0, :Q], torch.minimum(b[0].clamp(min=0.0), lim)) and torch.equal(cb[0, :Q], raw)
    assert torch.equal(cb[0, Q:], torch.minimum(unmirror_boxes(b[0], 64).clamp(min=0.0), lim))
    assert torch.equal(cs[0, Q:], cs[0, :Q]) and torch.equal(cl[0, Q:], cl[0, :Q])
    (p,) = res.predictions
    assert p.members is not None and bool((p.members >= 1).all()) and int(p.source.max()) < 2


def test_predict_cpu_without_flip_is_unchanged(tmp_path, recorded):
    from src.rtdetr_moe import engine

    path = _save(tmp_path, "a.png", _frame(48, 100, 3))
    kw = dict(imgsz=IMGSZ, batch=1, device="cpu", conf=0.0, workers=0)
    a = engine.predict(SPEC, [path], **kw).predictions[0]
    n_calls = len(StandIn.calls)
    b = engine.predict(SPEC, [path], flip=False, **kw)
    assert len(StandIn.calls) == 2 * n_calls == 2 and not recorded  # one forward, no merge
    assert set(b.speed) == {"preprocess", "inference", "postprocess"}
    (b,) = b.predictions
    assert torch.equal(a.boxes, b.boxes) and torch.equal(a.scores, b.scores) and torch.equal(a.labels, b.labels)
    assert a.source is None and b.source is None and b.members is None
    raw, sc, lb = _hand_pass(_frame(48, 100, 3), 0, 0, False)
    assert torch.equal(b.scores, sc) and torch.equal(b.boxes, raw)


def test_boundary_and_scripts_pass_flip(tmp_path, recorded):
    from scripts import predict_detector
    from src.models.vision import rtdetr as B

    path = _save(tmp_path, "a.png", _frame(48, 100, 4))
    res = B.predict_rtdetr_detector(SPEC, str(path), imgsz=IMGSZ, batch=1, device="cpu", conf=0.0, flip=True)
    assert res.speed["passes"] == 2 and res.predictions[0].source is not None
    trk = B.predict_rtdetr_tracker(SPEC, str(path), imgsz=IMGSZ, batch=1, device="cpu", conf=0.0, flip=True)
    assert trk.speed["passes"] == 2 and trk.predictions[0].track_ids is not None
    a = predict_detector.parse_args(["--weights", SPEC, "--source", "x", "--flip", "--merge", "fuse"])
    assert a.flip and a.merge == "fuse" and not predict_detector.parse_args(["--weights", SPEC, "--source", "x"]).flip


# ---------------------------------------------------------------------------
# validate(device="cpu", flip=True)
# ---------------------------------------------------------------------------
VAL_IMGSZ = (64, 112)  # padded to 64 x 128: the content's width is not the tensor's
CW, BAND = 112, 16
# per image its painted rectangles (x1, y1, x2, y2) in pixels: 4 columns wide, one per band of 16 columns, every
# height different (the stand-in scores by height); the set is not symmetric about the content's middle column
RECTS = [[(2, 4, 6, 20), (25, 10, 29, 42), (81, 30, 85, 38)], [(35, 0, 39, 24), (106, 20, 110, 60)]]


def _painted_batches(*a, **kw):
    """In place of engine._batches: one batch of two black images with RECTS painted white, RECTS the truth."""
    images = torch.zeros((2, 3, 64, 128))
    targets = []
    for i, rects in enumerate(RECTS):
        for x1, y1, x2, y2 in rects:
            images[i, :, y1:y2, x1:x2] = 1.0
        boxes = torch.tensor([[(x1 + x2) / 2 / 128, (y1 + y2) / 2 / 64, (x2 - x1) / 128, (y2 - y1) / 64]
                              for x1, y1, x2, y2 in rects], dtype=torch.float32)
        targets.append({"boxes": boxes, "labels": torch.zeros(len(rects), dtype=torch.int64)})
    yield images, targets, torch.zeros(2, dtype=torch.int32)


class Painted:
    """A mirror-equivariant stand-in for engine.EvalForward on _painted_batches: query q answers with the bounding
    box of the white pixels of the content's column band [16 q, 16 q + 16), scored by the box's height (no white
    pixel: a score far under the evaluator's threshold).  Every value is exact in fp32.  Mirroring the content
    (112 columns) hands band q's pixels, mirrored, to query 6 - q, so the mirrored image's boxes are the mirrors of
    the image's, with the same scores."""
    calls = 0
    route_stats = None

    def __init__(self, model=None):
        pass

    def prepare(self, images, ctx):
        pass

    def __call__(self, images, ctx):
        Painted.calls += 1
        B, _, H, W = images.shape
        nq = CW // BAND
        logits, boxes = torch.full((B, nq, 1), -20.0), torch.zeros((B, nq, 4))
        for b in range(B):
            for q in range(nq):
                on = images[b, 0, :, q * BAND:(q + 1) * BAND] > 0.5
                if bool(on.any()):
                    cols, rows = on.any(0).nonzero().flatten(), on.any(1).nonzero().flatten()
                    x1, x2 = q * BAND + int(cols.min()), q * BAND + int(cols.max()) + 1
                    y1, y2 = int(rows.min()), int(rows.max()) + 1
                    boxes[b, q] = torch.tensor([(x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H])
                    logits[b, q, 0] = (y2 - y1) / 8 - 1
        return {"pred_logits": logits, "pred_boxes": boxes}


def test_validate_cpu_flip_with_an_equivariant_forward_keeps_the_metrics(monkeypatch):
    from src.rtdetr_moe import engine, merge

    monkeypatch.setattr(engine, "EvalForward", Painted)
    monkeypatch.setattr(engine, "_batches", _painted_batches)
    kw = dict(imgsz=VAL_IMGSZ, batch=2, device="cpu", workers=0)
    Painted.calls = 0
    off = engine.validate(SPEC, "painted", **kw)
    assert Painted.calls == 1
    assert off.box.map50 == 1.0 and off.box.map == 1.0  # the stand-in finds every truth exactly
    named = engine.validate(SPEC, "painted", flip=False, merge="fuse", merge_metric="not looked at", **kw)
    assert Painted.calls == 2 and named.results_dict == off.results_dict
    for mode in ("nms", "fuse"):
        Painted.calls = 0
        on = engine.validate(SPEC, "painted", flip=True, merge=mode, size_report=True, **kw)
        assert Painted.calls == 2  # twice the forwards
        # the mirrored pass's rows, un-mirrored with the content's width, are the first pass's: the merge drops the
        # copies (the fusion averages a box with itself) and the evaluator sees the single pass's rows
        assert on.results_dict == off.results_dict and on.box.map == 1.0
        assert on.size is not None and on.size["images"] == 2 and on.size["detection"]["all"]["AP50"] == 1.0
        assert set(on.speed) == set(off.speed) and on.speed["inference"] > 0
    # the test can tell: un-mirrored with another width, or not at all, the copies land elsewhere, survive the merge
    # as false positives and the metrics move
    true_unmirror = merge.unmirror_boxes
    for broken in (lambda b, w: b, lambda b, w: true_unmirror(b, 128), lambda b, w: true_unmirror(b, w + 3)):
        monkeypatch.setattr(merge, "unmirror_boxes", broken)
        bad = engine.validate(SPEC, "painted", flip=True, **kw)
        assert bad.box.map50 < 1.0 and bad.results_dict != off.results_dict
    monkeypatch.setattr(merge, "unmirror_boxes", true_unmirror)
    with pytest.raises(ValueError, match="merge_metric"):
        engine.validate(SPEC, "painted", flip=True, merge_metric="giou", **kw)
    # the boundary keeps the reference's signature: its switch is the environment's
    from src.models.vision import rtdetr as B

    Painted.calls = 0
    B.eval_rtdetr_detector("painted", SPEC, imgsz=VAL_IMGSZ, batch=2, device="cpu")
    assert Painted.calls == 1
    monkeypatch.setenv("MOE_EVAL_FLIP", "1")
    monkeypatch.setenv("MOE_EVAL_MERGE", "fuse")
    m = B.eval_rtdetr_detector("painted", SPEC, imgsz=VAL_IMGSZ, batch=2, device="cpu")
    assert Painted.calls == 3 and m.results_dict == off.results_dict
    monkeypatch.setenv("MOE_EVAL_MERGE", "wbf")
    with pytest.raises(ValueError, match="merge"):
        B.eval_rtdetr_detector("painted", SPEC, imgsz=VAL_IMGSZ, batch=2, device="cpu")


@pytest.mark.parametrize("mode", ["nms", "fuse"])
def test_validate_cpu_flip_scores_the_rows_built_by_hand(monkeypatch, mode):
    """The rows the evaluator is handed, against the rule written out: the first pass's rows, the mirrored pass's
    un-mirrored with the content's width, concatenated in that order, merged (fused) to K rows at conf 0.  The
    stand-in is predict's above: its answers to an image and to its mirror differ, and its boxes are not symmetric."""
    from src.rtdetr_moe import engine, metrics
    from src.rtdetr_moe.merge import fuse_reference, merge_reference, unmirror_boxes
    from src.rtdetr_moe.model import RTDETRMoE

    handed = []
    update = metrics.DetectionEvaluator.update

    def spy(self, boxes, scores, labels, *a, **kw):
        handed.append((np.array(boxes), np.array(scores), np.array(labels)))
        return update(self, boxes, scores, labels, *a, **kw)

    monkeypatch.setattr(engine, "EvalForward", StandIn)
    monkeypatch.setattr(metrics.DetectionEvaluator, "update", spy)
    StandIn.calls = []
    engine.validate(SPEC, "synthetic:2", imgsz=VAL_IMGSZ, batch=3, device="cpu", workers=0, flip=True, merge=mode,
                    merge_iou=0.4, merge_metric="iou", fuse_iou=0.3)
    assert len(StandIn.calls) == 4 and len(handed) == 6
    n = 0
    for images, mirrored in zip(StandIn.calls[0::2], StandIn.calls[1::2]):
        assert tuple(images.shape) == (3, 3, 64, 128) and bool((images[..., :CW] != 0).any())
        want = images.clone()
        want[..., :CW] = torch.flip(images[..., :CW], dims=(-1,))
        assert torch.equal(mirrored, want) and not torch.equal(mirrored, images)  # the content mirrored, padding kept
        first = RTDETRMoE.postprocess_batched(None, StandIn()(images, None), [(128, 64)] * 3)
        second = RTDETRMoE.postprocess_batched(None, StandIn()(mirrored, None), [(128, 64)] * 3)
        assert not torch.equal(first[1], second[1])
        for i in range(3):
            cb = torch.cat([first[0][i], unmirror_boxes(second[0][i], CW)])
            cs, cl = torch.cat([first[1][i], second[1][i]]), torch.cat([first[2][i], second[2][i]])
            if mode == "fuse":
                win = torch.tensor([[0.0, 0.0, 112.0, 64.0]] * 2)
                keep, boxes, members = fuse_reference(cb, cs, cl, None, 0.0, 0.4, "iou", Q, False, 0.3, win)
                boxes = boxes.reshape(-1, 4)
            else:
                keep = merge_reference(cb, cs, cl, None, 0.0, 0.4, "iou", Q)
                boxes = cb[torch.from_numpy(keep)].numpy()
            assert 1 <= len(keep) <= Q
            got = handed[n]
            assert np.array_equal(got[0], boxes) and np.array_equal(got[1], cs[torch.from_numpy(keep)].numpy())
            assert np.array_equal(got[2], cl[torch.from_numpy(keep)].numpy())
            n += 1
    StandIn.calls = []


def test_validate_cpu_flip_with_the_real_model():
    from src.rtdetr_moe import engine

    torch.manual_seed(0)
    m = engine.validate(SPEC, "synthetic:1", imgsz=(128, 128), batch=2, device="cpu", workers=0, flip=True,
                        context_report=True)
    assert 0.0 <= m.box.map50 <= 1.0 and m.speed["inference"] > 0
    torch.manual_seed(0)
    one = engine.validate(SPEC, "synthetic:1", imgsz=(128, 128), batch=2, device="cpu", workers=0,
                          context_report=True)
    # the routing tables count the unmirrored pass only
    assert m.context["routing"] == one.context["routing"]
