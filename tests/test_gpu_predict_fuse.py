"""engine.predict(tiles=..., merge="fuse") on the GPU: the fusion in one
rtdetr_box_fuse launch per batch in place of the merge's, members with the one
packed copy back (rtdetr-r18-moe4-top1, random weights, conf 0; the model and
the sizes of tests/test_gpu_predict_tiles.py)."""
from __future__ import annotations

from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FRAMES = ROOT / "tests" / "golden" / "zod_mini" / "frames"
SPEC = "rtdetr-r18-moe4-top1"
IMGSZ = (320, 640)
SIZES = [(640, 320), (483, 271), (1248, 704), (640, 320), (483, 271)]


def _resized_copies(tmp_path, sizes):
    """The zod_mini frames written at the given (w, h) sizes (PNG: decoded bytes are the written ones)."""
    from PIL import Image

    out = []
    for i, (p, wh) in enumerate(zip(sorted(FRAMES.glob("*.jpg")), sizes)):
        q = tmp_path / f"{i:02d}_{p.stem}.png"
        Image.open(p).convert("RGB").resize(wh, Image.BILINEAR).save(q)
        out.append(q)
    return out


def _predict(source, batch, **kw):
    from src.rtdetr_moe import engine

    torch.manual_seed(0)  # the spec's random weights: the same model in every run
    return engine.predict(SPEC, source, imgsz=IMGSZ, batch=batch, device="0", conf=0.0, workers=0, **kw)


def test_fuse_on_the_gpu_as_on_the_host_and_nms_unchanged(hip_lib, tmp_path, monkeypatch):
    from src.moe import _lib as L
    from src.rtdetr_moe.merge import merge_reference

    paths = _resized_copies(tmp_path, SIZES)
    runs, counts = {}, {}
    for switch in ("1", "0"):
        monkeypatch.setenv("MOE_PREDICT_MERGE", switch)
        L.launch_counts(reset=True)
        runs[switch] = _predict(tmp_path, batch=2, tiles=(2, 2), merge="fuse")
        counts[switch] = L.launch_counts(reset=True)
    # batches of 2, 2 and 1 frames: one fuse launch each and no merge launch; the host path launches neither
    assert counts["1"].get("box_fuse") == 3 and "merge" not in counts["1"], counts["1"]
    assert "box_fuse" not in counts["0"] and "merge" not in counts["0"], counts["0"]
    monkeypatch.setenv("MOE_PREDICT_MERGE", "1")
    L.launch_counts(reset=True)
    nms = _predict(tmp_path, batch=2, tiles=(2, 2), merge="nms")
    c = L.launch_counts(reset=True)
    assert c.get("merge") == 3 and "box_fuse" not in c, c
    plain = _predict(tmp_path, batch=2, tiles=(2, 2))  # the call as it was before the argument existed
    fused_rows = 0
    for a, b, s, q, (w, h) in zip(runs["1"].predictions, runs["0"].predictions, nms.predictions, plain.predictions,
                                  SIZES):
        assert [a.path, b.path] == [s.path, s.path]
        assert torch.equal(a.boxes, b.boxes) and torch.equal(a.members, b.members)
        assert torch.equal(a.scores, b.scores) and torch.equal(a.labels, b.labels) and torch.equal(a.source, b.source)
        n = len(a.scores)
        assert a.size == (w, h) and 2 <= n <= 300 and tuple(a.boxes.shape) == (n, 4)
        assert a.members.dtype == torch.int64 and tuple(a.members.shape) == (n,) and bool((a.members >= 1).all())
        assert bool(torch.isfinite(a.boxes).all())
        assert bool((a.boxes >= 0).all() and (a.boxes[:, [0, 2]] <= w).all() and (a.boxes[:, [1, 3]] <= h).all())
        assert bool((a.boxes[:, 0] <= a.boxes[:, 2]).all() and (a.boxes[:, 1] <= a.boxes[:, 3]).all())
        assert bool((a.scores[:-1] >= a.scores[1:]).all())
        # merge="nms": the parent's results -- the default call's, which are merge_reference's kept rows (as
        # tests/test_gpu_predict_tiles.py holds them to) -- and the rows fusion keeps, boxes apart
        assert s.members is None and q.members is None
        assert torch.equal(s.boxes, q.boxes) and torch.equal(s.scores, q.scores) and torch.equal(s.labels, q.labels)
        assert torch.equal(s.source, q.source)
        assert torch.equal(s.scores, a.scores) and torch.equal(s.labels, a.labels) and torch.equal(s.source, a.source)
        again = merge_reference(s.boxes, s.scores, s.labels, None, 0.0, 0.5, "ios", 300)
        assert again.tolist() == list(range(n))
        # a row that fused nothing keeps its box up to the two roundings of (s c) / s: |error| <= 2 u (1 + u) c
        # with u = 2^-24 and c <= max(w, h), below 2^-22 max(w, h)
        fused_rows += int((a.members >= 2).sum())
        assert bool(((a.boxes - s.boxes).abs().max(1).values[a.members == 1] <= 2.0 ** -22 * max(w, h)).all())
    assert fused_rows >= 5 and any(not torch.equal(a.boxes, s.boxes)
                                   for a, s in zip(runs["1"].predictions, nms.predictions))


def test_fuse_limits_and_options_are_refused_before_any_launch(hip_lib, tmp_path, monkeypatch):
    from src.moe import _lib as L
    from src.rtdetr_moe import engine

    _resized_copies(tmp_path, [(640, 320)])
    made = []
    monkeypatch.setattr(engine, "EvalForward", lambda *a, **kw: made.append(1))
    L.launch_counts(reset=True)
    with pytest.raises(ValueError, match="tiles"):
        _predict(tmp_path, batch=2, merge="fuse")
    with pytest.raises(ValueError, match="merge"):
        _predict(tmp_path, batch=2, tiles=(2, 2), merge="soft")
    with pytest.raises(ValueError, match="passes"):
        _predict(tmp_path, batch=2, tiles=(8, 9), merge="fuse", max_det=50)
    assert not made and not L.launch_counts(reset=True)
