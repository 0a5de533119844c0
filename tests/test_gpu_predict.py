"""engine.predict on the GPU: frames resized by rtdetr_resize_pad_u8, the
graph-replayed forward, detections in source pixels (rtdetr-r18-moe4-top1,
random weights, conf 0)."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FRAMES = ROOT / "tests" / "golden" / "zod_mini" / "frames"
SPEC = "rtdetr-r18-moe4-top1"
IMGSZ = (320, 640)

# Largest |score difference|, rank by rank, allowed between two runs whose inputs differ by the resize
# path (the kernel's image against PIL's: up to one grey level, passed through a bf16 forward) or by the
# other images of the batch.  Measured on the MI355X with EvalForward as it stands, on these frames:
# 4.1e-4 (1248 x 704 source), 0 (640 x 320: identity scale, the same bits) and 7.7e-4 (483 x 271) between
# the kernel and the host path, and 0 between the last slot of a partial batch and a batch of one (the
# forward is deterministic and per-image here).  The margin is one bf16 ulp below 1.0, 2^-8 = 3.9e-3:
# five times the largest figure measured, and what one rounding of a score-sized activation costs.
SCORE_MARGIN = 2.0 ** -8


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


def _inside(p):
    w, h = p.size
    b = p.boxes
    return bool((b >= 0).all() and (b[:, [0, 2]] <= w).all() and (b[:, [1, 3]] <= h).all())


def _rows_ok(p):
    return (tuple(p.boxes.shape) == (300, 4) and tuple(p.scores.shape) == (300,) == tuple(p.labels.shape)
            and bool(torch.isfinite(p.boxes).all() and torch.isfinite(p.scores).all()) and _inside(p)
            and bool((p.scores[:-1] >= p.scores[1:]).all()))


def test_identity_scale_equals_the_loader_path(hip_lib, tmp_path):
    from PIL import Image

    from src.rtdetr_moe import engine
    from src.rtdetr_moe.data import _padded_image
    from src.rtdetr_moe.preprocess import FrameSource

    paths = _resized_copies(tmp_path, [(640, 320)] * 6)
    res = _predict(tmp_path, batch=2)
    assert [p.path for p in res.predictions] == [str(q) for q in paths]
    model = res.model.model
    model.eval()
    fwd = engine.EvalForward(model)
    ctx_of = FrameSource(paths).context_id
    dev = torch.device("cuda", 0)
    for s in range(0, 6, 2):
        chunk = paths[s:s + 2]
        x = torch.stack([_padded_image(np.asarray(Image.open(q)), 320, 640, False) for q in chunk])
        x = x.to(dev).contiguous(memory_format=torch.channels_last)
        ctx = torch.tensor([ctx_of(q) for q in chunk], dtype=torch.int32, device=dev)
        b, sc, lb = model.postprocess_batched(fwd(x, ctx), [(640.0, 320.0)] * 2)
        lim = torch.tensor([640.0, 320.0, 640.0, 320.0], device=dev)
        b = torch.minimum(b.clamp(min=0.0), lim)
        for i in range(2):
            p = res.predictions[s + i]
            assert p.size == (640, 320) and _rows_ok(p)
            assert torch.equal(p.boxes, b[i].cpu()) and torch.equal(p.scores, sc[i].cpu())
            assert torch.equal(p.labels, lb[i].cpu())


def test_mixed_sizes_in_one_batch(hip_lib, tmp_path, monkeypatch):
    sizes = [(1248, 704), (640, 320), (483, 271)]
    _resized_copies(tmp_path, sizes)
    runs = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("MOE_PREDICT_RESIZE", switch)
        runs[switch] = _predict(tmp_path, batch=3).predictions
    for switch, preds in runs.items():
        assert [p.size for p in preds] == sizes
        assert all(_rows_ok(p) for p in preds), switch
    for a, b in zip(runs["1"], runs["0"]):
        assert torch.equal(a.labels, b.labels)
        d = float((a.scores - b.scores).abs().max())
        print(f"{a.size}: max |score(kernel) - score(host)| = {d:.3e}")
        assert d <= SCORE_MARGIN


def test_partial_last_batch(hip_lib, tmp_path, monkeypatch):
    from src.rtdetr_moe import engine

    paths = _resized_copies(tmp_path, [(640, 320), (483, 271), (1248, 704), (640, 320), (483, 271)])
    made = []

    class Recording(engine.EvalForward):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(engine, "EvalForward", Recording)
    res = _predict(tmp_path, batch=2)
    assert len(res.predictions) == 5 and [p.path for p in res.predictions] == [str(q) for q in paths]
    assert all(_rows_ok(p) for p in res.predictions)
    assert len(made) == 1 and 1 <= len(made[0].graphs) <= 2
    alone = _predict([paths[4]], batch=1).predictions[0]
    last = res.predictions[4]
    assert last.size == alone.size == (483, 271) and torch.equal(last.labels, alone.labels)
    d = float((last.scores - alone.scores).abs().max())
    print(f"last of 5 at batch 2 against batch 1: max |score difference| = {d:.3e}")
    assert d <= SCORE_MARGIN


def test_speed_and_one_resize_launch_per_batch(hip_lib, tmp_path, monkeypatch):
    from src.moe import _lib as L

    _resized_copies(tmp_path, [(483, 271)] * 5)
    L.launch_counts(reset=True)
    res = _predict(tmp_path, batch=2, project=str(tmp_path), name="out")
    counts = L.launch_counts(reset=True)
    assert counts.get("resize") == 3, counts  # 5 frames at batch 2: three batches, one launch each
    assert set(res.speed) == {"preprocess", "inference", "postprocess"}
    assert all(v > 0 for v in res.speed.values())
    assert (res.save_dir / "predictions.json").exists()
    monkeypatch.setenv("MOE_PREDICT_RESIZE", "0")
    _predict(tmp_path, batch=2)
    assert "resize" not in L.launch_counts(reset=True)
