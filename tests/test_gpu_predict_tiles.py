"""engine.predict(tiles=...) on the GPU: the tiles as further descriptor rows of
rtdetr_resize_pad_u8 into the uploaded buffer, the same captured graph for every
pass, the merge in one rtdetr_nms_merge launch per batch (rtdetr-r18-moe4-top1,
random weights, conf 0; the model and the size of tests/test_gpu_predict.py)."""
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


def test_tiles_equal_the_pipeline_built_by_hand(hip_lib, tmp_path):
    from PIL import Image

    from src.moe import _lib as L
    from src.rtdetr_moe import engine
    from src.rtdetr_moe.merge import merge_reference
    from src.rtdetr_moe.preprocess import FrameSource, mapped_sizes

    (path,) = _resized_copies(tmp_path, [(1248, 704)])
    res = _predict(tmp_path, batch=1, tiles=(2, 1))
    (p,) = res.predictions
    assert p.size == (1248, 704) and res.speed["passes"] == 3
    model = res.model.model
    model.eval()
    fwd = engine.EvalForward(model)
    dev = torch.device("cuda", 0)
    frame = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
    assert frame.shape == (704, 1248, 3)
    buf = torch.from_numpy(frame.reshape(-1).copy()).to(dev)
    ctx = torch.tensor([FrameSource([path]).context_id(path)], dtype=torch.int32, device=dev)
    stride = 3 * 1248
    # the frame, and the windows of tile_windows(1248, 704, (2, 1), 0.2): rows 0..392 and 312..704
    passes = [((0, 0, 1248, 704), [0, 704, 1248, stride]),
              ((0, 0, 1248, 392), [0, 392, 1248, stride]),
              ((0, 312, 1248, 392), [312 * stride, 392, 1248, stride])]
    cand = []
    for (x0, y0, tw, th), row in passes:
        x = L.resize_pad(buf, torch.tensor([row], dtype=torch.int64), IMGSZ, IMGSZ)
        b, sc, lb = model.postprocess_batched(fwd(x, ctx), mapped_sizes([(tw, th)], IMGSZ, IMGSZ), num_top=300)
        lo = torch.tensor([x0, y0, x0, y0], dtype=b.dtype, device=dev)
        hi = torch.tensor([x0 + tw, y0 + th, x0 + tw, y0 + th], dtype=b.dtype, device=dev)
        cand.append((torch.minimum(torch.maximum(b[0] + lo, lo), hi).cpu(), sc[0].cpu(), lb[0].cpu()))
    k = 300
    cb, cs, cl = (torch.cat([c[j] for c in cand]) for j in range(3))
    keep = torch.from_numpy(merge_reference(cb, cs, cl, None, 0.0, 0.5, "ios", 300))
    assert 2 <= len(keep) < 3 * k
    assert torch.equal(p.boxes, cb[keep]) and torch.equal(p.scores, cs[keep]) and torch.equal(p.labels, cl[keep])
    assert torch.equal(p.source, keep // k) and p.source.dtype == torch.int64
    # without tiles: the full-frame pass alone, and no source
    (q,) = _predict(tmp_path, batch=1).predictions
    assert q.source is None
    assert torch.equal(q.boxes, cand[0][0]) and torch.equal(q.scores, cand[0][1]) and torch.equal(q.labels, cand[0][2])


def test_host_resize_path_crops_on_the_host(hip_lib, tmp_path, monkeypatch):
    """MOE_PREDICT_RESIZE=0: the tiles are numpy crops through host_resize; no resize launch, one merge launch."""
    from PIL import Image

    from src.moe import _lib as L
    from src.rtdetr_moe import engine
    from src.rtdetr_moe.merge import merge_reference, tile_windows
    from src.rtdetr_moe.preprocess import FrameSource, host_resize, mapped_sizes

    (path,) = _resized_copies(tmp_path, [(483, 271)])
    monkeypatch.setenv("MOE_PREDICT_RESIZE", "0")
    L.launch_counts(reset=True)
    res = _predict(tmp_path, batch=1, tiles=(1, 2), merge_metric="iou", merge_iou=0.6)
    counts = L.launch_counts(reset=True)
    assert "resize" not in counts and counts.get("merge") == 1
    (p,) = res.predictions
    model = res.model.model
    model.eval()
    fwd = engine.EvalForward(model)
    dev = torch.device("cuda", 0)
    frame = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
    ctx = torch.tensor([FrameSource([path]).context_id(path)], dtype=torch.int32, device=dev)
    cand = []
    for x0, y0, tw, th in [(0, 0, 483, 271)] + tile_windows(483, 271, (1, 2), 0.2):
        x = host_resize(np.ascontiguousarray(frame[y0:y0 + th, x0:x0 + tw]), IMGSZ, IMGSZ)[None]
        x = x.to(dev).contiguous(memory_format=torch.channels_last)
        b, sc, lb = model.postprocess_batched(fwd(x, ctx), mapped_sizes([(tw, th)], IMGSZ, IMGSZ), num_top=300)
        lo = torch.tensor([x0, y0, x0, y0], dtype=b.dtype, device=dev)
        hi = torch.tensor([x0 + tw, y0 + th, x0 + tw, y0 + th], dtype=b.dtype, device=dev)
        cand.append((torch.minimum(torch.maximum(b[0] + lo, lo), hi).cpu(), sc[0].cpu(), lb[0].cpu()))
    cb, cs, cl = (torch.cat([c[j] for c in cand]) for j in range(3))
    keep = torch.from_numpy(merge_reference(cb, cs, cl, None, 0.0, 0.6, "iou", 300))
    assert torch.equal(p.boxes, cb[keep]) and torch.equal(p.scores, cs[keep]) and torch.equal(p.labels, cl[keep])
    assert torch.equal(p.source, keep // 300)


def test_partial_batch_and_partial_tile_chunk_merge_on_the_gpu_as_on_the_host(hip_lib, tmp_path, monkeypatch):
    from src.moe import _lib as L
    from src.rtdetr_moe import engine
    from src.rtdetr_moe.merge import merge_reference, tile_windows

    sizes = [(640, 320), (483, 271), (1248, 704), (640, 320), (483, 271)]
    paths = _resized_copies(tmp_path, sizes)
    made = []

    class Recording(engine.EvalForward):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(engine, "EvalForward", Recording)
    runs, counts = {}, {}
    for switch in ("1", "0"):
        monkeypatch.setenv("MOE_PREDICT_MERGE", switch)
        L.launch_counts(reset=True)
        runs[switch] = _predict(tmp_path, batch=2, tiles=(2, 2))
        counts[switch] = L.launch_counts(reset=True)
    # batches of 2, 2 and 1 frames: 8, 8 and 4 tile slots in chunks of 2 -> 3 + 10 resize launches, one graph
    assert counts["1"].get("merge") == 3 and counts["1"].get("resize") == 13, counts["1"]
    assert "merge" not in counts["0"] and counts["0"].get("resize") == 13, counts["0"]
    assert len(made) == 2 and all(1 <= len(f.graphs) <= 2 for f in made)
    for res in runs.values():
        assert [p.path for p in res.predictions] == [str(q) for q in paths]
        assert set(res.speed) == {"preprocess", "inference", "postprocess", "passes"} and res.speed["passes"] == 5
        assert all(res.speed[key] > 0 for key in ("preprocess", "inference", "postprocess"))
    for a, b, (w, h) in zip(runs["1"].predictions, runs["0"].predictions, sizes):
        assert torch.equal(a.boxes, b.boxes) and torch.equal(a.scores, b.scores)
        assert torch.equal(a.labels, b.labels) and torch.equal(a.source, b.source)
        n = len(a.scores)
        assert a.size == (w, h) and 2 <= n <= 300 and tuple(a.boxes.shape) == (n, 4)
        assert bool(torch.isfinite(a.boxes).all() and torch.isfinite(a.scores).all())
        assert bool((a.boxes >= 0).all() and (a.boxes[:, [0, 2]] <= w).all() and (a.boxes[:, [1, 3]] <= h).all())
        assert bool((a.scores[:-1] >= a.scores[1:]).all())
        assert set(a.source.tolist()) <= set(range(5))
        for t, (x0, y0, tw, th) in enumerate(tile_windows(w, h, (2, 2), 0.2), start=1):
            bx = a.boxes[a.source == t]
            assert bool((bx[:, [0, 2]] >= x0).all() and (bx[:, [0, 2]] <= x0 + tw).all())
            assert bool((bx[:, [1, 3]] >= y0).all() and (bx[:, [1, 3]] <= y0 + th).all())
        # the kept rows do not suppress one another: merged again, all of them stay
        again = merge_reference(a.boxes, a.scores, a.labels, None, 0.0, 0.5, "ios", 300)
        assert again.tolist() == list(range(n))


def test_candidate_limit(hip_lib, tmp_path, monkeypatch):
    from src.moe import _lib as L
    from src.rtdetr_moe import engine

    _resized_copies(tmp_path, [(640, 320)])
    res = _predict(tmp_path, batch=4, tiles=(3, 4), max_det=300)  # 13 x 300 = 3900 candidates
    (p,) = res.predictions
    assert res.speed["passes"] == 13 and 2 <= len(p.scores) <= 300 and set(p.source.tolist()) <= set(range(13))
    made = []
    monkeypatch.setattr(engine, "EvalForward", lambda *a, **kw: made.append(1))
    L.launch_counts(reset=True)
    with pytest.raises(ValueError, match="candidates"):
        _predict(tmp_path, batch=4, tiles=(4, 4), max_det=300)  # 17 x 300 = 5100
    assert not made and not L.launch_counts(reset=True)
