"""predict() on the CPU and the pieces under it: the resize semantics
(preprocess.resize_reference) against an fp64 restatement of the formula and
against the loader's PIL resize, FrameSource and the packed batch, the box
mapping, and engine.predict(device="cpu") end to end on the zod_mini frames."""
from __future__ import annotations

import json
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
FRAMES = ROOT / "tests" / "golden" / "zod_mini" / "frames"
SPEC = "rtdetr-r18-moe4-top1"

# source (h, w) -> content (h, w) of the nine kernel cases (tests/test_gpu_resize.py)
PAIRS = [((37, 53), (37, 53)), ((271, 483), (88, 156)), ((64, 96), (32, 48)), ((50, 70), (120, 200)),
         ((30, 200), (64, 96)), ((1, 1), (32, 32)), ((5, 7), (32, 32)), ((256, 512), (32, 64)),
         ((8, 4000), (8, 1300))]


def _content(rng, h, w, smooth=False):
    a = rng.integers(0, 256, (h, w, 3)).astype(np.float64)
    if smooth and h > 2 and w > 2:
        a = (a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 0) + np.roll(a, -1, 1)) / 5
    return a.round().astype(np.uint8)


def _axis_weights(n_in, n_out):
    """fp64 [n_out, n_in] filter matrix of one axis, straight from the formula."""
    m = np.zeros((n_out, n_in), np.float64)
    scale = n_in / n_out
    support = max(scale, 1.0)
    inv = 1.0 / support
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo, hi = max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n_in)
        w = np.array([max(0.0, 1.0 - abs((j - c + 0.5) * inv)) for j in range(lo, hi)])
        m[i, lo:hi] = w / w.sum()
    return m


@pytest.mark.parametrize("src,out", PAIRS)
def test_reference_equals_the_formula(src, out):
    from src.rtdetr_moe.preprocess import resize_reference

    rng = np.random.default_rng(src[0] * 10007 + src[1])
    x = _content(rng, *src)
    pad = (out[0] + 5, out[1] + 3)
    ref = resize_reference(x, out[0], out[1], *pad)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (3, *pad)
    wy, wx = _axis_weights(src[0], out[0]), _axis_weights(src[1], out[1])
    want = np.stack([wy @ x[:, :, c].astype(np.float64) @ wx.T for c in range(3)]) / 255
    got = ref.numpy()
    assert np.abs(got[:, :out[0], :out[1]] - want).max() <= 1e-12
    assert (got[:, out[0]:, :] == 0).all() and (got[:, :, out[1]:] == 0).all()


@pytest.mark.parametrize("src,out", [((271, 483), (88, 156)), ((50, 70), (120, 200)), ((720, 1280), (704, 1248))])
@pytest.mark.parametrize("smooth", [False, True])
def test_reference_is_the_loader_image_within_one_grey_level(src, out, smooth):
    from PIL import Image

    from src.rtdetr_moe.preprocess import resize_reference

    x = _content(np.random.default_rng(3), *src, smooth=smooth)
    pil = np.asarray(Image.fromarray(x).resize((out[1], out[0]), Image.BILINEAR), dtype=np.float64)
    ref = 255 * resize_reference(x, out[0], out[1], out[0], out[1]).permute(1, 2, 0).numpy()
    err = np.abs(ref - pil).max()
    print(f"{src} -> {out} smooth={smooth}: max |255 reference - PIL| = {err:.6f} grey levels")
    assert err <= 1 + 1e-3


def test_reference_is_exact_at_identity_scale():
    from PIL import Image

    from src.rtdetr_moe.data import _padded_image
    from src.rtdetr_moe.preprocess import host_resize, resize_reference

    x = _content(np.random.default_rng(4), 97, 131)
    pil = np.asarray(Image.fromarray(x).resize((131, 97), Image.BILINEAR))
    assert np.array_equal(pil, x)
    ref = resize_reference(x, 97, 131, 128, 160)
    assert torch.equal(255 * ref[:, :97, :131], torch.from_numpy(x).permute(2, 0, 1).double())
    assert torch.equal(host_resize(x, (97, 131), (128, 160)), _padded_image(x, 128, 160, False))


# ---------------------------------------------------------------------------
# FrameSource, packing, descriptor validation
# ---------------------------------------------------------------------------
def _write_frames(d: Path, sizes, seed=0):
    from PIL import Image

    d.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(seed)
    out = []
    for i, (h, w) in enumerate(sizes):
        p = d / f"{i + 1:04d}.png"
        Image.fromarray(_content(rng, h, w)).save(p)
        out.append(p)
    return out


def test_frame_source_context_resolution_order(tmp_path):
    from src.moe.context import CONTEXT_LABELS, MISSING_ID
    from src.rtdetr_moe.preprocess import FrameSource

    d = tmp_path / "set" / "frames"
    paths = _write_frames(d, [(8, 9), (10, 7)])
    night, mid, low = (CONTEXT_LABELS.index(s) for s in ("night(<-6)", "mid_sun(15..45)", "low_sun(0..15)"))
    # nothing known: missing
    assert [FrameSource(d)[i][2] for i in range(2)] == [MISSING_ID, MISSING_ID]
    # COCO jsons of the dataset root
    ann = tmp_path / "set" / "annotations"
    ann.mkdir()
    (ann / "instances.json").write_text(json.dumps({"images": [
        {"id": 1, "file_name": "0001.png", "solar_context_bin": "night(<-6)"}]}))
    assert [FrameSource(d)[i][2] for i in range(2)] == [night, MISSING_ID]
    # contexts.json beside the source wins over the COCO jsons
    (tmp_path / "set" / "contexts.json").write_text(json.dumps({"0001": "mid_sun(15..45)", "0002": "night(<-6)"}))
    assert [FrameSource(d)[i][2] for i in range(2)] == [mid, night]
    # the argument wins over both: a mapping, or one label for all
    assert [FrameSource(d, contexts={"0002": "low_sun(0..15)"})[i][2] for i in range(2)] == [MISSING_ID, low]
    assert [FrameSource(d, contexts="low_sun(0..15)")[i][2] for i in range(2)] == [low, low]
    # the other source forms: a list, a glob, one file
    assert FrameSource([str(p) for p in paths]).paths == paths
    assert FrameSource(str(d / "*.png")).paths == paths
    assert FrameSource(paths[1]).paths == paths[1:]
    arr, path, _ = FrameSource(d)[1]
    assert arr.dtype == np.uint8 and arr.shape == (10, 7, 3) and path == str(paths[1])
    with pytest.raises(FileNotFoundError):
        FrameSource(tmp_path / "nothing_here")


def test_frame_source_reads_a_dataset_yaml():
    from src.moe.context import CONTEXT_LABELS
    from src.rtdetr_moe.preprocess import FrameSource

    ds = FrameSource(ROOT / "tests" / "golden" / "zod_mini" / "dataset.yaml", split="val")
    assert [p.name for p in ds.paths] == ["000201.jpg", "000202.jpg"]
    assert [ds[i][2] for i in range(2)] == [CONTEXT_LABELS.index("low_sun(0..15)"),
                                            CONTEXT_LABELS.index("twilight(-6..0)")]
    assert FrameSource(FRAMES).context_id("000101.jpg") == CONTEXT_LABELS.index("night(<-6)")


def test_packed_batch_reads_back_through_its_descriptor():
    from src.rtdetr_moe.preprocess import PackCollate, pack_frames, unpack_frame

    rng = np.random.default_rng(5)
    frames = [_content(rng, h, w) for h, w in ((37, 53), (8, 121), (64, 9))]
    bt = PackCollate((32, 64))([(f, f"{i}.png", i) for i, f in enumerate(frames)])
    buf, desc = bt["buf"], bt["desc"]
    assert buf.dtype == torch.uint8 and buf.dim() == 1 and buf.numel() == sum(f.size for f in frames)
    assert desc.dtype == torch.int64 and tuple(desc.shape) == (3, 4)
    for f, row in zip(frames, desc.tolist()):
        assert row[1:] == [f.shape[0], f.shape[1], 3 * f.shape[1]]
        assert np.array_equal(unpack_frame(buf, row), f)
    assert bt["sizes"] == [(53, 37), (121, 8), (9, 64)] and bt["ctx"].tolist() == [0, 1, 2]
    # a frame reduced more than 8x on an axis is handed over at identity scale, already reduced on the host
    big = _content(rng, 40, 600)
    buf, desc = pack_frames([big], out_hw=(32, 64))
    assert desc.tolist() == [[0, 32, 64, 192]] and buf.numel() == 32 * 64 * 3
    assert pack_frames([big], out_hw=(32, 128))[1].tolist() == [[0, 40, 600, 1800]]


def test_iter_batches_keeps_the_order_with_and_without_threads(tmp_path):
    from src.rtdetr_moe.preprocess import FrameSource, PackCollate, iter_batches, unpack_frame

    sizes = [(8 + i, 20 - i) for i in range(7)]
    ds = FrameSource(_write_frames(tmp_path, sizes))
    runs = [list(iter_batches(ds, 3, workers, PackCollate((32, 64)))) for workers in (0, 3)]
    for bts in runs:
        assert [len(b["paths"]) for b in bts] == [3, 3, 1]
        assert [p for b in bts for p in b["paths"]] == [str(p) for p in ds.paths]
        assert [s for b in bts for s in b["sizes"]] == [(w, h) for h, w in sizes]
    for a, b in zip(*runs):
        assert torch.equal(a["buf"], b["buf"]) and torch.equal(a["desc"], b["desc"])
    assert np.array_equal(unpack_frame(runs[1][2]["buf"], runs[1][2]["desc"][0]), ds[6][0])
    it = iter_batches(ds, 2, 2, PackCollate((32, 64)))
    next(it)
    it.close()  # a consumer that stops early leaves no thread behind


def test_descriptor_validation():
    from src.moe import _lib as L

    ok = torch.tensor([[0, 4, 5, 15], [60, 2, 3, 11], [0, 0, 0, 0]], dtype=torch.int64)
    L.check_resize_desc(ok, 60 + 11 + 9)
    with pytest.raises(L.MoEKernelError, match="outside"):
        L.check_resize_desc(ok, 60 + 11 + 8)  # the last row of slot 1 ends one byte past the buffer
    with pytest.raises(L.MoEKernelError, match="outside"):
        L.check_resize_desc(torch.tensor([[100, 4, 5, 15]], dtype=torch.int64), 100)  # offset past the buffer
    with pytest.raises(L.MoEKernelError, match="outside"):
        L.check_resize_desc(torch.tensor([[0, 4, 5, 14]], dtype=torch.int64), 1000)  # stride below 3 w
    with pytest.raises(L.MoEKernelError, match="outside"):
        L.check_resize_desc(torch.tensor([[-1, 4, 5, 15]], dtype=torch.int64), 1000)
    with pytest.raises(L.MoEKernelError, match="largest side"):
        L.check_resize_desc(torch.tensor([[0, 1, 16385, 49155]], dtype=torch.int64), 1 << 20)
    with pytest.raises(L.MoEKernelError, match=r"int64 \[B, 4\]"):
        L.check_resize_desc(torch.zeros((2, 3), dtype=torch.int64), 10)
    with pytest.raises(L.MoEKernelError, match="GPU tensor"):
        L.resize_pad(torch.zeros(60, dtype=torch.uint8), ok[:1], (8, 8), (32, 32))
    assert "rtdetr_resize_pad_u8" in L.SIGNATURES and L.PROF_KINDS[18] == "resize"


# ---------------------------------------------------------------------------
# box mapping
# ---------------------------------------------------------------------------
def test_box_mapping_by_hand():
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.preprocess import mapped_sizes, padded_hw

    out_hw, pad_hw = padded_hw((720, 1280))
    assert (out_hw, pad_hw) == ((720, 1280), (736, 1280))
    sizes = mapped_sizes([(3848, 2168)], out_hw, pad_hw)
    out = {"pred_logits": torch.tensor([[[2.0]]]), "pred_boxes": torch.tensor([[[0.5, 360 / 736, 0.25, 0.5]]])}
    xyxy, _, _ = RTDETRMoE.postprocess_batched(None, out, sizes)
    x1, y1, x2, y2 = xyxy[0, 0].double().tolist()
    assert abs((x1 + x2) / 2 - 1924) < 1e-3 and abs((y1 + y2) / 2 - 1084) < 1e-3
    # 0.25 x 1280 = 320 columns and 0.5 x 736 = 368 rows of the tensor: 320 x 3848 / 1280 = 962 and
    # 368 x 2168 / 720 = 1108.09 source pixels
    assert abs((x2 - x1) - 962) < 1e-3 and abs((y2 - y1) - 368 * 2168 / 720) < 1e-3 and round(y2 - y1) == 1108


# ---------------------------------------------------------------------------
# predict(device="cpu")
# ---------------------------------------------------------------------------
IMGSZ = (320, 640)


@pytest.fixture(scope="module")
def cpu_run(tmp_path_factory):
    from src.rtdetr_moe import engine

    torch.manual_seed(0)
    out = tmp_path_factory.mktemp("predict_cpu")
    res = engine.predict(SPEC, FRAMES, imgsz=IMGSZ, batch=4, device="cpu", conf=0.0, workers=0,
                         project=str(out), name="run", save_json=True, save_img=True)
    return res, out / "run"


def _own_run(model, paths, imgsz, batch, num_top=300):
    """PIL resize -> _padded_image -> model -> postprocess_batched with the mapped sizes, clipped to the frame."""
    from PIL import Image

    from src.rtdetr_moe.data import _padded_image
    from src.rtdetr_moe.preprocess import FrameSource, mapped_sizes, padded_hw

    (h, w), (ph, pw) = padded_hw(imgsz)
    ds_ctx = FrameSource(paths)
    rows = []
    model.eval()
    for s in range(0, len(paths), batch):
        chunk = paths[s:s + batch]
        pil = [Image.open(p).convert("RGB") for p in chunk]
        sizes = [im.size for im in pil]
        x = torch.stack([_padded_image(np.asarray(im.resize((w, h), Image.BILINEAR), dtype=np.uint8), ph, pw, False)
                         for im in pil])
        ctx = torch.tensor([ds_ctx.context_id(p) for p in chunk], dtype=torch.int32)
        with torch.no_grad():
            out = model(x, ctx)
        b, sc, lb = model.postprocess_batched(out, mapped_sizes(sizes, (h, w), (ph, pw)), num_top=num_top)
        lim = torch.tensor([[sw, sh, sw, sh] for sw, sh in sizes], dtype=b.dtype)
        b = torch.minimum(b.clamp(min=0.0), lim[:, None, :])
        rows += [(b[i], sc[i], lb[i]) for i in range(len(chunk))]
    return rows


def test_predict_cpu_rows(cpu_run):
    from src.moe.context import CONTEXT_LABELS

    res, _ = cpu_run
    assert [Path(p.path).name for p in res.predictions] == sorted(f.name for f in FRAMES.glob("*.jpg"))
    assert set(res.speed) == {"preprocess", "inference", "postprocess"} and res.speed["inference"] > 0
    assert res.predictions[0].ctx == CONTEXT_LABELS.index("night(<-6)")
    for p in res.predictions:
        assert p.size == (1248, 704)
        assert tuple(p.boxes.shape) == (300, 4) and p.boxes.dtype == torch.float32
        assert tuple(p.scores.shape) == (300,) == tuple(p.labels.shape) and p.labels.dtype == torch.int64
        assert (p.scores[:-1] >= p.scores[1:]).all()
        assert (p.boxes >= 0).all() and (p.boxes[:, [0, 2]] <= 1248).all() and (p.boxes[:, [1, 3]] <= 704).all()
        assert (p.boxes[:, 2] >= p.boxes[:, 0]).all() and (p.boxes[:, 3] >= p.boxes[:, 1]).all()


def test_predict_cpu_equals_the_loader_path(cpu_run):
    res, _ = cpu_run
    want = _own_run(res.model.model, [p.path for p in res.predictions], IMGSZ, 4)
    for p, (b, sc, lb) in zip(res.predictions, want):
        assert torch.equal(p.boxes, b) and torch.equal(p.scores, sc) and torch.equal(p.labels, lb)


def test_predictions_json_round_trips(cpu_run):
    res, save_dir = cpu_run
    rows = json.loads((save_dir / "predictions.json").read_text())
    assert len(rows) == 300 * len(res.predictions)
    by_image = {}
    for r in rows:
        assert set(r) == {"image_id", "file_name", "category_id", "bbox", "score"}
        by_image.setdefault(r["image_id"], []).append(r)
    for p in res.predictions:
        got = by_image[int(Path(p.path).stem)]  # numeric stems are ints
        assert got[0]["file_name"] == Path(p.path).name
        xywh = torch.tensor([r["bbox"] for r in got], dtype=torch.float64)
        bd = p.boxes.double()
        want = torch.cat([bd[:, :2], bd[:, 2:] - bd[:, :2]], 1)
        assert (xywh - want).abs().max() <= 5.1e-4  # 3 decimals
        assert (torch.tensor([r["score"] for r in got], dtype=torch.float64) - p.scores.double()).abs().max() <= 5.1e-6
        assert [r["category_id"] for r in got] == p.labels.tolist()


def test_save_img_writes_the_source_size(cpu_run):
    from PIL import Image

    res, save_dir = cpu_run
    for p in res.predictions:
        assert Image.open(save_dir / Path(p.path).name).size == p.size


def test_predict_cpu_batches_keep_the_source_order(tmp_path):
    from src.rtdetr_moe import engine

    paths = sorted(FRAMES.glob("*.jpg"))[:5]
    for i, p in enumerate(paths):
        shutil.copy(p, tmp_path / f"frame_{i}.jpg")
    torch.manual_seed(0)
    res = engine.predict(SPEC, tmp_path, imgsz=(128, 256), batch=2, device="cpu", conf=0.0, max_det=50, workers=0)
    assert [Path(p.path).name for p in res.predictions] == [f"frame_{i}.jpg" for i in range(5)]
    assert all(tuple(p.boxes.shape) == (50, 4) for p in res.predictions) and res.save_dir is None
    want = _own_run(res.model.model, [p.path for p in res.predictions], (128, 256), 2, num_top=50)
    for p, (b, sc, lb) in zip(res.predictions, want):
        assert torch.equal(p.boxes, b) and torch.equal(p.scores, sc) and torch.equal(p.labels, lb)
    # conf cuts the rows
    conf = float(res.predictions[0].scores[9])
    torch.manual_seed(0)
    cut = engine.predict(SPEC, [tmp_path / "frame_0.jpg"], imgsz=(128, 256), batch=2, device="cpu", conf=conf,
                         max_det=50, workers=0).predictions[0]
    assert 0 < len(cut.scores) < 50 and (cut.scores >= conf).all() and tuple(cut.boxes.shape) == (len(cut.scores), 4)


def test_boundary_exports_predict(tmp_path):
    from src.models.vision import rtdetr as B

    assert "predict_rtdetr_detector" in B.__all__
    torch.manual_seed(0)
    res = B.predict_rtdetr_detector(SPEC, str(FRAMES / "000101.jpg"), imgsz=(128, 256), batch=1, device="cpu",
                                    conf=0.0, project=str(tmp_path), name="b")
    assert len(res.predictions) == 1 and (tmp_path / "b" / "predictions.json").exists()
