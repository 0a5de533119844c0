"""Batch augmentation on the CPU: the -aug spec token, the plain-torch
reference (identity, flip, the box keep thresholds), the parameter draw, and a
CPU TrainStep with and without it."""
from __future__ import annotations

import pytest
import torch

SPEC = "rtdetr-r18-moe4-top1-dec1"
H, W, HP, WP = 40, 60, 64, 64


def _batch(B=3, M=16, seed=0):
    from src.rtdetr_moe.criterion import pad_targets

    g = torch.Generator().manual_seed(seed)
    img = torch.zeros((B, 3, HP, WP), dtype=torch.uint8)
    img[:, :, :H, :W] = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    targets = []
    for b in range(B):
        n = 2 + b
        xy = torch.rand((n, 2), generator=g) * torch.tensor([W - 24.0, H - 24.0]) + 12.0   # centres, content px
        wh = torch.rand((n, 2), generator=g) * 12.0 + 6.0
        boxes = torch.cat([xy, wh], dim=1) / torch.tensor([WP, HP, WP, HP], dtype=torch.float32)
        targets.append({"boxes": boxes, "labels": torch.arange(1, n + 1)})
    return img, pad_targets(targets, M)


def test_spec_token():
    from src.moe.config import parse_moe_spec

    assert parse_moe_spec("rtdetr-r18-moe4-top2-aug").augment is True
    assert parse_moe_spec("rtdetr-r18-moe4-top2").augment is False
    s = parse_moe_spec("rtdetr-r18-moe4-top1-ema")
    assert s.ema_decay == 0.9999 and s.ema_tau == 2000.0 and not s.augment
    s = parse_moe_spec("rtdetr-r50-aug-ema0.999-ematau50")
    assert s.ema_decay == 0.999 and s.ema_tau == 50.0 and s.augment and s.moe is None
    s = parse_moe_spec("rtdetr-r18-moe4-top2-ep2-ematau50-dn100-aug")
    assert s.ema_decay == 0.0 and s.ema_tau == 50.0 and s.moe.ep_size == 2 and s.num_denoising == 100 and s.augment
    with pytest.raises(ValueError):
        parse_moe_spec("rtdetr-r18-augx")


def test_identity_table():
    from src.rtdetr_moe.augment import augment_reference, identity_table
    from src.rtdetr_moe.criterion import PAD_BOX

    img, (tb, tl, nv) = _batch()
    out, ob, ol, onv, total = augment_reference(img, tb, tl, nv, identity_table(3, (H, W)), (H, W))
    want = img.float() / 255.0
    assert out.dtype == torch.float32 and out.shape == img.shape
    torch.testing.assert_close(out[:, :, :H, :W], want[:, :, :H, :W], rtol=0, atol=2 ** -23)
    assert (out[:, :, H:] == 0).all() and (out[:, :, :, W:] == 0).all()
    torch.testing.assert_close(ob, tb, rtol=0, atol=1e-6)
    assert torch.equal(ol, tl) and torch.equal(onv, nv) and float(total) == float(nv.sum())
    assert torch.equal(ob[0, 2:], torch.tensor(PAD_BOX).expand(14, 4))


def test_pure_flip_table():
    from src.rtdetr_moe.augment import augment_reference, make_table

    img, (tb, tl, nv) = _batch()
    B = 3
    table = make_table([1.0] * B, [W / 2] * B, [H / 2] * B, [True] * B, [0.0] * B, [1.0] * B, [1.0] * B, (H, W))
    out, ob, ol, onv, _ = augment_reference(img, tb, tl, nv, table, (H, W))
    want = torch.flip(img[:, :, :H, :W].float() / 255.0, dims=[3])
    assert torch.equal(out[:, :, :H, :W], want)
    assert (out[:, :, H:] == 0).all() and (out[:, :, :, W:] == 0).all()
    assert torch.equal(onv, nv) and torch.equal(ol, tl)
    for b in range(B):
        n = int(nv[b])
        torch.testing.assert_close(ob[b, :n, 0], W / WP - tb[b, :n, 0], rtol=0, atol=1e-6)
        torch.testing.assert_close(ob[b, :n, 1:], tb[b, :n, 1:], rtol=0, atol=1e-6)


def test_box_keep_thresholds():
    """Image 0 halves everything about its centre (the 2 px size test); image 1
    shifts right by 60 px (the area-ratio test and a box fully outside)."""
    from src.rtdetr_moe.augment import augment_reference, make_table
    from src.rtdetr_moe.criterion import PAD_BOX, pad_targets

    h = w = 100
    Hp = Wp = 128

    def norm(x1, y1, x2, y2):
        return [(x1 + x2) / 2 / Wp, (y1 + y2) / 2 / Hp, (x2 - x1) / Wp, (y2 - y1) / Hp]

    img0 = [norm(40, 30, 43, 50),    # 3 px wide -> 1.5 px: dropped
            norm(50, 30, 55, 50),    # 5 px wide -> 2.5 px: kept
            norm(10, 10, 40, 40)]    # kept
    img1 = [norm(37, 30, 97, 70),    # -> x in [97, 157]: 3 of 60 px inside, 95 % out: dropped (area)
            norm(5, 30, 25, 70),     # -> [65, 85]: inside, kept
            norm(45, 30, 65, 70),    # -> [105, 125]: fully outside, dropped
            norm(28, 30, 88, 70)]    # -> [88, 148]: 12 of 60 px inside, 80 % out: kept
    targets = [{"boxes": torch.tensor(img0), "labels": torch.tensor([1, 2, 3])},
               {"boxes": torch.tensor(img1), "labels": torch.tensor([4, 5, 6, 7])}]
    tb, tl, nv = pad_targets(targets, 16)
    table = make_table([0.5, 1.0], [w / 2, w / 2 + 60], [h / 2, h / 2], [False, False], [0.0, 0.0], [1.0, 1.0],
                       [1.0, 1.0], (h, w))
    img = torch.zeros((2, 3, Hp, Wp))
    for dtype in (torch.float32, torch.float64):
        _, ob, ol, onv, total = augment_reference(img, tb, tl, nv, table, (h, w), dtype=dtype)
        assert onv.tolist() == [2, 2] and float(total) == 4.0 and onv.dtype == torch.int32
        assert ol[0].tolist() == [2, 3] + [0] * 14 and ol[1].tolist() == [5, 7] + [0] * 14   # order kept
        pad = torch.tensor(PAD_BOX, dtype=dtype).expand(14, 4)
        assert torch.equal(ob[0, 2:], pad) and torch.equal(ob[1, 2:], pad)
        # image 0: x' = 0.5 x + 25; image 1: x' = x + 60, clipped at 100
        want0 = torch.tensor([norm(50, 40, 52.5, 50), norm(30, 30, 45, 45)], dtype=dtype)
        want1 = torch.tensor([norm(65, 30, 85, 70), norm(88, 30, 100, 70)], dtype=dtype)
        torch.testing.assert_close(ob[0, :2], want0, rtol=0, atol=1e-6)
        torch.testing.assert_close(ob[1, :2], want1, rtol=0, atol=1e-6)


def test_draw_params_ranges_and_seeding():
    from src.rtdetr_moe.augment import AugmentParams, BatchAugment, draw_params

    p = AugmentParams()
    n = 1000
    t = draw_params(torch.Generator().manual_seed(5), n, (H, W), (HP, WP), p).double()
    assert t.shape == (n, 16) and t.dtype == torch.float64
    s = t[:, 15]
    flip = t[:, 0] < 0
    eps = 1e-5
    assert (s >= 1 - p.scale - eps).all() and (s <= 1 + p.scale + eps).all()
    assert torch.allclose(t[:, 0].abs(), s) and torch.allclose(t[:, 4], s)
    assert (t[:, [1, 3, 7, 9]] == 0).all()
    c = torch.where(flip, W - t[:, 2], t[:, 2])          # tx - s w / 2
    tx, ty = (c + s * W / 2) / W, (t[:, 5] + s * H / 2) / H
    for v in (tx, ty):
        assert (v >= 0.5 - p.translate - eps).all() and (v <= 0.5 + p.translate + eps).all()
    assert 0.4 < flip.double().mean() < 0.6
    assert (t[:, 12].abs() <= p.hsv_h + eps).all()
    assert ((t[:, 13] - 1).abs() <= p.hsv_s + eps).all() and ((t[:, 14] - 1).abs() <= p.hsv_v + eps).all()
    assert s.max() - s.min() > 0.9 and t[:, 13].max() - t[:, 13].min() > 1.2   # the ranges are used
    # forward . inverse = identity
    x = t[:, 6] * (t[:, 0] * 7.0 + t[:, 2]) + t[:, 8]
    y = t[:, 10] * (t[:, 4] * 3.0 + t[:, 5]) + t[:, 11]
    assert torch.allclose(x, torch.full_like(x, 7.0), atol=1e-4) and torch.allclose(y, torch.full_like(y, 3.0),
                                                                                      atol=1e-4)
    mk = lambda seed, rank: BatchAugment(4, (H, W), (HP, WP), "cpu", seed=seed, rank=rank)  # noqa: E731
    a, b, c2, d = mk(3, 0), mk(3, 0), mk(3, 1), mk(4, 0)
    ta = [a.draw() for _ in range(2)]
    assert not torch.equal(ta[0], ta[1])
    assert all(torch.equal(x, b.draw()) for x in ta)      # reproducible for a seed
    assert not torch.equal(ta[0], c2.draw()) and not torch.equal(ta[0], d.draw())   # ranks and seeds differ


def test_batch_augment_cpu_matches_reference():
    from src.rtdetr_moe.augment import BatchAugment, augment_reference

    img, (tb, tl, nv) = _batch()
    aug = BatchAugment(3, (H, W), (HP, WP), "cpu", seed=2)
    got = aug(img, tb, tl, nv)
    want = augment_reference(img, tb, tl, nv, aug.table_host, (H, W))
    for g, w_ in zip(got, want):
        assert torch.equal(g, w_)
    assert (got[0][:, :, H:] == 0).all()


def _cpu_step(**kw):
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.data import SyntheticZOD
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.step import TrainStep

    torch.manual_seed(0)
    model = RTDETRMoE(SPEC)
    images, targets, ctx = SyntheticZOD(batch=1, img_h=128, img_w=128, seed=3).sample()
    step = TrainStep(model, SetCriterion(num_classes=1), images, ctx, graphs=False, lr=1e-3, **kw)
    return step, (images, ctx, targets, 2.0)


def test_cpu_train_step():
    step, batch = _cpu_step(augment=True)
    assert step.aug is not None
    losses = [float(step(*batch)) for _ in range(2)]
    assert all(torch.isfinite(torch.tensor(losses))), losses
    off, batch = _cpu_step(augment=False)
    plain, _ = _cpu_step()
    assert off.aug is None and plain.aug is None
    a, b = off(*batch), plain(*batch)
    assert torch.equal(a, b)


def test_datasets_as_uint8(tmp_path):
    """as_uint8 yields the padded uint8 tensor whose x / 255 is the default path's image, targets unchanged."""
    import json

    import numpy as np
    from PIL import Image

    from src.rtdetr_moe.data import CocoDataset, YoloDataset

    rng = np.random.default_rng(0)
    (tmp_path / "images" / "train").mkdir(parents=True)
    (tmp_path / "labels" / "train").mkdir(parents=True)
    Image.fromarray(rng.integers(0, 256, (40, 60, 3), dtype=np.uint8)).save(tmp_path / "images" / "train" / "a.png")
    (tmp_path / "labels" / "train" / "a.txt").write_text("0 0.5 0.5 0.2 0.4\n")
    (tmp_path / "dataset.yaml").write_text(f"path: {tmp_path}\ntrain: images/train\nnames:\n  0: pedestrian\n")
    (tmp_path / "ann.json").write_text(json.dumps({
        "images": [{"id": 1, "file_name": "a.png", "width": 60, "height": 40}], "categories": [{"id": 1}],
        "annotations": [{"id": 1, "image_id": 1, "category_id": 1, "bbox": [10, 10, 20, 20]}]}))
    pairs = [(YoloDataset(tmp_path / "dataset.yaml", imgsz=(40, 60), as_uint8=u) for u in (False, True)),
             (CocoDataset(tmp_path / "images" / "train", tmp_path / "ann.json", imgsz=(40, 60), as_uint8=u)
              for u in (False, True))]
    for plain, u8 in pairs:
        (img, t, c), (img8, t8, c8) = plain[0], u8[0]
        assert img.dtype == torch.float32 and img8.dtype == torch.uint8 and img8.shape == img.shape == (3, 64, 64)
        assert torch.equal(img8.float() / 255.0, img) and int(img8[:, 40:].max()) == 0 and int(img8.max()) > 0
        assert torch.equal(t["boxes"], t8["boxes"]) and torch.equal(t["labels"], t8["labels"]) and c == c8


def test_hsv_jitter_against_colorsys():
    """The colour map against the standard library's RGB <-> HSV: primaries,
    greys, a hue next to the red wrap, saturation and value gains that clamp."""
    import colorsys

    from src.rtdetr_moe.augment import _hsv_jitter

    g = torch.Generator().manual_seed(1)
    px = torch.cat([torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0],
                                  [1.0, 1.0, 1.0], [0.9, 0.1, 0.12], [0.9, 0.12, 0.1], [0.2, 0.7, 0.7]],
                                 dtype=torch.float64),
                    torch.rand((40, 3), generator=g, dtype=torch.float64)])
    for dh, gs, gv in ((0.0, 1.0, 1.0), (0.015, 1.7, 1.4), (-0.015, 0.3, 0.6), (0.4, 1.2, 0.9), (-0.7, 1.0, 2.0)):
        rgb = px.t().reshape(1, 3, 1, -1)
        col = lambda v: torch.full((1, 1, 1), v, dtype=torch.float64)  # noqa: E731
        got = _hsv_jitter(rgb, col(dh), col(gs), col(gv)).reshape(3, -1).t()
        for i, (r, gr, b) in enumerate(px.tolist()):
            h, s, v = colorsys.rgb_to_hsv(r, gr, b)
            want = colorsys.hsv_to_rgb((h + dh) % 1.0, min(1.0, s * gs), min(1.0, v * gv))
            assert max(abs(a - w) for a, w in zip(got[i].tolist(), want)) < 1e-12, (dh, gs, gv, px[i], got[i], want)


def test_batch_augment_takes_a_shorter_batch():
    from src.rtdetr_moe.augment import BatchAugment, augment_reference

    img, (tb, tl, nv) = _batch()
    aug = BatchAugment(3, (H, W), (HP, WP), "cpu", seed=2)
    aug(img, tb, tl, nv)
    got = aug(img[:2], tb[:2], tl[:2], nv[:2])
    assert got[0].shape == (2, 3, HP, WP) and got[1].shape == (2, 16, 4) and aug.table_host.shape == (2, 16)
    want = augment_reference(img[:2], tb[:2], tl[:2], nv[:2], aug.table_host, (H, W))
    for g_, w_ in zip(got, want):
        assert torch.equal(g_, w_)
    with pytest.raises(ValueError):
        aug(torch.cat([img, img[:1]]), tb, tl, nv)


def test_engine_cpu_short_last_batch(tmp_path):
    """engine.train on the CPU keeps an epoch's short last batch (3 images,
    batch 2): with -aug the step must take it like the plain step does."""
    import numpy as np
    from PIL import Image

    from src.rtdetr_moe.engine import TrainArgs, train

    rng = np.random.default_rng(0)
    for split, n in (("train", 3), ("val", 1)):
        (tmp_path / "images" / split).mkdir(parents=True)
        (tmp_path / "labels" / split).mkdir(parents=True)
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (128, 128, 3), dtype=np.uint8)).save(
                tmp_path / "images" / split / f"{i}.png")
            (tmp_path / "labels" / split / f"{i}.txt").write_text("0 0.5 0.5 0.3 0.4\n0 0.25 0.3 0.2 0.2\n")
    (tmp_path / "dataset.yaml").write_text(
        f"path: {tmp_path}\ntrain: images/train\nval: images/val\nnames:\n  0: pedestrian\n")
    res = train(TrainArgs(model=SPEC + "-aug", data=str(tmp_path / "dataset.yaml"), imgsz=128, epochs=1, batch=2,
                          device="cpu", project=str(tmp_path / "runs"), name="aug", workers=0, lr=1e-3))
    assert res is not None and torch.load(res.last, map_location="cpu", weights_only=True)
