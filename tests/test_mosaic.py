"""Mosaic augmentation on the CPU: the -mosaic spec token, mosaic_reference
against a canvas built literally as Ultralytics' _mosaic4 builds it, an exact
known answer, the degenerate rows against augment_reference, the random stream,
the box order / bound / overflow clamp, and close_mosaic in engine.train."""
from __future__ import annotations

import math
from pathlib import Path

import pytest
import torch

SPEC = "rtdetr-r18-moe4-top1-dec1"
FIX = Path(__file__).resolve().parent / "golden" / "zod_mini"
FILL = 114.0 / 255.0


def test_spec_token():
    from src.moe.config import parse_moe_spec

    s = parse_moe_spec("rtdetr-r18-moe4-top2-mosaic")
    assert s.mosaic == 1.0 and s.augment is True and s.moe.num_experts == 4
    s = parse_moe_spec("rtdetr-r18-moe4-top2-mosaic0.5")
    assert s.mosaic == 0.5 and s.augment is True
    s = parse_moe_spec("rtdetr-r50-mosaic0.25-ema-dn100-ep2")
    assert s.mosaic == 0.25 and s.augment and s.ema_decay == 0.9999 and s.num_denoising == 100 and s.moe.ep_size == 2
    s = parse_moe_spec("rtdetr-r18-moe8-top2-aug-mosaic")
    assert s.mosaic == 1.0 and s.augment and s.moe.num_experts == 8
    s = parse_moe_spec("rtdetr-r18-moe4-top2-aug")
    assert s.mosaic == 0.0 and s.augment
    assert parse_moe_spec("rtdetr-r18-moe4-top2").mosaic == 0.0
    for bad in ("rtdetr-r18-mosaic1.5", "rtdetr-r18-mosaicx", "rtdetr-r18-mosaicnan"):
        with pytest.raises(ValueError):
            parse_moe_spec(bad)


# ---------------------------------------------------------------------------
# images against a literal _mosaic4 canvas
# ---------------------------------------------------------------------------
def _images(B, hw, phw, seed=3):
    g = torch.Generator().manual_seed(seed)
    img = torch.zeros((B, 3, *phw), dtype=torch.uint8)
    img[:, :, :hw[0], :hw[1]] = torch.randint(0, 256, (B, 3, *hw), generator=g, dtype=torch.uint8)
    return img


def _tables(B, hw):
    """{name: [B, 24]}: three random draws (one of them with mosaic on half the
    rows), s = 0.5 with an extreme centre, a flipped one."""
    from src.rtdetr_moe import augment as A

    h, w = hw
    out = {}
    for i, p in enumerate((1.0, 1.0, 0.5)):
        out[f"rand{i}"] = A.draw_mosaic_params(torch.Generator().manual_seed(40 + i), B, hw, hw, p)
    on, one, zero = [True] * B, [1.0] * B, [0.0] * B
    partners = [[(n + 1) % B, (n + 2) % B, (n + 3) % B] for n in range(B)]
    out["half_extreme"] = A.make_mosaic_table([0.5] * B, [w / 2] * B, [h / 2] * B, [False] * B, [0.01] * B, [1.3] * B,
                                              [0.8] * B, hw, on, [w // 2] * B, [3 * h // 2 - 1] * B, partners)
    out["flip"] = A.make_mosaic_table([0.8] * B, [w * 0.45] * B, [h * 0.56] * B, on, zero, one, one, hw, on,
                                      [w - 2] * B, [h + 1] * B, partners)
    return out


def _literal_canvas(src, row, hw):
    """_mosaic4's four slice assignments for one table row: (canvas [3,2h,2w]
    float64, mask [2h,2w]); src [B,3,h,w] float64."""
    h, w = hw
    xc, yc = int(row[16]), int(row[17])
    canvas = torch.full((3, 2 * h, 2 * w), FILL, dtype=torch.float64)
    mask = torch.zeros((2 * h, 2 * w), dtype=torch.bool)
    for i in range(4):
        idx = int(row[18 + i])
        if idx < 0:
            continue
        if i == 0:    # top left
            x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
            x1b, y1b, x2b, y2b = w - (x2a - x1a), h - (y2a - y1a), w, h
        elif i == 1:  # top right
            x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, 2 * w), yc
            x1b, y1b, x2b, y2b = 0, h - (y2a - y1a), min(w, x2a - x1a), h
        elif i == 2:  # bottom left
            x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(2 * h, yc + h)
            x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, w, min(y2a - y1a, h)
        else:         # bottom right
            x1a, y1a, x2a, y2a = xc, yc, min(xc + w, 2 * w), min(2 * h, yc + h)
            x1b, y1b, x2b, y2b = 0, 0, min(w, x2a - x1a), min(y2a - y1a, h)
        canvas[:, y1a:y2a, x1a:x2a] = src[idx, :, y1b:y2b, x1b:x2b]
        mask[y1a:y2a, x1a:x2a] = True
    return canvas, mask


def _literal_images(images, table, hw):
    """The semantics by a plain loop, float64: canvas, inverse map, four taps,
    colour, the no-valid-tap rule, zero padding."""
    from src.rtdetr_moe.augment import _hsv_jitter

    h, w = hw
    B = table.shape[0]
    src = images[:, :, :h, :w].double() / 255.0
    t = table.double()
    out = torch.zeros((B, 3, *images.shape[-2:]), dtype=torch.float64)
    for n in range(B):
        canvas, mask = _literal_canvas(src, table[n].tolist(), hw)
        r = t[n].tolist()
        val = torch.zeros((3, h, w), dtype=torch.float64)
        some = torch.zeros((h, w), dtype=torch.bool)
        for y in range(h):
            for x in range(w):
                u = (r[6] * (x + 0.5) + r[7] * (y + 0.5)) + r[8]
                v = (r[9] * (x + 0.5) + r[10] * (y + 0.5)) + r[11]
                fx, fy = u - 0.5, v - 0.5
                X0, Y0 = math.floor(fx), math.floor(fy)
                ax, ay = fx - X0, fy - Y0
                acc = torch.zeros(3, dtype=torch.float64)
                for dy, dx, wt in ((0, 0, (1 - ax) * (1 - ay)), (0, 1, ax * (1 - ay)), (1, 0, (1 - ax) * ay),
                                   (1, 1, ax * ay)):
                    X, Y = X0 + dx, Y0 + dy
                    if 0 <= X < 2 * w and 0 <= Y < 2 * h and bool(mask[Y, X]):
                        acc = acc + canvas[:, Y, X] * wt
                        some[y, x] = True
                    else:
                        acc = acc + FILL * wt
                val[:, y, x] = acc
        if not (r[12] == 0 and r[13] == 1 and r[14] == 1):
            col = lambda i: torch.full((1, 1, 1), r[i], dtype=torch.float64)  # noqa: E731
            val = _hsv_jitter(val.unsqueeze(0), col(12), col(13), col(14))[0]
        out[n, :, :h, :w] = torch.where(some.unsqueeze(0), val, torch.full((), FILL, dtype=torch.float64))
    return out


@pytest.mark.parametrize("phw", [(8, 12), (16, 16)])
def test_reference_images_against_literal_canvas(phw):
    from src.rtdetr_moe.augment import mosaic_reference_images

    B, hw = 4, (8, 12)
    images = _images(B, hw, phw)
    for name, table in _tables(B, hw).items():
        got = mosaic_reference_images(images, table, hw, dtype=torch.float64)
        want = _literal_images(images, table, hw)
        err = float((got - want).abs().max())
        assert err <= 1e-12, (name, phw, err)
        assert (got[:, :, hw[0]:] == 0).all() and (got[:, :, :, hw[1]:] == 0).all()
        if name != "rand2":
            assert (table[:, 19:22] >= 0).all()
    t = _tables(B, hw)["rand2"]
    assert (t[:, 19] < 0).any() and (t[:, 19] >= 0).any()          # degenerate and mosaic rows in one table


def test_exact_quarters():
    """s = 1, the canvas centre to the image centre, the mosaic centre at the
    canvas centre, no colour: each output quarter is the opposite quarter of
    its quadrant's source, bit for bit (uint8 and float sources, fp32 and fp64)."""
    from src.rtdetr_moe import augment as A

    B, hw = 4, (8, 12)
    h, w = hw
    images = _images(B, hw, (16, 16))
    partners = [[(n + 1) % B, (n + 2) % B, (n + 3) % B] for n in range(B)]
    table = A.make_mosaic_table([1.0] * B, [w / 2] * B, [h / 2] * B, [False] * B, [0.0] * B, [1.0] * B, [1.0] * B, hw,
                                [True] * B, [w] * B, [h] * B, partners)
    for dtype in (torch.float32, torch.float64):
        for src in (images, images.to(dtype) / 255.0):
            out = A.mosaic_reference_images(src, table, hw, dtype=dtype)
            ref = images[:, :, :h, :w].to(dtype) / 255.0
            for n in range(B):
                tl, (tr, bl, br) = n, partners[n]
                assert torch.equal(out[n, :, :h // 2, :w // 2], ref[tl, :, h // 2:, w // 2:])
                assert torch.equal(out[n, :, :h // 2, w // 2:w], ref[tr, :, h // 2:, :w // 2])
                assert torch.equal(out[n, :, h // 2:h, :w // 2], ref[bl, :, :h // 2, w // 2:])
                assert torch.equal(out[n, :, h // 2:h, w // 2:w], ref[br, :, :h // 2, :w // 2])


# ---------------------------------------------------------------------------
# degenerate rows, the random stream
# ---------------------------------------------------------------------------
def _batch(B=3, M=16, hw=(40, 60), phw=(64, 64), seed=0, counts=None):
    """Images and padded targets with every box inside the content rectangle;
    the label of slot j of image b is 100 b + j + 1."""
    from src.rtdetr_moe.criterion import pad_targets

    h, w = hw
    g = torch.Generator().manual_seed(seed)
    targets = []
    for b in range(B):
        n = 2 + b if counts is None else counts[b]
        xy = torch.rand((n, 2), generator=g) * torch.tensor([w - 24.0, h - 24.0]) + 12.0   # centres, content px
        wh = torch.rand((n, 2), generator=g) * 8.0 + 8.0
        boxes = torch.cat([xy, wh], dim=1) / torch.tensor([phw[1], phw[0], phw[1], phw[0]], dtype=torch.float32)
        targets.append({"boxes": boxes, "labels": 100 * b + torch.arange(1, n + 1)})
    return _images(B, hw, phw, seed + 1), pad_targets(targets, M)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_degenerate_rows_are_the_plain_augmentation(dtype):
    from src.rtdetr_moe import augment as A

    hw = (40, 60)
    img, (tb, tl, nv) = _batch()
    terms = A._draw_terms(torch.Generator().manual_seed(5), 3, hw, (64, 64), A.AugmentParams())
    plain, deg = A.make_table(*terms, hw), A.make_mosaic_table(*terms, hw)
    assert torch.equal(deg[:, :16], plain)
    assert torch.equal(deg[:, 16:], torch.tensor([[60.0, 40.0, n, -1, -1, -1, 0, 0] for n in range(3)]))
    want = A.augment_reference(img, tb, tl, nv, plain, hw, dtype=dtype)
    got = A.mosaic_reference(img, tb, tl, nv, deg, hw, dtype=dtype)
    assert 0 < int(want[3].sum())
    for g_, w_ in zip(got, want):
        assert g_.dtype == w_.dtype and torch.equal(g_, w_)


def test_random_stream():
    from src.rtdetr_moe import augment as A

    B, hw, phw = 4, (40, 60), (64, 64)
    # mosaic = 0: the plain object, the plain draws
    aug, g = A.BatchAugment(B, hw, phw, "cpu", seed=3, mosaic=0.0), torch.Generator().manual_seed(3000)
    assert not aug.mosaic_path
    for _ in range(3):
        assert torch.equal(aug.draw(), A.draw_params(g, B, hw, phw))
    # mosaic on: the seven uniforms keep their place, the mosaic ones follow in a call of their own
    aug, g = A.BatchAugment(B, hw, phw, "cpu", seed=3, mosaic=1.0), torch.Generator().manual_seed(3000)
    p = A.AugmentParams()
    for _ in range(2):
        t = aug.draw()
        u = torch.rand((B, 7), generator=g, dtype=torch.float64)
        um = torch.rand((B, 6), generator=g, dtype=torch.float64)
        s = 1.0 + (2 * u[:, 0] - 1) * p.scale
        tx, ty = (0.5 + (2 * u[:, 1] - 1) * p.translate) * hw[1], (0.5 + (2 * u[:, 2] - 1) * p.translate) * hw[0]
        flip = u[:, 3] < p.fliplr
        plain = A.make_table(s, tx, ty, flip, (2 * u[:, 4] - 1) * p.hsv_h, 1 + (2 * u[:, 5] - 1) * p.hsv_s,
                             1 + (2 * u[:, 6] - 1) * p.hsv_v, hw, centre=(hw[1], hw[0]))
        assert t.shape == (B, A.MOSAIC_COLS) and torch.equal(t[:, :16], plain)
        assert torch.equal(t[:, 12:16], A.make_table(s, tx, ty, flip, (2 * u[:, 4] - 1) * p.hsv_h,
                                                     1 + (2 * u[:, 5] - 1) * p.hsv_s,
                                                     1 + (2 * u[:, 6] - 1) * p.hsv_v, hw)[:, 12:16])
        # forward matrix: x' = a x + c with the canvas centre (w, h) sent to (tx, ty)
        a, c = t[:, 0].double(), t[:, 2].double()
        assert torch.allclose(a * hw[1] + c, torch.where(flip, hw[1] - tx, tx), atol=1e-4)
        assert torch.equal(t[:, 16].double(), torch.floor(hw[1] / 2 + um[:, 1] * hw[1]))
        assert torch.equal(t[:, 17].double(), torch.floor(hw[0] / 2 + um[:, 2] * hw[0]))
        assert torch.equal(t[:, 18].double(), torch.arange(B, dtype=torch.float64))
        assert torch.equal(t[:, 19:22].double(), torch.floor(um[:, 3:6] * B))
        assert (t[:, 16] >= hw[1] / 2).all() and (t[:, 16] < 3 * hw[1] / 2).all() and (t[:, 22:] == 0).all()
    # set to 0 later: degenerate rows of the same width, and no second call
    aug.mosaic = 0.0
    t = aug.draw()
    assert torch.equal(t[:, :16], A.draw_params(g, B, hw, phw)) and (t[:, 19:22] == -1).all()
    assert torch.equal(aug.draw()[:, :16], A.draw_params(g, B, hw, phw))
    with pytest.raises(ValueError):
        aug.mosaic = 1.5


# ---------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------
def _whole_canvas_table(B, hw, partners):
    """s = 0.5 about the canvas centre: the output shows the whole canvas, every box at half size."""
    from src.rtdetr_moe import augment as A

    h, w = hw
    return A.make_mosaic_table([0.5] * B, [w / 2] * B, [h / 2] * B, [False] * B, [0.0] * B, [1.0] * B, [1.0] * B, hw,
                               [True] * B, [w] * B, [h] * B, partners)


def test_box_order_bound_and_overflow():
    from src.rtdetr_moe import augment as A
    from src.rtdetr_moe.criterion import PAD_BOX

    B, hw, phw, M = 4, (40, 60), (64, 64), 16
    counts = [5, 0, 3, 7]
    img, (tb, tl, nv) = _batch(B, M, hw, phw, seed=2, counts=counts)
    partners = [[2, 3, 0], [1, 1, 1], [3, 3, 2], [0, 2, 2]]
    table = _whole_canvas_table(B, hw, partners)
    aug = A.BatchAugment(B, hw, phw, "cpu", mosaic=1.0)
    need = aug.need(counts, table)
    assert need == max(counts[n] + sum(counts[p] for p in partners[n]) for n in range(B)) == 20
    ob, ol, onv, total = A.mosaic_reference_boxes(tb, tl, nv, table, hw, phw, M_out=32)
    assert ob.shape == (B, 32, 4) and ol.shape == (B, 32)
    for n in range(B):   # boxes of 8..16 px at half size all survive: quadrant-major, slots in order
        want = [100 * s + j + 1 for s in [n] + partners[n] for j in range(counts[s])]
        assert int(onv[n]) == len(want) <= need
        assert ol[n, :len(want)].tolist() == want and (ol[n, len(want):] == 0).all()
        assert torch.equal(ob[n, len(want):], torch.tensor(PAD_BOX).expand(32 - len(want), 4))
    assert float(total) == float(onv.sum())
    # a top-left box lands at half size in the top-left quarter of the output
    x = (tb[0, 0] * torch.tensor([64.0, 64.0, 64.0, 64.0]))
    assert torch.allclose(ob[0, 0] * 64.0, x * 0.5, atol=1e-4)
    # the top-right partner's first box: shifted by (xc, yc - h) = (w, 0) on the canvas
    src = partners[0][0]
    x = tb[src, 0] * 64.0
    assert torch.allclose(ob[0, counts[0]] * 64.0, torch.stack([(x[0] + 60) * 0.5, x[1] * 0.5, x[2] * 0.5, x[3] * 0.5]),
                          atol=1e-4)
    # overflow: the first M_out survivors, the count clamped
    sb, sl, snv, stot = A.mosaic_reference_boxes(tb, tl, nv, table, hw, phw, M_out=6)
    for n in range(B):
        k = min(int(onv[n]), 6)
        assert int(snv[n]) == k and torch.equal(sl[n, :k], ol[n, :k]) and torch.equal(sb[n, :k], ob[n, :k])
    assert float(stot) == float(snv.sum()) and sb.shape == (B, 6, 4)
    # boxes cut by the canvas edge refer to their clipped area: a centre at the far corner cuts every quadrant
    far = A.make_mosaic_table([1.0] * B, [30.0] * B, [20.0] * B, [False] * B, [0.0] * B, [1.0] * B, [1.0] * B, hw,
                              [True] * B, [89] * B, [59] * B, partners)
    terms, occupied, quad = A.mosaic_box_terms(tb, nv, far, hw, phw, torch.float64)
    assert quad.tolist() == [[n] + partners[n] for n in range(B)]
    assert int(occupied.sum()) == sum(counts[s] for n in range(B) for s in [n] + partners[n])
    assert (terms["area_ref"][occupied] >= 0).all() and (terms["area_ref"][occupied] == 0).any()


def test_batch_augment_cpu_mosaic_matches_reference():
    from src.rtdetr_moe import augment as A

    B, hw, phw, M = 3, (40, 60), (64, 64), 16
    img, (tb, tl, nv) = _batch(B, M, hw, phw)
    aug = A.BatchAugment(B, hw, phw, "cpu", seed=2, mosaic=1.0)
    assert aug.mosaic_path and aug.table.shape == (B, A.MOSAIC_COLS)
    got = aug(img, tb, tl, nv, M_out=32)
    assert aug.need(nv.tolist()) <= 32
    want = A.mosaic_reference(img, tb, tl, nv, aug.table_host, hw, 32)
    for g_, w_ in zip(got, want):
        assert torch.equal(g_, w_)
    assert got[1].shape == (B, 32, 4) and (aug.table_host[:, 19:22] >= 0).all()
    with pytest.raises(ValueError):
        A.BatchAugment(B, hw, phw, "cpu")(img, tb, tl, nv, M_out=32)     # the plain path has no M_out


# ---------------------------------------------------------------------------
# the engine: close_mosaic
# ---------------------------------------------------------------------------
def test_close_mosaic_in_cpu_training(tmp_path, monkeypatch):
    """Two epochs over the four training frames of tests/golden/zod_mini
    (batch 2) with -aug-mosaic and close_mosaic = 1: mosaic rows in epoch 0,
    only degenerate rows of the same [b, 24] table in epoch 1, finite losses."""
    from src.rtdetr_moe import augment as A
    from src.rtdetr_moe import step as S
    from src.rtdetr_moe.engine import TrainArgs, train

    tables, losses = [], []
    real_call, real_step = A.BatchAugment.__call__, S.TrainStep.__call__

    def call(self, *a, **kw):
        out = real_call(self, *a, **kw)
        tables.append(self.table_host.clone())
        return out

    def step(self, *a, **kw):
        loss = real_step(self, *a, **kw)
        losses.append(float(loss))
        return loss

    monkeypatch.setattr(A.BatchAugment, "__call__", call)
    monkeypatch.setattr(S.TrainStep, "__call__", step)
    res = train(TrainArgs(model=SPEC + "-aug-mosaic", data=str(FIX / "dataset.yaml"), imgsz=128, epochs=2, batch=2,
                          device="cpu", project=str(tmp_path / "runs"), name="mosaic", workers=0, lr=1e-3,
                          close_mosaic=1))
    assert res is not None and res.epochs_run == 2
    assert len(tables) == 4 and len(losses) == 4 and all(math.isfinite(v) for v in losses), losses
    for t in tables:
        assert t.shape == (2, A.MOSAIC_COLS)
    for t in tables[:2]:
        assert (t[:, 19:22] >= 0).all()
    for t in tables[2:]:
        assert (t[:, 19:22] == -1).all() and (t[:, 16] == 128).all() and (t[:, 17] == 128).all()
