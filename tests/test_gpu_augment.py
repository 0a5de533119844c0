"""The augmentation kernels (train_augment_images / train_augment_boxes)
against augment_reference evaluated in float64.

Tolerance: on the same inputs, e32 = max |reference in float32 - reference in
float64|; the kernel may be 4 e32 off (it contracts to fma and orders the four
taps differently), floor 2^-22 (values lie in [0, 1]).  Measured figures:
DESIGN.md, "GPU batch augmentation".

Shapes: B = 3, content 40x60 inside 64x64, M = 16 (one compaction round, a
quarter of the lanes); B = 1, content 32x32 = padded, M = 64 with 64 valid
boxes (a full table); test_boxes_two_rounds adds M = 80, two compaction rounds."""
from __future__ import annotations

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2.0 ** -22
SHAPES = {"pad": dict(B=3, hw=(40, 60), phw=(64, 64), M=16, full=False),
          "full": dict(B=1, hw=(32, 32), phw=(32, 32), M=64, full=True)}
TABLES = ["identity", "flip", "half", "zoom_shift", "rand0", "rand1", "rand2"]
SOURCES = [(torch.uint8, "nchw"), (torch.uint8, "nhwc"), (torch.float32, "nchw"), (torch.float32, "nhwc")]
MARGIN = 1e-3


def _table(name, B, hw):
    from src.rtdetr_moe import augment as A

    h, w = hw
    one, zero, no = [1.0] * B, [0.0] * B, [False] * B
    if name == "identity":
        return A.identity_table(B, hw)
    if name == "flip":
        return A.make_table(one, [w / 2] * B, [h / 2] * B, [True] * B, zero, one, one, hw)
    if name == "half":
        return A.make_table([0.5] * B, [w / 2] * B, [h / 2] * B, no, [0.01] * B, [1.3] * B, [0.8] * B, hw)
    if name == "zoom_shift":  # most taps outside the source
        return A.make_table([1.5] * B, [w * 1.37] * B, [h * 1.21] * B, [b % 2 == 1 for b in range(B)], [-0.012] * B,
                            [0.6] * B, [1.35] * B, hw)
    return A.draw_params(torch.Generator().manual_seed(100 + int(name[-1])), B, hw, hw)


def _keep_margins(terms, n_valid):
    """Distance of every valid slot's keep decision from its thresholds
    (float64 terms): px for the size tests, absolute for the ratios."""
    nw, nh, ref = terms["w"], terms["h"], terms["area_ref"]
    B, M = nw.shape
    valid = torch.arange(M).reshape(1, M) < n_valid.reshape(B, 1)
    big = torch.full_like(nw, 1e9)
    lo, hi = torch.minimum(nw, nh), torch.maximum(nw, nh)
    m = torch.minimum((nw - 2).abs(), (nh - 2).abs())
    m = torch.minimum(m, torch.where(lo > 0, (hi / lo.clamp(min=1e-300) - 100).abs(), big))
    m = torch.minimum(m, torch.where(ref > 0, (nw * nh / ref.clamp(min=1e-300) - 0.1).abs(), big))
    return torch.where(valid, m, big)


def _make_boxes(B, M, counts, hw, phw, table, seed):
    """Random boxes (content px: widths 1..24, centres anywhere in the frame),
    constructed so that every keep decision of the float64 reference clears
    its thresholds by MARGIN: candidates are drawn in a fixed order and the
    first ``counts[b]`` that clear them are taken."""
    from src.rtdetr_moe import augment as A
    from src.rtdetr_moe.criterion import pad_targets

    h, w = hw
    Hp, Wp = phw
    g = torch.Generator().manual_seed(seed)
    n_cand = 4 * M
    xy = torch.rand((B, n_cand, 2), generator=g, dtype=torch.float64) * torch.tensor([w, h], dtype=torch.float64)
    wh = torch.rand((B, n_cand, 2), generator=g, dtype=torch.float64) * 23.0 + 1.0
    cand = (torch.cat([xy, wh], dim=-1) / torch.tensor([Wp, Hp, Wp, Hp], dtype=torch.float64)).float()
    terms = A.box_terms(cand, table, hw, phw, torch.float64)
    ok = _keep_margins(terms, torch.full((B,), n_cand)) >= 2 * MARGIN
    targets = []
    for b in range(B):
        idx = torch.nonzero(ok[b]).flatten()[:counts[b]]
        assert len(idx) == counts[b]
        targets.append({"boxes": cand[b, idx], "labels": torch.randint(1, 80, (counts[b],), generator=g)})
    return pad_targets(targets, M)


@functools.lru_cache(maxsize=None)
def _case(shape, tname):
    """Inputs and references of one (shape, table) case, computed once on the
    CPU and shared (read-only) by the tests."""
    from src.rtdetr_moe import augment as A

    sh = SHAPES[shape]
    B, hw, phw, M = sh["B"], sh["hw"], sh["phw"], sh["M"]
    table = _table(tname, B, hw)
    g = torch.Generator().manual_seed(7)
    u8 = torch.zeros((B, 3, *phw), dtype=torch.uint8)
    u8[:, :, :hw[0], :hw[1]] = torch.randint(0, 256, (B, 3, *hw), generator=g, dtype=torch.uint8)
    srcs = {torch.uint8: u8, torch.float32: u8.float() / 255.0}
    counts = [M] * B if sh["full"] else [M, 0, 5][:B]
    tb, tl, nv = _make_boxes(B, M, counts, hw, phw, table, seed=11)
    c = dict(B=B, hw=hw, phw=phw, M=M, table=table, srcs=srcs, targets=(tb, tl, nv))
    for dt, s in srcs.items():
        r64 = A.reference_images(s, table, hw, dtype=torch.float64)
        r32 = A.reference_images(s, table, hw, dtype=torch.float32)
        c[("img64", dt)] = r64
        c[("img_e32", dt)] = float((r32.double() - r64).abs().max())
    c["box64"] = A.reference_boxes(tb, tl, nv, table, hw, phw, torch.float64)
    b32 = A.reference_boxes(tb, tl, nv, table, hw, phw, torch.float32)
    c["box32"] = b32
    c["box_e32"] = float((b32[0].double() - c["box64"][0]).abs().max())
    c["terms64"] = A.box_terms(tb, table, hw, phw, torch.float64)
    return c


def _src(c, dtype, layout):
    s = c["srcs"][dtype].to(DEV)
    return s.contiguous(memory_format=torch.channels_last) if layout == "nhwc" else s.contiguous()


def _out(c, dtype):
    return torch.empty((c["B"], 3, *c["phw"]), dtype=dtype, device=DEV, memory_format=torch.channels_last)


@pytest.mark.parametrize("tname", TABLES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_images_fp32(hip_lib, shape, tname):
    from src.rtdetr_moe.augment import augment_images_hip

    c = _case(shape, tname)
    table = c["table"].to(DEV)
    for dtype, layout in SOURCES:
        got = augment_images_hip(_src(c, dtype, layout), table, _out(c, torch.float32), c["hw"]).cpu()
        e32 = c[("img_e32", dtype)]
        err = float((got.double() - c[("img64", dtype)]).abs().max())
        bound = max(4 * e32, FLOOR)
        print(f"{shape} {tname} {dtype} {layout}: reference fp32 error {e32:.3e}, kernel error {err:.3e}, "
              f"bound {bound:.3e}")
        assert err <= bound, (shape, tname, dtype, layout, err, bound)


@pytest.mark.parametrize("tname", TABLES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_images_bf16_is_the_fp32_result_rounded_once(hip_lib, shape, tname):
    from src.rtdetr_moe.augment import augment_images_hip

    c = _case(shape, tname)
    table = c["table"].to(DEV)
    for dtype, layout in SOURCES:
        src = _src(c, dtype, layout)
        f32 = augment_images_hip(src, table, _out(c, torch.float32), c["hw"])
        b16 = augment_images_hip(src, table, _out(c, torch.bfloat16), c["hw"])
        assert torch.equal(b16.view(torch.int16), f32.to(torch.bfloat16).view(torch.int16)), (shape, tname, dtype)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_padding_is_zero_and_identity_is_exact(hip_lib, shape):
    from src.rtdetr_moe.augment import augment_images_hip

    h, w = SHAPES[shape]["hw"]
    for tname in TABLES:
        c = _case(shape, tname)
        for dtype, layout in SOURCES[1:3]:
            out = _out(c, torch.float32).fill_(7.0)
            got = augment_images_hip(_src(c, dtype, layout), c["table"].to(DEV), out, c["hw"])
            assert (got[:, :, h:] == 0).all() and (got[:, :, :, w:] == 0).all(), (tname, dtype)
    c = _case(shape, "identity")
    # x / 255 as the loader forms it: the correctly rounded quotient, computed on the host (on the GPU torch
    # multiplies by a rounded 1 / 255, which is an ulp off for some x)
    want = c["srcs"][torch.float32].to(DEV)
    for layout in ("nchw", "nhwc"):
        got = augment_images_hip(_src(c, torch.uint8, layout), c["table"].to(DEV), _out(c, torch.float32), c["hw"])
        assert torch.equal(got, want)
        b16 = augment_images_hip(_src(c, torch.uint8, layout), c["table"].to(DEV), _out(c, torch.bfloat16), c["hw"])
        assert torch.equal(b16, want.to(torch.bfloat16))


def _check_boxes(c, got):
    gb, gl, gnv, gtot = (t.cpu() for t in got)
    rb, rl, rnv, rtot = c["box64"]
    margins = _keep_margins(c["terms64"], c["targets"][2])
    assert float(margins.min()) >= MARGIN, float(margins.min())      # every decision is clear of its thresholds
    assert torch.equal(gnv, rnv) and float(gtot) == float(rtot) and gtot.dtype == torch.float32
    assert torch.equal(gl, rl)                                       # survivor set, order, padding labels
    err = float((gb.double() - rb).abs().max())
    bound = max(4 * c["box_e32"], FLOOR)
    print(f"boxes: kept {rnv.tolist()}, reference fp32 error {c['box_e32']:.3e}, kernel error {err:.3e}, "
          f"bound {bound:.3e}")
    assert err <= bound, (err, bound)
    from src.rtdetr_moe.criterion import PAD_BOX

    for b in range(c["B"]):                                          # the tail is PAD_BOX exactly
        n = int(rnv[b])
        assert torch.equal(gb[b, n:], torch.tensor(PAD_BOX).expand(gb.shape[1] - n, 4))


@pytest.mark.parametrize("tname", TABLES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_boxes(hip_lib, shape, tname):
    from src.rtdetr_moe.augment import augment_boxes_hip

    c = _case(shape, tname)
    tb, tl, nv = (t.to(DEV) for t in c["targets"])
    if tname == "half":
        assert 0 < int(c["box64"][2].sum()) < int(nv.sum())          # some kept, some dropped
    _check_boxes(c, augment_boxes_hip(tb, tl, nv, c["table"].to(DEV), c["hw"], c["phw"]))


def test_boxes_two_rounds(hip_lib):
    """M = 80: two 64-slot rounds, the second partly filled; survivors of the
    second round land behind those of the first."""
    from src.rtdetr_moe import augment as A

    B, hw, phw, M = 2, (40, 60), (64, 64), 80
    table = _table("rand1", B, hw)
    tb, tl, nv = _make_boxes(B, M, [80, 70], hw, phw, table, seed=13)
    c = dict(B=B, targets=(tb, tl, nv), box64=A.reference_boxes(tb, tl, nv, table, hw, phw, torch.float64),
             terms64=A.box_terms(tb, table, hw, phw, torch.float64))
    c["box_e32"] = float((A.reference_boxes(tb, tl, nv, table, hw, phw)[0].double() - c["box64"][0]).abs().max())
    assert 0 < int(c["box64"][2][0]) < 80
    _check_boxes(c, A.augment_boxes_hip(tb.to(DEV), tl.to(DEV), nv.to(DEV), table.to(DEV), hw, phw))


def test_batch_augment_gpu_matches_its_kernels(hip_lib):
    from src.rtdetr_moe import augment as A

    c = _case("pad", "rand0")
    tb, tl, nv = (t.to(DEV) for t in c["targets"])
    aug = A.BatchAugment(c["B"], c["hw"], c["phw"], DEV, seed=9)
    src = _src(c, torch.uint8, "nchw")
    img, ob, ol, onv, total = aug(src, tb, tl, nv)
    assert img.is_contiguous(memory_format=torch.channels_last) and img.dtype == torch.float32
    table = aug.table_host.to(DEV)
    assert torch.equal(aug.table, table)
    assert torch.equal(img, A.augment_images_hip(src, table, _out(c, torch.float32), c["hw"]))
    wb, wl, wnv, wtot = A.augment_boxes_hip(tb, tl, nv, table, c["hw"], c["phw"])
    assert torch.equal(ob, wb) and torch.equal(ol, wl) and torch.equal(onv, wnv) and torch.equal(total, wtot)
    first = aug.table_host.clone()
    aug(src, tb, tl, nv)
    assert not torch.equal(first, aug.table_host)                    # a new draw per call
    # a shorter batch uses the leading rows of the buffers
    img2, ob2, ol2, onv2, total2 = aug(src[:2], tb[:2], tl[:2], nv[:2])
    t2 = aug.table_host.to(DEV)
    assert t2.shape == (2, 16) and img2.shape[0] == 2
    out2 = torch.empty((2, 3, *c["phw"]), dtype=torch.float32, device=DEV, memory_format=torch.channels_last)
    assert torch.equal(img2, A.augment_images_hip(src[:2], t2, out2, c["hw"]))
    wb, wl, wnv, wtot = A.augment_boxes_hip(tb[:2], tl[:2], nv[:2], t2, c["hw"], c["phw"])
    assert torch.equal(ob2, wb) and torch.equal(ol2, wl) and torch.equal(onv2, wnv) and torch.equal(total2, wtot)


def test_argument_checks(hip_lib):
    """Each bad call comes back with a non-zero code (MoEKernelError carries
    it and the moe_last_error message) before any launch."""
    from src.moe import _lib as L
    from src.rtdetr_moe import augment as A

    torch.cuda.synchronize()
    L.launch_counts(reset=True)
    hw = (40, 60)
    table = A.identity_table(1, hw).to(DEV)
    src = torch.zeros((1, 3, 64, 62), dtype=torch.uint8, device=DEV)
    out = torch.empty((1, 3, 64, 62), dtype=torch.float32, device=DEV, memory_format=torch.channels_last)
    with pytest.raises(L.MoEKernelError, match=r"rc=-1.*multiple of 4"):
        A.augment_images_hip(src, table, out, hw)
    src = torch.zeros((1, 3, 64, 64), dtype=torch.uint8, device=DEV)
    flat = torch.empty(64 * 64 * 3 + 4, dtype=torch.float32, device=DEV)
    out = flat[1:1 + 64 * 64 * 3].view(1, 64, 64, 3).permute(0, 3, 1, 2)   # channels_last, 4 B off alignment
    assert out.is_contiguous(memory_format=torch.channels_last) and out.data_ptr() % 16 == 4
    with pytest.raises(L.MoEKernelError, match=r"rc=-1.*16-B aligned"):
        A.augment_images_hip(src, table, out, hw)
    M = 2048
    tb = torch.zeros((1, M, 4), device=DEV)
    tl = torch.zeros((1, M), dtype=torch.int64, device=DEV)
    nv = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(L.MoEKernelError, match=r"rc=-1.*1\.\.1024"):
        A.augment_boxes_hip(tb, tl, nv, table, hw, (64, 64))
    good = torch.empty((1, 3, 64, 64), dtype=torch.float32, device=DEV, memory_format=torch.channels_last)
    with pytest.raises(L.MoEKernelError, match="GPU tensor"):
        A.augment_images_hip(src.cpu(), table, good, hw)
    with pytest.raises(L.MoEKernelError, match="GPU tensor"):
        A.augment_boxes_hip(tb[:, :16].cpu(), tl[:, :16].cpu(), nv.cpu(), table, hw, (64, 64))
    assert "augment" not in L.launch_counts()
    A.augment_images_hip(src, table, good, hw)
    assert L.launch_counts(reset=True).get("augment") == 1
