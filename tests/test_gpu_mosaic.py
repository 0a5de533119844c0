"""The mosaic kernels (train_mosaic_images / train_mosaic_boxes) against
mosaic_reference evaluated in float64.

Tolerance (tests/test_gpu_augment.py's): on the same inputs, e32 = max
|reference in float32 - reference in float64|; the kernel may be 4 e32 off (it
contracts to fma and orders the four taps differently), floor 2^-22 (values lie
in [0, 1]).  Measured figures: DESIGN.md, "GPU mosaic augmentation".

The rule "a pixel with no valid tap is exactly fill and gets no colour" is
discontinuous where the set of valid taps changes, so every case asserts on the
CPU, when it is built, that in float64 no output pixel's canvas coordinate lies
within 1e-4 px of an integer at which that set changes (the exact-quarters
table, whose coordinates are exact, aside); the seeds were picked for it.

Shapes: B = 4, content 40x60 inside 64x64, M_in 16 -> M_out 64, counts
[16, 0, 5, 9]; B = 1, content 32x32 = padded (every partner is the image
itself), M_in = M_out = 64 with 16 valid; test_boxes_two_rounds adds M_in = 80
(70 valid in one source: two rounds per quadrant) -> M_out 128 with more than
64 survivors; test_boxes_overflow M_out = 16 with more than 16."""
from __future__ import annotations

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2.0 ** -22
SHAPES = {"pad": dict(B=4, hw=(40, 60), phw=(64, 64), M_in=16, M_out=64, counts=[16, 0, 5, 9]),
          "self": dict(B=1, hw=(32, 32), phw=(32, 32), M_in=64, M_out=64, counts=[16])}
TABLES = ["quarters", "degenerate", "half", "rand0", "rand1", "rand2"]
SEEDS = {"rand0": 200, "rand1": 201, "rand2": 202}
SOURCES = [(torch.uint8, "nchw"), (torch.uint8, "nhwc"), (torch.float32, "nchw"), (torch.float32, "nhwc")]
MARGIN = 1e-3
EDGE = 1e-4


def _partners(B):
    return [[(n + 1) % B, (n + 2) % B, (n + 3) % B] for n in range(B)]


def _table(name, B, hw):
    from src.rtdetr_moe import augment as A

    h, w = hw
    one, zero, no, on = [1.0] * B, [0.0] * B, [False] * B, [True] * B
    if name == "quarters":    # each output quarter is the opposite quarter of its quadrant's source
        return A.make_mosaic_table(one, [w / 2] * B, [h / 2] * B, no, zero, one, one, hw, on, [w] * B, [h] * B,
                                   _partners(B))
    if name == "degenerate":  # the plain augmentation, through the mosaic kernels
        return A.make_mosaic_table(*A._draw_terms(torch.Generator().manual_seed(100), B, hw, hw, A.AugmentParams()),
                                   hw)
    if name == "half":        # the whole canvas, the grey bands around it and the outside of the canvas
        return A.make_mosaic_table([0.5] * B, [w / 2] * B, [h / 2] * B, on, [0.01] * B, [1.3] * B, [0.8] * B, hw, on,
                                   [w // 2] * B, [3 * h // 2 - 1] * B, _partners(B))
    return A.draw_mosaic_params(torch.Generator().manual_seed(SEEDS[name]), B, hw, hw, 1.0)


def _valid_mask(table, hw, B_src):
    """[B, 2h + 4, 2w + 4] bool: which canvas pixels hold an image pixel (the
    tap rule, restated), with a border of two invalid pixels all around."""
    h, w = hw
    B = table.shape[0]
    Y = torch.arange(-2, 2 * h + 2).reshape(1, -1, 1)
    X = torch.arange(-2, 2 * w + 2).reshape(1, 1, -1)
    xc, yc = table[:, 16].long().reshape(B, 1, 1), table[:, 17].long().reshape(B, 1, 1)
    q = table[:, 18:22].long()
    q = [torch.where((q[:, i] >= 0) & (q[:, i] < B_src), q[:, i], -1).reshape(B, 1, 1) for i in range(4)]
    right, bottom = X >= xc, Y >= yc
    sx, sy = X - torch.where(right, xc, xc - w), Y - torch.where(bottom, yc, yc - h)
    idx = torch.where(bottom, torch.where(right, q[3], q[2]), torch.where(right, q[1], q[0]))
    return (X >= 0) & (X < 2 * w) & (Y >= 0) & (Y < 2 * h) & (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h) & (idx >= 0)


def _edge_distance(table, hw, B_src):
    """The least distance (px, float64) of an output pixel's canvas coordinate
    from an integer at which its set of valid taps changes: crossing the
    integer k in x swaps the tap column k - 1 for k + 1 (rows likewise)."""
    h, w = hw
    B = table.shape[0]
    t = table.double()
    col = lambda i: t[:, i].reshape(B, 1, 1)  # noqa: E731
    xs = (torch.arange(w, dtype=torch.float64) + 0.5).reshape(1, 1, w)
    ys = (torch.arange(h, dtype=torch.float64) + 0.5).reshape(1, h, 1)
    fx = ((col(6) * xs + col(7) * ys) + col(8) - 0.5).expand(B, h, w)
    fy = ((col(9) * xs + col(10) * ys) + col(11) - 0.5).expand(B, h, w)
    mask = _valid_mask(table, hw, B_src)
    n = torch.arange(B).reshape(B, 1, 1).expand(B, h, w)

    def at(X, Y):   # validity of canvas pixel (X, Y), anything far outside is invalid
        ok = (X >= -2) & (X < 2 * w + 2) & (Y >= -2) & (Y < 2 * h + 2)
        return mask[n, (Y + 2).clamp(0, 2 * h + 3), (X + 2).clamp(0, 2 * w + 3)] & ok

    best = torch.full((B, h, w), 1.0, dtype=torch.float64)
    for f, g, swap in ((fx, fy, False), (fy, fx, True)):
        k, lo = torch.round(f).long(), torch.floor(g).long()
        changes = torch.zeros((B, h, w), dtype=torch.bool)
        for d in (0, 1):
            a = at(lo + d, k - 1) if swap else at(k - 1, lo + d)
            b = at(lo + d, k + 1) if swap else at(k + 1, lo + d)
            changes |= a != b
        best = torch.minimum(best, torch.where(changes, (f - k).abs(), torch.ones_like(f)))
    return float(best.min())


def _keep_margins(terms, occupied):
    """Distance of every occupied slot's keep decision from its thresholds
    (float64 terms): px for the size tests, absolute for the ratios."""
    nw, nh, ref = terms["w"], terms["h"], terms["area_ref"]
    big = torch.full_like(nw, 1e9)
    lo, hi = torch.minimum(nw, nh), torch.maximum(nw, nh)
    m = torch.minimum((nw - 2).abs(), (nh - 2).abs())
    m = torch.minimum(m, torch.where(lo > 0, (hi / lo.clamp(min=1e-300) - 100).abs(), big))
    m = torch.minimum(m, torch.where(ref > 0, (nw * nh / ref.clamp(min=1e-300) - 0.1).abs(), big))
    return torch.where(occupied, m, big)


def _make_boxes(B, M, counts, hw, phw, table, seed):
    """Random boxes (content px: widths 1..24, centres anywhere in the frame),
    as tests/test_gpu_augment.py builds them: candidates are drawn in a fixed
    order and a source image takes the first ``counts[b]`` whose keep decision
    clears its thresholds by MARGIN in EVERY quadrant of every output image
    that uses it (float64)."""
    from src.rtdetr_moe import augment as A
    from src.rtdetr_moe.criterion import pad_targets

    h, w = hw
    Hp, Wp = phw
    g = torch.Generator().manual_seed(seed)
    n_cand = 4 * M
    xy = torch.rand((B, n_cand, 2), generator=g, dtype=torch.float64) * torch.tensor([w, h], dtype=torch.float64)
    wh = torch.rand((B, n_cand, 2), generator=g, dtype=torch.float64) * 23.0 + 1.0
    cand = (torch.cat([xy, wh], dim=-1) / torch.tensor([Wp, Hp, Wp, Hp], dtype=torch.float64)).float()
    full = torch.full((B,), n_cand, dtype=torch.int32)
    terms, occupied, quad = A.mosaic_box_terms(cand, full, table, hw, phw, torch.float64)
    clear = (_keep_margins(terms, occupied) >= 2 * MARGIN).reshape(B, 4, n_cand)
    targets = []
    for b in range(B):
        ok = torch.ones(n_cand, dtype=torch.bool)
        for n in range(B):
            for q in range(4):
                if int(quad[n, q]) == b:
                    ok &= clear[n, q]
        idx = torch.nonzero(ok).flatten()[:counts[b]]
        assert len(idx) == counts[b]
        targets.append({"boxes": cand[b, idx], "labels": torch.randint(1, 80, (counts[b],), generator=g)})
    return pad_targets(targets, M)


def _box_refs(c, tb, tl, nv, table, hw, phw, M_out):
    from src.rtdetr_moe import augment as A

    c["box64"] = A.mosaic_reference_boxes(tb, tl, nv, table, hw, phw, M_out, torch.float64)
    b32 = A.mosaic_reference_boxes(tb, tl, nv, table, hw, phw, M_out, torch.float32)
    c["box_e32"] = float((b32[0].double() - c["box64"][0]).abs().max())
    terms, occupied, _ = A.mosaic_box_terms(tb, nv, table, hw, phw, torch.float64)
    c["margin"] = float(_keep_margins(terms, occupied).min())
    return c


@functools.lru_cache(maxsize=None)
def _case(shape, tname):
    """Inputs and references of one (shape, table) case, computed once on the
    CPU and shared (read-only) by the tests."""
    from src.rtdetr_moe import augment as A

    sh = SHAPES[shape]
    B, hw, phw, M_in, M_out = sh["B"], sh["hw"], sh["phw"], sh["M_in"], sh["M_out"]
    table = _table(tname, B, hw)
    if tname != "quarters":
        d = _edge_distance(table, hw, B)
        assert d >= EDGE, (shape, tname, d)
    g = torch.Generator().manual_seed(7)
    u8 = torch.zeros((B, 3, *phw), dtype=torch.uint8)
    u8[:, :, :hw[0], :hw[1]] = torch.randint(0, 256, (B, 3, *hw), generator=g, dtype=torch.uint8)
    srcs = {torch.uint8: u8, torch.float32: u8.float() / 255.0}
    tb, tl, nv = _make_boxes(B, M_in, sh["counts"], hw, phw, table, seed=11)
    c = dict(B=B, hw=hw, phw=phw, M_in=M_in, M_out=M_out, table=table, srcs=srcs, targets=(tb, tl, nv))
    for dt, s in srcs.items():
        r64 = A.mosaic_reference_images(s, table, hw, dtype=torch.float64)
        r32 = A.mosaic_reference_images(s, table, hw, dtype=torch.float32)
        c[("img64", dt)] = r64
        c[("img_e32", dt)] = float((r32.double() - r64).abs().max())
    return _box_refs(c, tb, tl, nv, table, hw, phw, M_out)


def _src(c, dtype, layout):
    s = c["srcs"][dtype].to(DEV)
    return s.contiguous(memory_format=torch.channels_last) if layout == "nhwc" else s.contiguous()


def _out(c, dtype):
    return torch.empty((c["B"], 3, *c["phw"]), dtype=dtype, device=DEV, memory_format=torch.channels_last)


@pytest.mark.parametrize("tname", TABLES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_images(hip_lib, shape, tname):
    """fp32 destination within the bound of the float64 reference; the bf16
    destination is that result rounded once; padding is exactly 0."""
    from src.rtdetr_moe.augment import mosaic_images_hip

    c = _case(shape, tname)
    h, w = c["hw"]
    table = c["table"].to(DEV)
    for dtype, layout in SOURCES:
        src = _src(c, dtype, layout)
        f32 = mosaic_images_hip(src, table, _out(c, torch.float32).fill_(7.0), c["hw"])
        b16 = mosaic_images_hip(src, table, _out(c, torch.bfloat16).fill_(7.0), c["hw"])
        got = f32.cpu()
        e32 = c[("img_e32", dtype)]
        err = float((got.double() - c[("img64", dtype)]).abs().max())
        bound = max(4 * e32, FLOOR)
        print(f"{shape} {tname} {dtype} {layout}: reference fp32 error {e32:.3e}, kernel error {err:.3e}, "
              f"bound {bound:.3e}")
        assert err <= bound, (shape, tname, dtype, layout, err, bound)
        assert torch.equal(b16.view(torch.int16), f32.to(torch.bfloat16).view(torch.int16)), (shape, tname, dtype)
        assert (got[:, :, h:] == 0).all() and (got[:, :, :, w:] == 0).all(), (tname, dtype)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_quarters_are_the_sources_bitwise(hip_lib, shape):
    from src.rtdetr_moe.augment import mosaic_images_hip

    c = _case(shape, "quarters")
    h, w = c["hw"]
    B = c["B"]
    # x / 255 as the loader forms it: the correctly rounded quotient, computed on the host
    ref = c["srcs"][torch.float32][:, :, :h, :w].to(DEV)
    for dtype, layout in SOURCES:
        out = mosaic_images_hip(_src(c, dtype, layout), c["table"].to(DEV), _out(c, torch.float32), c["hw"])
        for n in range(B):
            tr, bl, br = _partners(B)[n]
            assert torch.equal(out[n, :, :h // 2, :w // 2], ref[n, :, h // 2:, w // 2:])
            assert torch.equal(out[n, :, :h // 2, w // 2:w], ref[tr, :, h // 2:, :w // 2])
            assert torch.equal(out[n, :, h // 2:h, :w // 2], ref[bl, :, :h // 2, w // 2:])
            assert torch.equal(out[n, :, h // 2:h, w // 2:w], ref[br, :, :h // 2, :w // 2])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_degenerate_rows_are_the_plain_kernel_bitwise(hip_lib, shape):
    from src.rtdetr_moe.augment import augment_images_hip, mosaic_images_hip

    c = _case(shape, "degenerate")
    table = c["table"].to(DEV)
    plain = table[:, :16].contiguous()
    for dtype, layout in SOURCES:
        src = _src(c, dtype, layout)
        for dst in (torch.float32, torch.bfloat16):
            bits = torch.int32 if dst == torch.float32 else torch.int16
            got = mosaic_images_hip(src, table, _out(c, dst), c["hw"])
            want = augment_images_hip(src, plain, _out(c, dst), c["hw"])
            assert torch.equal(got.view(bits), want.view(bits)), (shape, dtype, layout, dst)


def _check_boxes(c, got, M_out):
    from src.rtdetr_moe.criterion import PAD_BOX

    gb, gl, gnv, gtot = (t.cpu() for t in got)
    rb, rl, rnv, rtot = c["box64"]
    assert c["margin"] >= MARGIN, c["margin"]                        # every decision is clear of its thresholds
    assert gb.shape == (c["B"], M_out, 4) and gl.shape == (c["B"], M_out)
    assert torch.equal(gnv, rnv) and float(gtot) == float(rtot) and gtot.dtype == torch.float32
    assert torch.equal(gl, rl)                                       # survivor set, order, padding labels
    err = float((gb.double() - rb).abs().max())
    bound = max(4 * c["box_e32"], FLOOR)
    print(f"boxes: kept {rnv.tolist()}, reference fp32 error {c['box_e32']:.3e}, kernel error {err:.3e}, "
          f"bound {bound:.3e}")
    assert err <= bound, (err, bound)
    for b in range(c["B"]):                                          # the tail is PAD_BOX exactly
        n = int(rnv[b])
        assert torch.equal(gb[b, n:], torch.tensor(PAD_BOX).expand(M_out - n, 4))


@pytest.mark.parametrize("tname", TABLES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_boxes(hip_lib, shape, tname):
    from src.rtdetr_moe.augment import mosaic_boxes_hip

    c = _case(shape, tname)
    tb, tl, nv = (t.to(DEV) for t in c["targets"])
    if tname == "half" and shape == "pad":
        kept, raw = c["box64"][2], c["targets"][2]
        assert int(kept.max()) > int(raw.max())                      # an image holds more boxes than any source
    _check_boxes(c, mosaic_boxes_hip(tb, tl, nv, c["table"].to(DEV), c["hw"], c["phw"], M_out=c["M_out"]),
                 c["M_out"])


@functools.lru_cache(maxsize=None)
def _many():
    """B = 2, M_in = 80 with 70 valid boxes in image 0 (two rounds per
    quadrant): output image 0 holds image 0 in its top-left and bottom-left
    quadrant, output image 1 in its top-left and top-right one."""
    from src.rtdetr_moe import augment as A

    B, hw, phw, M_in = 2, (40, 60), (64, 64), 80
    h, w = hw
    table = A.make_mosaic_table([0.62, 0.7], [w * 0.48, w * 0.53], [h * 0.51, h * 0.46], [False, True], [0.0] * B,
                                [1.0] * B, [1.0] * B, hw, [True] * B, [w - 3, w + 2], [h + 1, h - 2],
                                [[1, 0, 1], [0, 1, 1]])
    tb, tl, nv = _make_boxes(B, M_in, [70, 20], hw, phw, table, seed=13)
    return dict(B=B, hw=hw, phw=phw, table=table, targets=(tb, tl, nv))


def test_boxes_two_rounds(hip_lib):
    """Survivors of later rounds and quadrants land behind the earlier ones, past slot 64."""
    from src.rtdetr_moe.augment import mosaic_boxes_hip

    c = dict(_many())
    tb, tl, nv = c["targets"]
    _box_refs(c, tb, tl, nv, c["table"], c["hw"], c["phw"], 128)
    assert 64 < int(c["box64"][2].max()) <= 128, c["box64"][2]
    _check_boxes(c, mosaic_boxes_hip(tb.to(DEV), tl.to(DEV), nv.to(DEV), c["table"].to(DEV), c["hw"], c["phw"],
                                     M_out=128), 128)


def test_boxes_overflow_keeps_the_first_and_stays_inside(hip_lib):
    """M_out = 16 with more than 16 survivors per image: n_valid = 16, the
    first 16 survivors in order, and nothing written outside the outputs (views
    into the middle of sentinel-filled buffers)."""
    from src.rtdetr_moe.augment import mosaic_boxes_hip

    c = dict(_many())
    tb, tl, nv = c["targets"]
    B, Mo, G = c["B"], 16, 64
    _box_refs(c, tb, tl, nv, c["table"], c["hw"], c["phw"], 128)
    full_b, full_l, full_nv, _ = c["box64"]
    assert int(full_nv.min()) > Mo
    fb = torch.full((G + B * Mo * 4 + G,), -7.0, device=DEV)
    fl = torch.full((G + B * Mo + G,), -7, dtype=torch.int64, device=DEV)
    fn = torch.full((G + B + G,), -7, dtype=torch.int32, device=DEV)
    ft = torch.full((3,), -7.0, device=DEV)
    out = (fb[G:G + B * Mo * 4].view(B, Mo, 4), fl[G:G + B * Mo].view(B, Mo), fn[G:G + B], ft[1:2].view(()))
    ob, ol, onv, total = mosaic_boxes_hip(tb.to(DEV), tl.to(DEV), nv.to(DEV), c["table"].to(DEV), c["hw"], c["phw"],
                                          out=out)
    torch.cuda.synchronize()
    assert onv.tolist() == [Mo] * B and float(total) == float(Mo * B)
    assert torch.equal(ol.cpu(), full_l[:, :Mo])
    err = float((ob.cpu().double() - full_b[:, :Mo]).abs().max())
    assert err <= max(4 * c["box_e32"], FLOOR), err
    for flat, n in ((fb, B * Mo * 4), (fl, B * Mo), (fn, B)):
        assert (flat[:G] == -7).all() and (flat[G + n:] == -7).all()
    assert float(ft[0]) == -7.0 and float(ft[2]) == -7.0


def test_batch_augment_gpu_matches_its_kernels(hip_lib):
    from src.rtdetr_moe import augment as A

    c = _case("pad", "rand0")
    tb, tl, nv = (t.to(DEV) for t in c["targets"])
    aug = A.BatchAugment(c["B"], c["hw"], c["phw"], DEV, seed=9, mosaic=1.0)
    src = _src(c, torch.uint8, "nchw")
    img, ob, ol, onv, total = aug(src, tb, tl, nv, M_out=64)
    assert aug.need(c["targets"][2].tolist()) <= 64
    table = aug.table_host.to(DEV)
    assert torch.equal(aug.table, table) and table.shape == (c["B"], A.MOSAIC_COLS)
    assert torch.equal(img, A.mosaic_images_hip(src, table, _out(c, torch.float32), c["hw"]))
    wb, wl, wnv, wtot = A.mosaic_boxes_hip(tb, tl, nv, table, c["hw"], c["phw"], M_out=64)
    assert torch.equal(ob, wb) and torch.equal(ol, wl) and torch.equal(onv, wnv) and torch.equal(total, wtot)
    # set to 0 between steps: degenerate rows through the same kernels = the plain kernels' result
    aug.mosaic = 0.0
    img, ob, ol, onv, total = aug(src, tb, tl, nv, M_out=64)
    t = aug.table_host
    assert (t[:, 19:22] == -1).all()
    plain = t[:, :16].contiguous().to(DEV)
    assert torch.equal(img, A.augment_images_hip(src, plain, _out(c, torch.float32), c["hw"]))


def test_argument_checks(hip_lib):
    """Each bad call comes back with a non-zero code (MoEKernelError carries
    it and the moe_last_error message) before any launch."""
    from src.moe import _lib as L
    from src.rtdetr_moe import augment as A

    torch.cuda.synchronize()
    L.launch_counts(reset=True)
    hw = (40, 60)
    table = A.make_mosaic_table(*A._draw_terms(torch.Generator().manual_seed(1), 1, hw, hw, A.AugmentParams()),
                                hw).to(DEV)
    src = torch.zeros((1, 3, 64, 62), dtype=torch.uint8, device=DEV)
    out = torch.empty((1, 3, 64, 62), dtype=torch.float32, device=DEV, memory_format=torch.channels_last)
    with pytest.raises(L.MoEKernelError, match=r"rc=-1.*multiple of 4"):
        A.mosaic_images_hip(src, table, out, hw)
    src = torch.zeros((1, 3, 64, 64), dtype=torch.uint8, device=DEV)
    good = torch.empty((1, 3, 64, 64), dtype=torch.float32, device=DEV, memory_format=torch.channels_last)
    with pytest.raises(L.MoEKernelError, match="24"):                    # a plain table
        A.mosaic_images_hip(src, table[:, :16].contiguous(), good, hw)
    with pytest.raises(L.MoEKernelError, match=r"rc=-1.*content rectangle"):
        A.mosaic_images_hip(src, table, good, (80, 60))
    tb = torch.zeros((1, 16, 4), device=DEV)
    tl = torch.zeros((1, 16), dtype=torch.int64, device=DEV)
    nv = torch.zeros(1, dtype=torch.int32, device=DEV)
    tot = torch.zeros((), device=DEV)
    with pytest.raises(L.MoEKernelError, match="24"):
        A.mosaic_boxes_hip(tb, tl, nv, table[:, :16].contiguous(), hw, (64, 64))
    with pytest.raises(L.MoEKernelError, match=r"rc=-1.*alias"):         # in place
        A.mosaic_boxes_hip(tb, tl, nv, table, hw, (64, 64), out=(tb, tl, torch.empty_like(nv), tot))
    with pytest.raises(L.MoEKernelError, match=r"rc=-1.*alias"):
        A.mosaic_boxes_hip(tb, tl, nv, table, hw, (64, 64), out=(torch.empty_like(tb), torch.empty_like(tl), nv, tot))
    with pytest.raises(L.MoEKernelError, match=r"rc=-1.*1\.\.1024"):
        A.mosaic_boxes_hip(tb, tl, nv, table, hw, (64, 64), M_out=2048)
    with pytest.raises(L.MoEKernelError, match="GPU tensor"):
        A.mosaic_images_hip(src.cpu(), table, good, hw)
    assert "augment" not in L.launch_counts()
    # a table whose indices point past the batch reads nothing: those quadrants are empty
    bad = table.clone()
    bad[:, 12:15] = torch.tensor([0.0, 1.0, 1.0])                        # no colour: continuous everywhere
    bad[:, 16:18] = torch.tensor([30.0, 20.0])
    bad[:, 19:22] = torch.tensor([1.0, 7.0, 1e9])
    got = A.mosaic_images_hip(src, bad, good, hw)
    assert L.launch_counts(reset=True).get("augment") == 1
    want = A.mosaic_reference_images(src.cpu(), bad.cpu(), hw, dtype=torch.float64)
    assert float((got.cpu().double() - want).abs().max()) <= 1e-6
