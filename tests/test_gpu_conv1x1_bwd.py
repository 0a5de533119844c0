"""rtdetr_conv1x1_bwd (csrc/conv.hip: the ResNet stage-1 1x1 convolutions'
data gradient and weight-gradient slices in one launch) against the two
launches it replaces, rtdetr_conv_dgrad + rtdetr_conv_wgrad, on the same
inputs.

Acceptance is bitwise: the fused kernel keeps the data gradient's K order
(ascending 32-deep MFMA steps over N from a zero accumulator), the epilogue's
arithmetic and order (bf16 result, + add, ReLU mask of x), the slice bounds of
rtdetr_conv_wgrad_splits and the ascending pixel order inside a slice, so dx,
the fp32 partials and the reduced dW must all be equal bit for bit -- also
against the two-launch path's other tile choices (flipped weight, 32-deep
K-tiles: what it runs at the training shapes).

Shapes (B, H, W): (1, 5, 7) P = 35, less than one 64-pixel K-tile;
(2, 9, 13) P = 234, ragged tail; (3, 16, 24) 18 K-tiles in 2 slices;
(2, 41, 52) 67 K-tiles in 8 slices with a short last slice and a 40-pixel
tail.  x is a ReLU output (about half its entries exactly zero)."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

_SHAPES = [(1, 5, 7), (2, 9, 13), (3, 16, 24), (2, 41, 52)]
_CHANNELS = [(64, 256), (256, 64)]
_PAD = 4096  # sentinel elements behind every output: nothing may be written there
_INPUTS: dict = {}
_REFS: dict = {}


def _inputs(B, H, W, C, N):
    """(x, g, w, add) for a case: flat NHWC bf16, made once and never modified."""
    key = (B, H, W, C, N)
    if key not in _INPUTS:
        gen = torch.Generator(device=DEV).manual_seed(1000 * B + 10 * H + W + C)
        P = B * H * W
        x = torch.relu(torch.randn(P, C, device=DEV, generator=gen)).to(torch.bfloat16)
        g = torch.randn(P, N, device=DEV, generator=gen).to(torch.bfloat16)
        w = (0.05 * torch.randn(N, C, device=DEV, generator=gen)).to(torch.bfloat16)
        add = torch.randn(P, C, device=DEV, generator=gen).to(torch.bfloat16)
        _INPUTS[key] = (x, g, w, add)
    return _INPUTS[key]


def _outputs(P, C, N, ns):
    dx = torch.full((P * C + _PAD,), 7.0, dtype=torch.bfloat16, device=DEV)
    part = torch.full((ns * N * C + _PAD,), float("nan"), dtype=torch.float32, device=DEV)
    dw = torch.full((N * C + _PAD,), 7.0, dtype=torch.bfloat16, device=DEV)
    return dx, part, dw


def _check_pads(P, C, N, ns, dx, part, dw):
    assert (dx[P * C:] == 7.0).all() and (dw[N * C:] == 7.0).all() and torch.isnan(part[ns * N * C:]).all()


def _splits(hip_lib, B, H, W, C, N):
    return hip_lib.rtdetr_conv_wgrad_splits(B, H, W, C, N, 1)


def _two_launches(hip_lib, B, H, W, C, N, mask, use_add, ns):
    """dx, partials, dW of rtdetr_conv_dgrad + rtdetr_conv_wgrad."""
    from src.moe import _lib as L
    from src.rtdetr_moe import conv as Cv

    x, g, w, add = _inputs(B, H, W, C, N)
    P = B * H * W
    dx, part, dw = _outputs(P, C, N, ns)
    z, s = Cv._zero(x.device).data_ptr(), L._stream()
    nb = hip_lib.rtdetr_conv_dgrad_workspace(B, H, W, C, N, 1)
    work = torch.empty(max(nb // 2, 8), dtype=torch.bfloat16, device=DEV)
    L._check(hip_lib.rtdetr_conv_dgrad(g.data_ptr(), w.data_ptr(), work.data_ptr() if nb else None, dx.data_ptr(), z,
                                       B, H, W, C, N, 1, 1, add.data_ptr() if use_add else None,
                                       x.data_ptr() if mask else None, s), "rtdetr_conv_dgrad")
    L._check(hip_lib.rtdetr_conv_wgrad(g.data_ptr(), x.data_ptr(), part.data_ptr(), ns, dw.data_ptr(), 1, z,
                                       B, H, W, C, N, 1, 1, s), "rtdetr_conv_wgrad")
    _check_pads(P, C, N, ns, dx, part, dw)
    return dx, part, dw


def _reference(hip_lib, B, H, W, C, N, mask, use_add):
    key = (B, H, W, C, N, mask, use_add)
    if key not in _REFS:
        _REFS[key] = _two_launches(hip_lib, B, H, W, C, N, mask, use_add, _splits(hip_lib, B, H, W, C, N))
    return _REFS[key]


def _fused(hip_lib, B, H, W, C, N, mask, use_add, ns):
    from src.moe import _lib as L
    from src.rtdetr_moe import conv as Cv

    x, g, w, add = _inputs(B, H, W, C, N)
    P = B * H * W
    dx, part, dw = _outputs(P, C, N, ns)
    s = L._stream()
    L._check(hip_lib.rtdetr_conv1x1_bwd(g.data_ptr(), x.data_ptr(), w.data_ptr(), dx.data_ptr(), part.data_ptr(), ns,
                                        Cv._zero(x.device).data_ptr(), B, H, W, C, N,
                                        add.data_ptr() if use_add else None, int(mask), s), "rtdetr_conv1x1_bwd")
    Cv._reduce_wgrads([(part, ns, N * C, dw)], s)
    _check_pads(P, C, N, ns, dx, part, dw)
    return dx, part, dw


def _same_bits(a, b, what):
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    else:
        a, b = a.view(torch.int16), b.view(torch.int16)
    bad = (a != b).sum().item()
    assert bad == 0, f"{what}: {bad} of {a.numel()} elements differ"


@pytest.mark.parametrize("use_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("C,N", _CHANNELS)
@pytest.mark.parametrize("B,H,W", _SHAPES)
def test_fused_matches_two_launches_bitwise(hip_lib, B, H, W, C, N, mask, use_add):
    x = _inputs(B, H, W, C, N)[0]
    zeros = (x == 0).float().mean().item()
    assert 0.4 < zeros < 0.6  # the mask is exercised
    ns = _splits(hip_lib, B, H, W, C, N)
    assert ns == {35: 1, 234: 1, 1152: 2, 4264: 8}[B * H * W]
    ref = _reference(hip_lib, B, H, W, C, N, mask, use_add)
    got = _fused(hip_lib, B, H, W, C, N, mask, use_add, ns)
    for a, b, what in zip(got, ref, ("dx", "partials", "dW")):
        _same_bits(a, b, what)
    if mask:
        P = B * H * W
        assert (got[0][:P * C].view(P, C)[x == 0] == 0).all()


@pytest.mark.parametrize("C,N", _CHANNELS)
def test_empty_slices_write_zeros(hip_lib, C, N):
    """More slices than K-tiles (P = 35 in 4 slices; P = 234 in 3, whose last is empty): the slices with no
    pixels are zeros, as rtdetr_conv_wgrad_part leaves them."""
    for (B, H, W), ns in (((1, 5, 7), 4), ((2, 9, 13), 3)):
        ref = _two_launches(hip_lib, B, H, W, C, N, True, True, ns)
        got = _fused(hip_lib, B, H, W, C, N, True, True, ns)
        for a, b, what in zip(got, ref, ("dx", "partials", "dW")):
            _same_bits(a, b, what)
        ktot = -(-B * H * W // 64)
        kt_per = -(-ktot // ns)
        first_empty = -(-ktot // kt_per)
        assert first_empty < ns and (got[1][first_empty * N * C:ns * N * C] == 0).all()


@pytest.mark.parametrize("knobs", [dict(conv_dgrad_flip=1, conv_k32=1), dict(conv_dgrad_flip=1, conv_k32=0),
                                   dict(conv_dgrad_flip=0, conv_k32=2, conv_bm=64), dict(conv_wg_stages=3)],
                         ids=["flip_k32", "flip_k64", "inplace_k32_bm64", "wg3"])
@pytest.mark.parametrize("C,N", _CHANNELS)
def test_fused_matches_the_other_tile_choices(hip_lib, C, N, knobs):
    """The two launches with the flipped weight / 32-deep K-tiles (their choice at the training shapes) and other
    rings give the same bits, so the equality above carries over to those shapes."""
    B, H, W = 2, 41, 52
    ns = _splits(hip_lib, B, H, W, C, N)
    for k, v in knobs.items():
        assert hip_lib.rtdetr_conv_set_tuning(k.encode(), v) == 0
    try:
        ref = _two_launches(hip_lib, B, H, W, C, N, True, True, ns)
    finally:
        for k, v in dict(conv_dgrad_flip=-1, conv_k32=-1, conv_bm=0, conv_wg_stages=0).items():
            hip_lib.rtdetr_conv_set_tuning(k.encode(), v)
    got = _fused(hip_lib, B, H, W, C, N, True, True, ns)
    for a, b, what in zip(got, ref, ("dx", "partials", "dW")):
        _same_bits(a, b, what)


@pytest.mark.parametrize("C,N", _CHANNELS)
def test_two_runs_are_identical(hip_lib, C, N):
    B, H, W = _SHAPES[-1]
    ns = _splits(hip_lib, B, H, W, C, N)
    a = _fused(hip_lib, B, H, W, C, N, True, True, ns)
    b = _fused(hip_lib, B, H, W, C, N, True, True, ns)
    _same_bits(a[0], b[0], "dx")
    _same_bits(a[1], b[1], "partials")


def test_unsupported_shape_falls_back(hip_lib, monkeypatch):
    """C = 128, N = 512: the entry returns an error, conv._bwd takes the two launches."""
    from src.moe import _lib as L
    from src.rtdetr_moe import conv as Cv

    B, H, W, C, N = 2, 9, 13, 128, 512
    x, g, w, add = _inputs(B, H, W, C, N)
    P = B * H * W
    ns = _splits(hip_lib, B, H, W, C, N)
    dx, part, dw = _outputs(P, C, N, ns)
    rc = hip_lib.rtdetr_conv1x1_bwd(g.data_ptr(), x.data_ptr(), w.data_ptr(), dx.data_ptr(), part.data_ptr(), ns,
                                    Cv._zero(x.device).data_ptr(), B, H, W, C, N, None, 1, L._stream())
    assert rc != 0 and "rtdetr_conv1x1_bwd" in hip_lib.moe_last_error().decode()
    assert (dx == 7.0).all() and torch.isnan(part).all()  # nothing ran
    ref = _two_launches(hip_lib, B, H, W, C, N, True, True, ns)
    nchw = lambda t, ch: t.view(B, H, W, ch).permute(0, 3, 1, 2)  # noqa: E731  (channels_last views)
    monkeypatch.setattr(Cv, "_BWD_FUSE_ON", True)
    gx, gw = Cv._bwd(nchw(x, C), w.view(N, C, 1, 1), nchw(g, N), True, True, True, nchw(add, C))
    torch.cuda.synchronize()
    _same_bits(gx.permute(0, 2, 3, 1).reshape(-1), ref[0][:P * C], "dx")
    _same_bits(gw.reshape(-1), ref[2][:N * C], "dW")


@pytest.mark.parametrize("C,N", _CHANNELS)
def test_bwd_switch(hip_lib, monkeypatch, C, N):
    """conv._bwd with MOE_CONV_BWD_FUSE on and off (conv._BWD_FUSE_ON): the same bits, inside and outside a
    deferred_wgrads scope."""
    from src.rtdetr_moe import conv as Cv

    B, H, W = 3, 16, 24
    x, g, w, add = _inputs(B, H, W, C, N)
    nchw = lambda t, ch: t.view(B, H, W, ch).permute(0, 3, 1, 2)  # noqa: E731
    res = []
    for fuse in (True, False):
        monkeypatch.setattr(Cv, "_BWD_FUSE_ON", fuse)
        for defer in (False, True):
            with Cv.deferred_wgrads(defer):
                gx, gw = Cv._bwd(nchw(x, C), w.view(N, C, 1, 1), nchw(g, N), True, True, True, nchw(add, C))
            res.append((gx, gw))
    for gx, gw in res[1:]:
        _same_bits(gx.permute(0, 2, 3, 1).reshape(-1), res[0][0].permute(0, 2, 3, 1).reshape(-1), "dx")
        _same_bits(gw.reshape(-1), res[0][1].reshape(-1), "dW")


@pytest.mark.parametrize("defer", [False, True], ids=["per_conv_sums", "deferred_wgrads"])
def test_backbone_stage1_switch_is_bitwise(hip_lib, monkeypatch, defer):
    """PResNet(50)'s stem + stage 1 on a 2 x 3 x 64 x 96 input (calibrated frozen BN): every parameter gradient
    and the gradient of the stage's input are the same bits with the fused backward on and off."""
    from src.rtdetr_moe import backbone as bb
    from src.rtdetr_moe import conv as Cv

    torch.manual_seed(0)
    m = bb.PResNet(50)
    img = torch.randn(2, 3, 64, 96)
    bb.calibrate_frozen_bn(m, img)
    m = m.to(DEV).to(torch.bfloat16).to(memory_format=torch.channels_last)
    x = img.to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    params = [p for p in m.stages[0].parameters() if p.requires_grad]
    r = None
    res = []
    for fuse in (True, False):
        monkeypatch.setattr(Cv, "_BWD_FUSE_ON", fuse)
        m._fold_all()
        with torch.no_grad():
            h = bb.stem_max_pool(m._stem(x), m.pool)
        h = h.detach().requires_grad_(True)
        y, ys = h, None
        for blk in m.stages[0]:
            y, ys = blk(y, ys)
        if r is None:
            r = torch.randn(y.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)).to(y.dtype)
        loss = (y.float() * r.float()).sum()
        with Cv.deferred_wgrads(defer):
            grads = torch.autograd.grad(loss, params + [h], allow_unused=True)
        torch.cuda.synchronize()
        res.append(grads)
    used = 0
    for a, b in zip(*res):
        assert (a is None) == (b is None)
        if a is not None:
            used += 1
            assert torch.isfinite(a.float()).all()
            _same_bits(a.contiguous().reshape(-1), b.contiguous().reshape(-1), "gradient")
    assert used >= 11 and res[0][-1] is not None  # the ten stage-1 convolutions' weights and the input
