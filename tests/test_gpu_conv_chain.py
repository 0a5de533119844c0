"""rtdetr_conv1x1_block_out (csrc/conv.hip: a ResNet stage-1 block output, the
first block's shortcut convolution and the next block's branch2a in one
launch) against the separate rtdetr_conv_fwd launches it replaces, and the
backbone with MOE_CONV_CHAIN on against off.

Every comparison is bitwise: the kernel keeps conv_fwd_kernel's MFMA operand
roles and K order (ascending 32-deep steps from a zero accumulator) and
conv_epilogue's arithmetic and order of adds, and the second GEMM reads the
bf16-rounded y tile, so y and h must equal the separate launches bit for bit.

Shapes (B, H, W): (1, 5, 7) P = 35, less than one 64-pixel tile; (2, 9, 13)
P = 234, a ragged last tile; (3, 16, 24) 18 tiles; (2, 41, 52) 67 tiles with a
40-pixel tail.  Each runs with the automatic workgroup count (one tile per
workgroup, fewer tiles than CUs) and with 8 workgroups (up to 9 tiles each:
the ring wraps, the last workgroup is short).  The operands are zero-mean, so
about half of the pre-ReLU values of y and of h are negative; both biases
have both signs."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

_SHAPES = [(1, 5, 7), (2, 9, 13), (3, 16, 24), (2, 41, 52)]
_PAD = 4096  # sentinel elements behind every output: nothing may be written there
_INPUTS: dict = {}
_REFS: dict = {}


def _inputs(B, H, W):
    """Flat NHWC bf16 operands of a case, made once and never modified."""
    key = (B, H, W)
    if key not in _INPUTS:
        gen = torch.Generator(device=DEV).manual_seed(100 * B + 10 * H + W)
        P = B * H * W
        rn = lambda *s: torch.randn(*s, device=DEV, generator=gen)  # noqa: E731
        _INPUTS[key] = dict(
            h2=torch.relu(rn(P, 64)).to(torch.bfloat16), w2c=(0.1 * rn(256, 64)).to(torch.bfloat16),
            resid=rn(P, 256).to(torch.bfloat16), xs=torch.relu(rn(P, 64)).to(torch.bfloat16),
            ws=(0.15 * rn(256, 64)).to(torch.bfloat16), bias=(0.3 * rn(256)).float().contiguous(),
            wn={n: (0.05 * rn(n, 256)).to(torch.bfloat16) for n in (64, 128)},
            bias_n={n: (0.3 * rn(n)).float().contiguous() for n in (64, 128)})
    return _INPUTS[key]


def _out(n):
    return torch.full((n + _PAD,), 7.0, dtype=torch.bfloat16, device=DEV)


def _conv_fwd(hip_lib, x, w, y, B, H, W, C, N, bias=None, resid=None, relu=False):
    from src.moe import _lib as L
    from src.rtdetr_moe import conv as Cv

    L._check(hip_lib.rtdetr_conv_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), Cv._zero(x.device).data_ptr(), B, H, W,
                                     C, N, 1, 1, None if bias is None else bias.data_ptr(),
                                     None if resid is None else resid.data_ptr(), int(relu), L._stream()),
             "rtdetr_conv_fwd")


def _reference(hip_lib, B, H, W, short_conv, nxt):
    """(y, h) of the separate launches: [the bias-free shortcut convolution,]
    branch2c + resid + bias + ReLU, then the next layer + bias + ReLU."""
    key = (B, H, W, short_conv, nxt)
    if key not in _REFS:
        t = _inputs(B, H, W)
        P = B * H * W
        resid = t["resid"]
        if short_conv:
            resid = _out(P * 256)
            _conv_fwd(hip_lib, t["xs"], t["ws"], resid, B, H, W, 64, 256)
        y, h = _out(P * 256), _out(P * max(nxt, 1))
        _conv_fwd(hip_lib, t["h2"], t["w2c"], y, B, H, W, 64, 256, t["bias"], resid, True)
        if nxt:
            _conv_fwd(hip_lib, y, t["wn"][nxt], h, B, H, W, 256, nxt, t["bias_n"][nxt], None, True)
        torch.cuda.synchronize()
        _REFS[key] = (y, h)
    return _REFS[key]


def _fused(hip_lib, B, H, W, short_conv, nxt, nwg):
    from src.moe import _lib as L
    from src.rtdetr_moe import conv as Cv

    t = _inputs(B, H, W)
    P = B * H * W
    y, h = _out(P * 256), _out(P * max(nxt, 1))
    L._check(hip_lib.rtdetr_conv1x1_block_out(
        t["h2"].data_ptr(), t["w2c"].data_ptr(), None if short_conv else t["resid"].data_ptr(),
        t["xs"].data_ptr() if short_conv else None, t["ws"].data_ptr() if short_conv else None, t["bias"].data_ptr(),
        y.data_ptr(), t["wn"][nxt].data_ptr() if nxt else None, t["bias_n"][nxt].data_ptr() if nxt else None,
        h.data_ptr() if nxt else None, nxt, Cv._zero(y.device).data_ptr(), B, H, W, nwg, L._stream()),
        "rtdetr_conv1x1_block_out")
    torch.cuda.synchronize()
    return y, h


def _same_bits(a, b, what):
    bad = (a.view(torch.int16) != b.view(torch.int16)).sum().item()
    assert bad == 0, f"{what}: {bad} of {a.numel()} elements differ"


@pytest.mark.parametrize("nxt", [0, 64, 128])
@pytest.mark.parametrize("short_conv", [False, True], ids=["resid_tensor", "resid_conv"])
@pytest.mark.parametrize("B,H,W", _SHAPES)
def test_kernel_matches_separate_launches_bitwise(hip_lib, B, H, W, short_conv, nxt):
    P = B * H * W
    ry, rh = _reference(hip_lib, B, H, W, short_conv, nxt)
    zy = (ry[:P * 256] == 0).float().mean().item()
    assert 0.3 < zy < 0.7  # about half of y's pre-ReLU values are negative
    if nxt:
        zh = (rh[:P * nxt] == 0).float().mean().item()
        assert 0.3 < zh < 0.7
    assert (ry[P * 256:] == 7.0).all()
    for nwg in (0, 8):
        y, h = _fused(hip_lib, B, H, W, short_conv, nxt, nwg)
        _same_bits(y, ry, f"y (nwg {nwg})")  # (the sentinels too: nothing written past the outputs)
        _same_bits(h, rh, f"h (nwg {nwg})")


@pytest.mark.parametrize("short_conv", [False, True], ids=["resid_tensor", "resid_conv"])
def test_two_runs_are_identical(hip_lib, short_conv):
    B, H, W = _SHAPES[-1]
    a = _fused(hip_lib, B, H, W, short_conv, 64, 8)
    b = _fused(hip_lib, B, H, W, short_conv, 64, 8)
    _same_bits(a[0], b[0], "y")
    _same_bits(a[1], b[1], "h")


def test_bad_arguments_are_errors(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe import conv as Cv

    t = _inputs(1, 5, 7)
    y = _out(35 * 256)
    z = Cv._zero(y.device).data_ptr()
    p = lambda k: t[k].data_ptr()  # noqa: E731
    # both kinds of residual, none of them, and a next width without an instance
    for resid, xs, nxt in ((p("resid"), p("xs"), 0), (None, None, 0), (p("resid"), None, 32)):
        rc = hip_lib.rtdetr_conv1x1_block_out(p("h2"), p("w2c"), resid, xs, p("ws"), p("bias"), y.data_ptr(),
                                              t["wn"][64].data_ptr(), t["bias_n"][64].data_ptr(), y.data_ptr(), nxt, z,
                                              1, 5, 7, 0, L._stream())
        assert rc != 0 and "rtdetr_conv1x1_block_out" in hip_lib.moe_last_error().decode()
    torch.cuda.synchronize()
    assert (y == 7.0).all()  # nothing ran


# ---- the backbone, MOE_CONV_CHAIN on against off ----

_NET: dict = {}


def _net():
    """PResNet(50) with calibrated frozen BNs, bf16 channels_last, and two 2 x 3 x 64 x 96 inputs."""
    if not _NET:
        from src.rtdetr_moe import backbone as bb

        torch.manual_seed(0)
        m = bb.PResNet(50)
        imgs = [torch.randn(2, 3, 64, 96) for _ in range(2)]
        bb.calibrate_frozen_bn(m, imgs[0])
        _NET["m"] = m.to(DEV).to(torch.bfloat16).to(memory_format=torch.channels_last)
        _NET["x"] = [i.to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last) for i in imgs]
    return _NET["m"], _NET["x"]


def _count_launches(monkeypatch, Cv):
    """Counts the rtdetr_conv1x1_block_out launches conv.py makes."""
    n = [0]
    real = Cv._fwd_block_out

    def counted(*a, **k):
        n[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(Cv, "_fwd_block_out", counted)
    return n


@pytest.mark.parametrize("defer", [False, True], ids=["per_conv_sums", "deferred_wgrads"])
def test_backbone_training_switch_is_bitwise(hip_lib, monkeypatch, defer):
    """C3-C5 and every parameter gradient are the same bits with the chained launches on and off."""
    from src.rtdetr_moe import conv as Cv

    m, (x, _) = _net()
    params = [p for p in m.parameters() if p.requires_grad]
    n = _count_launches(monkeypatch, Cv)
    res = []
    for on in (True, False):
        monkeypatch.setattr(Cv, "_CHAIN_ON", on)
        n[0] = 0
        outs = m(x)
        assert n[0] == (3 if on else 0)  # the three stage-1 blocks
        gen = torch.Generator(device=DEV).manual_seed(5)
        loss = sum((o.float() * torch.randn(o.shape, device=DEV, generator=gen)).sum() for o in outs)
        with Cv.deferred_wgrads(defer):
            grads = torch.autograd.grad(loss, params, allow_unused=True)
        torch.cuda.synchronize()
        res.append(([o.detach() for o in outs], grads))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.isfinite(a.float()).all()
        _same_bits(a.contiguous().reshape(-1), b.contiguous().reshape(-1), "stage output")
    used = 0
    for a, b in zip(res[0][1], res[1][1]):
        assert (a is None) == (b is None)
        if a is not None:
            used += 1
            assert torch.isfinite(a.float()).all()
            _same_bits(a.contiguous().reshape(-1), b.contiguous().reshape(-1), "gradient")
    assert used >= 50


def _forward_off(m, x, monkeypatch, Cv):
    monkeypatch.setattr(Cv, "_CHAIN_ON", False)
    with torch.no_grad():
        ref = [o.clone() for o in m(x)]
    monkeypatch.setattr(Cv, "_CHAIN_ON", True)
    return ref


def test_backbone_no_grad_switch_is_bitwise(hip_lib, monkeypatch):
    from src.rtdetr_moe import conv as Cv

    m, (x, _) = _net()
    ref = _forward_off(m, x, monkeypatch, Cv)
    n = _count_launches(monkeypatch, Cv)
    with torch.no_grad():
        outs = m(x)
    torch.cuda.synchronize()
    assert n[0] == 3
    for a, b in zip(outs, ref):
        _same_bits(a.contiguous().reshape(-1), b.contiguous().reshape(-1), "stage output")


def test_backbone_graph_replay_is_bitwise(hip_lib, monkeypatch):
    """The chained forward captured in a hipGraph and replayed on two inputs."""
    from src.rtdetr_moe import conv as Cv

    m, xs = _net()
    refs = [_forward_off(m, x, monkeypatch, Cv) for x in xs]
    static = xs[0].clone(memory_format=torch.channels_last)
    with torch.no_grad():
        m(static)  # first use outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        outs = m(static)
    for i in (1, 0):
        static.copy_(xs[i])
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, refs[i]):
            _same_bits(a.contiguous().reshape(-1), b.contiguous().reshape(-1), f"stage output (input {i})")


@pytest.mark.parametrize("change", ["weight_in_place", "weight_replaced", "bias"])
def test_parked_output_is_dropped_when_the_next_layer_changed(hip_lib, monkeypatch, change):
    """Block 1 parks block 2's branch2a output; block 2's weight or shift changes before block 2 runs: its
    branch2a launches with the new values (the result is the one the switch-off path gives with them)."""
    from src.rtdetr_moe import backbone as bb
    from src.rtdetr_moe import conv as Cv

    m, (x, _) = _net()
    b1, b2 = m.stages[0][0], m.stages[0][1]
    a2 = b2.branch2a
    bias0 = a2.norm.bias.clone()
    res = {}
    try:
        for on in (True, False):
            monkeypatch.setattr(Cv, "_CHAIN_ON", on)
            with torch.no_grad():
                m._fold_all()
                h = bb.stem_max_pool(m._stem(x), m.pool)
                y, ys = b1(h, None, a2)
                parked = y.grad_link.h_next
                assert (parked is not None) == on
                if change == "weight_in_place":
                    a2._w_folded.mul_(0.5)
                elif change == "weight_replaced":
                    a2._w_folded = a2._w_folded * 0.5
                else:
                    a2.norm.bias.add_(0.25)
                fa = a2.peek_folded()
                assert Cv.take_parked(y, fa) is None  # (and the parked output is gone from the link)
                if on:
                    y.grad_link.h_next = parked
                z, _ = b2(y, ys)
                a2.norm.bias.copy_(bias0)
            torch.cuda.synchronize()
            res[on] = z
    finally:
        with torch.no_grad():
            a2.norm.bias.copy_(bias0)
        for l in m.modules():
            if isinstance(l, bb.ConvNormLayer):
                l._w_folded = None
    _same_bits(res[True].contiguous().reshape(-1), res[False].contiguous().reshape(-1), "block 2 output")
    # ... and unchanged, block 2 does take it
    monkeypatch.setattr(Cv, "_CHAIN_ON", True)
    with torch.no_grad():
        m._fold_all()
        h = bb.stem_max_pool(m._stem(x), m.pool)
        y, ys = b1(h, None, a2)
        parked = y.grad_link.h_next
        assert parked is not None and Cv.take_parked(y, a2.peek_folded()) is parked[0]
    for l in m.modules():
        if isinstance(l, bb.ConvNormLayer):
            l._w_folded = None
