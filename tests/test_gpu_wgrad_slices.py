"""The convolution weight gradient's two A/B paths (csrc/conv.hip) are bitwise
one another: the slice sums with the threads laid along the row
(rtdetr_conv_set_tuning "conv_wg_reduce" 1) against the 16 x 16 layout (0),
and the partial tile stored as whole rows through LDS ("conv_wg_stage" 1)
against the stores from the accumulator fragments (0).

Every comparison is torch.equal of the raw bits (a NaN equals itself) against
the = 0 path of the same build, on the same inputs.

Reduce: nsplit over every path of the wide kernel (4 columns per thread up to
4 slices, 2 up to 8, 1 up to 32 in one and two rounds of 16, four waves
sharing the groups above that: whole rounds, a ragged last one, 255 / 256), n with
a partial last block, a weight smaller than one block and n % 4 == 0 only;
partials holding -0.0 (alone in its column: the sum is +0.0), +-inf, inf - inf
and NaN; a batch of 1, 2 and 48 descriptors of mixed nsplit and n against
batches of one; a sentinel behind every dw.

Stores: rtdetr_conv_wgrad_part over every tile instance ((C, N) over
{64, 128, 256}^2, KS 1 and 3, stride 1 and 2) at P = 35, 234, 1,152 and 4,264
pixels with 1 slice, more slices than K-tiles (the empty ones write zeros)
and the automatic count, over a part filled with garbage, a sentinel behind
it, two runs.

Model: the 52 parameter gradients of a PResNet-50 at 2 x 64 x 96 with both
keys 0 and both 1, with and without deferred_wgrads, eager and as a captured
graph replayed on two inputs."""
from __future__ import annotations

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
_KEYS = ("conv_wg_reduce", "conv_wg_stage")
_SENT = 12345.0


@pytest.fixture(autouse=True)
def _default_keys(hip_lib):
    """Every test leaves both keys at the build's defaults (1)."""
    yield
    for k in _KEYS:
        hip_lib.rtdetr_conv_set_tuning(k.encode(), 1)


def _set(hip_lib, reduce=None, stage=None):
    if reduce is not None:
        assert hip_lib.rtdetr_conv_set_tuning(b"conv_wg_reduce", reduce) == 0
    if stage is not None:
        assert hip_lib.rtdetr_conv_set_tuning(b"conv_wg_stage", stage) == 0


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), what


def _partials(nsplit, n, seed):
    """[nsplit][n] fp32 with the special values in columns spread over the row, the last element included."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.randn(nsplit, n, device=DEV, generator=g)
    k = nsplit // 2
    p[:, 0] = -0.0                   # -0.0 in every slice: sixteen +0.0f starts make it +0.0
    p[k, 1] = float("inf")
    p[:, 2] = float("nan")           # a NaN column
    if n > 4:
        p[k, n - 1] = float("-inf")
        p[0, n - 2] = float("inf")   # inf - inf where the column has two slices
        p[nsplit - 1, n - 2] = float("-inf")
        p[k, n // 2] = -0.0
        p[nsplit - 1, n // 2 + 1] = float("nan")
    return p.contiguous()


def _reduce_batch(descs, out_bf16):
    """rtdetr_conv_wgrad_reduce_batch over descs = [(part [nsplit][n], nsplit, n)]: the dws and their sentinels."""
    from src.moe import _lib as L

    dt = torch.bfloat16 if out_bf16 else torch.float32
    bufs = [torch.full((n + 64,), _SENT, dtype=dt, device=DEV) for _, _, n in descs]
    m = len(descs)
    cv = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    parts = (ctypes.c_void_p * m)(*[d[0].data_ptr() for d in descs])
    ns = (ctypes.c_int * m)(*[d[1] for d in descs])
    nw = (ctypes.c_longlong * m)(*[d[2] for d in descs])
    dws = (ctypes.c_void_p * m)(*[b.data_ptr() for b in bufs])
    L._check(L.lib().rtdetr_conv_wgrad_reduce_batch(m, cv(parts), cv(ns), cv(nw), cv(dws), int(out_bf16),
                                                    L._stream()), "rtdetr_conv_wgrad_reduce_batch")
    torch.cuda.synchronize()
    for b, (_, _, n) in zip(bufs, descs):
        assert bool((b[n:] == _SENT).all()), "the reduction wrote behind dw"
    return [b[:n] for b, (_, _, n) in zip(bufs, descs)]


_NS = [4, 60, 64, 68, 4096 + 4, 64 * 64 * 9]


@pytest.mark.parametrize("nsplit", [1, 2, 3, 8, 14, 15, 16, 17, 32, 56, 255, 256])
def test_reduce_wide_matches_groups(hip_lib, nsplit):
    for n in _NS:
        p = _partials(nsplit, n, nsplit * 131 + n)
        for out_bf16 in (True, False):
            _set(hip_lib, reduce=0)
            ref = _reduce_batch([(p, nsplit, n)], out_bf16)[0]
            _set(hip_lib, reduce=1)
            got = _reduce_batch([(p, nsplit, n)], out_bf16)[0]
            _same(got, ref, f"nsplit {nsplit} n {n} bf16 {out_bf16}")
            # the special columns came out as the sums say
            f = got.float()
            assert f[0].item() == 0.0 and not torch.signbit(f[0]).item()
            assert torch.isnan(f[2]).item() and (torch.isinf(f[1]).item() and f[1].item() > 0)
            if n > 4:
                assert f[n - 1].item() == float("-inf")
                assert torch.isnan(f[n - 2]).item() == (nsplit > 1)


@pytest.mark.parametrize("count", [1, 2, 48])
@pytest.mark.parametrize("out_bf16", [True, False])
def test_reduce_batch_mixed_descriptors(hip_lib, count, out_bf16):
    """A batch of mixed nsplit and n == its weights reduced one by one (batches of one), under both layouts,
    and the wide batch == the 16 x 16 batch."""
    splits = [3, 256, 8, 14, 1, 17, 56, 2, 16, 32, 15, 255]
    descs = []
    for q in range(count):
        ns, n = splits[q % len(splits)], _NS[(q * 5 + q // 6) % len(_NS)]
        descs.append((_partials(ns, n, 7 * q + 1), ns, n))
    outs = {}
    for mode in (0, 1):
        _set(hip_lib, reduce=mode)
        outs[mode] = _reduce_batch(descs, out_bf16)
        for d, got in zip(descs, outs[mode]):
            _same(got, _reduce_batch([d], out_bf16)[0], f"mode {mode} nsplit {d[1]} n {d[2]}")
    for d, a, b in zip(descs, outs[0], outs[1]):
        _same(b, a, f"nsplit {d[1]} n {d[2]}")


def _wgrad_part(x, gy, C, N, ks, st, nsplit):
    """rtdetr_conv_wgrad_part into a garbage-filled part with a sentinel behind it."""
    from src.moe import _lib as L
    from src.rtdetr_moe.conv import _zero

    B, H, W = x.shape[0], x.shape[2], x.shape[3]
    nw = N * ks * ks * C
    buf = torch.full((nsplit * nw + 256,), _SENT, dtype=torch.float32, device=DEV)
    L._check(L.lib().rtdetr_conv_wgrad_part(gy.data_ptr(), x.data_ptr(), buf.data_ptr(), nsplit,
                                            _zero(x.device).data_ptr(), B, H, W, C, N, ks, st, L._stream()),
             "rtdetr_conv_wgrad_part")
    torch.cuda.synchronize()
    assert bool((buf[nsplit * nw:] == _SENT).all()), "the slices wrote behind part"
    return buf[:nsplit * nw].view(nsplit, nw)


@pytest.mark.parametrize("B,H,W", [(1, 5, 7), (2, 9, 13), (3, 16, 24), (2, 41, 52)])
@pytest.mark.parametrize("ks,st", [(1, 1), (3, 1), (3, 2)])
def test_staged_stores_match_fragment_stores(hip_lib, B, H, W, ks, st):
    g = torch.Generator(device=DEV).manual_seed(B * H * W + ks + st)
    Ho, Wo = (H - 1) // st + 1, (W - 1) // st + 1
    ktot = (B * Ho * Wo + 63) // 64
    for C in (64, 128, 256):
        x = torch.randn(B, C, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last)
        for N in (64, 128, 256):
            gy = torch.randn(B, N, Ho, Wo, device=DEV, generator=g).to(torch.bfloat16).contiguous(
                memory_format=torch.channels_last)
            auto = hip_lib.rtdetr_conv_wgrad_splits(B, Ho, Wo, C, N, ks)
            for nsplit in sorted({1, ktot + 3, auto}):
                what = f"C {C} N {N} nsplit {nsplit}"
                _set(hip_lib, stage=0)
                ref = _wgrad_part(x, gy, C, N, ks, st, nsplit)
                _set(hip_lib, stage=1)
                got = _wgrad_part(x, gy, C, N, ks, st, nsplit)
                _same(got, ref, what)
                _same(_wgrad_part(x, gy, C, N, ks, st, nsplit), got, what + " (second run)")
                if nsplit > ktot:  # a slice past the last K-tile holds zeros, not the garbage it was given
                    assert not bool(got[ktot:].any()), what


def _backbone():
    from src.rtdetr_moe.backbone import PResNet

    torch.manual_seed(0)
    m = PResNet(50).to(DEV).to(torch.bfloat16).to(memory_format=torch.channels_last)
    for mod in m.modules():
        if hasattr(mod, "running_var") and not isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_var.uniform_(0.5, 2.0)
            mod.weight.uniform_(0.5, 1.5)
    xs = [torch.randn(2, 3, 64, 96, device=DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
          for _ in range(2)]
    return m, xs, [p for p in m.parameters() if p.requires_grad]


def _grads(m, x, params, defer):
    from src.rtdetr_moe import conv as Cv

    outs = m(x)
    loss = sum((o.float() * torch.linspace(-1, 1, o.numel(), device=DEV).view_as(o)).sum() for o in outs)
    with Cv.deferred_wgrads(enabled=defer):
        return torch.autograd.grad(loss, params, allow_unused=True)


def _compare_grads(ref, got, what):
    n = 0
    for a, b in zip(ref, got):
        assert (a is None) == (b is None), what
        if a is not None:
            _same(b, a, what)
            n += 1
    assert n == 52, n


@pytest.mark.parametrize("defer", [False, True])
def test_backbone_gradients_bitwise_eager(hip_lib, defer):
    m, xs, params = _backbone()
    res = {}
    for mode in (0, 1):
        _set(hip_lib, reduce=mode, stage=mode)
        grads = _grads(m, xs[0], params, defer)
        torch.cuda.synchronize()
        res[mode] = [None if g is None else g.clone() for g in grads]
    _compare_grads(res[0], res[1], f"defer {defer}")


@pytest.mark.parametrize("defer", [False, True])
def test_backbone_gradients_bitwise_graph(hip_lib, defer):
    """Both keys 1 captured in a hipGraph and replayed on two inputs == both keys 0, eager."""
    m, xs, params = _backbone()
    _set(hip_lib, reduce=0, stage=0)
    refs = []
    for x in xs:
        grads = _grads(m, x, params, defer)
        torch.cuda.synchronize()
        refs.append([None if g is None else g.clone() for g in grads])
    _set(hip_lib, reduce=1, stage=1)
    static = xs[0].clone(memory_format=torch.channels_last)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _grads(m, static, params, defer)  # first use outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        grads = _grads(m, static, params, defer)
    for i in (1, 0):
        static.copy_(xs[i])
        g.replay()
        torch.cuda.synchronize()
        _compare_grads(refs[i], grads, f"defer {defer}, input {i}")
