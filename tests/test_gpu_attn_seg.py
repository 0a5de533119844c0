"""Segment-masked HIP self-attention (csrc/attn.hip: rtdetr_attn_fwd_seg /
rtdetr_attn_bwd_seg) vs a plain PyTorch fp32 reference on the same bf16
inputs with the hidden scores set to -inf.

Mask rule: key k is visible to query q iff seg[k] < 0 or seg[k] == seg[q]
(seg: int32 [L], shared by all images and heads).  8 heads x 32 dims, q and k
read in place from one fused [B, L, 2d] projection output, inputs generated
as in tests/test_gpu_attn.py.

Tolerance (stated, that of tests/test_gpu_attn.py: the rounding structure is
the same, P and dS are rounded to bf16 before the second product): per
element |err| <= 2e-2 max|ref| and relative Frobenius error <= 1e-2 with the
same absolute floor.  Masked runs are bitwise repeatable, bitwise equal to
the unmasked kernels when nothing is hidden, and a group's rows do not
depend on another group's inputs bit for bit."""
from __future__ import annotations

import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, DH = 8, 32
D = H * DH


def _groups(n, size, shared):
    return [g for g in range(n) for _ in range(size)] + [-1] * shared


CASES = {
    "4x24+40": (2, 136, _groups(4, 24, 40)),
    "interleaved": (1, 7, [0, 0, 1, -1, -1, 1, 0]),
    "64+1": (2, 65, _groups(1, 64, 1)),
    "6x32+300": (1, 492, _groups(6, 32, 300)),
    "all-shared": (1, 130, [-1] * 130),
}


def _ref(qk, v, seg):
    B, L, _ = qk.shape
    q, k = qk.float().split(D, -1)
    heads = lambda t: t.reshape(B, L, H, DH).transpose(1, 2)  # noqa: E731
    s = heads(q) @ heads(k).transpose(-1, -2) / math.sqrt(DH)
    vis = (seg[None, :] < 0) | (seg[None, :] == seg[:, None])  # [query, key]
    s = s.masked_fill(~vis, float("-inf"))
    o = torch.softmax(s, -1) @ heads(v.float())
    return o.transpose(1, 2).reshape(B, L, D)


def _check(got, ref, what):
    got, ref = got.float(), ref.float()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    rel = ((got - ref).norm() / ref.norm().clamp(min=1e-30)).item()
    assert err <= 2e-2 * scale + 1e-6, f"{what}: max err {err:.3e} vs max|ref| {scale:.3e}"
    # relative Frobenius, with an absolute floor for outputs that vanish in exact
    # math (a query that sees only itself: dS = P (dP - delta) = 0, the kernel
    # returns rounding noise)
    assert (got - ref).norm().item() <= 1e-2 * ref.norm().item() + 1e-6 * got.numel() ** 0.5, \
        f"{what}: relative Frobenius {rel:.3e}"
    return rel


def _inputs(B, L, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    qk = (torch.randn(B, L, 2 * D, device=DEV, generator=g) * 1.5).to(torch.bfloat16)
    v = torch.randn(B, L, D, device=DEV, generator=g).to(torch.bfloat16)
    do = torch.randn(B, L, D, device=DEV, generator=g).to(torch.bfloat16)
    return qk, v, do


def _run(qk, v, do, seg):
    """(o, dqk, dv) of the HIP attention; seg None = the unmasked entry points."""
    from src.rtdetr_moe.linear import self_attention_hip

    a = qk.clone().requires_grad_(True)
    b = v.clone().requires_grad_(True)
    o = self_attention_hip(a, b, H, seg) if seg is not None else self_attention_hip(a, b, H)
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), a.grad, b.grad


def _seg(ids):
    return torch.tensor(ids, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("case", list(CASES))
def test_masked_attention_fwd_bwd_vs_fp32(hip_lib, case):
    B, L, ids = CASES[case]
    assert len(ids) == L
    seg = _seg(ids)
    qk, v, do = _inputs(B, L, B * 1000 + L)
    o, dqk, dv = _run(qk, v, do, seg)
    ra = qk.float().requires_grad_(True)
    rb = v.float().requires_grad_(True)
    ro = _ref(ra, rb, seg)
    ro.backward(do.float())
    _check(o, ro, "o")
    _check(dqk[..., :D], ra.grad[..., :D], "dq")
    _check(dqk[..., D:], ra.grad[..., D:], "dk")
    _check(dv, rb.grad, "dv")
    if case == "64+1":  # the shared query sees only itself: o = its v row
        assert torch.allclose(o[:, 64].float(), v[:, 64].float(), rtol=2 ** -7, atol=0)


@pytest.mark.parametrize("B,L", [(2, 65), (1, 300)])
def test_all_shared_is_bitwise_the_unmasked_attention(hip_lib, B, L):
    qk, v, do = _inputs(B, L, B * 1000 + L)
    o, dqk, dv = _run(qk, v, do, _seg([-1] * L))
    o0, dqk0, dv0 = _run(qk, v, do, None)
    assert torch.equal(o, o0) and torch.equal(dqk, dqk0) and torch.equal(dv, dv0)


def test_groups_are_isolated_bitwise(hip_lib):
    """Fresh inputs for group 1 (tokens 24..47) change no bit of any other
    token's o and dq, nor of dk and dv of the other groups' keys (seen by
    their own group only).  dk / dv of the shared keys, which group 1's
    queries see, may differ."""
    B, L, ids = CASES["4x24+40"]
    seg = _seg(ids)
    qk, v, do = _inputs(B, L, 1)
    o, dqk, dv = _run(qk, v, do, seg)
    qk2, v2, do2 = _inputs(B, L, 2)
    for t, t2 in ((qk, qk2), (v, v2), (do, do2)):
        t2[:, :24] = t[:, :24]
        t2[:, 48:] = t[:, 48:]
    assert not torch.equal(qk2[:, 24:48], qk[:, 24:48])
    o2, dqk2, dv2 = _run(qk2, v2, do2, seg)
    outside = torch.tensor([i for i in range(L) if ids[i] != 1], device=DEV)
    groups = torch.tensor([i for i in range(L) if ids[i] in (0, 2, 3)], device=DEV)
    assert torch.equal(o[:, outside], o2[:, outside])
    assert torch.equal(dqk[:, outside, :D], dqk2[:, outside, :D])
    assert torch.equal(dqk[:, groups, D:], dqk2[:, groups, D:])
    assert torch.equal(dv[:, groups], dv2[:, groups])
    assert not torch.equal(o[:, 24:48], o2[:, 24:48])  # the run did see the new inputs


@pytest.mark.parametrize("case", ["4x24+40", "interleaved"])
def test_masked_attention_is_repeatable(hip_lib, case):
    B, L, ids = CASES[case]
    seg = _seg(ids)
    qk, v, do = _inputs(B, L, 3)
    o, dqk, dv = _run(qk, v, do, seg)
    o2, dqk2, dv2 = _run(qk, v, do, seg)
    assert torch.equal(o, o2) and torch.equal(dqk, dqk2) and torch.equal(dv, dv2)


def test_seg_argument_checks(hip_lib):
    """A NULL seg is refused by the entry points and a CPU (or mis-typed,
    mis-sized) seg by the binding, before any launch."""
    from src.moe import _lib as L
    from src.rtdetr_moe.linear import self_attention_hip

    B, T = 1, 7
    qk, v, do = _inputs(B, T, 4)
    o = torch.empty_like(v)
    lse = torch.empty(B, H, T, dtype=torch.float32, device=DEV)
    fwd = (qk.data_ptr(), 2 * D, qk.data_ptr() + 2 * D, 2 * D, v.data_ptr(), D, o.data_ptr(), D, lse.data_ptr(),
           B, H, T, DH, 1.0 / math.sqrt(DH), L._stream())
    assert L.lib().rtdetr_attn_fwd_seg(*fwd, None) != 0
    assert b"seg" in L.lib().moe_last_error()
    dqk, dv, delta = torch.empty_like(qk), torch.empty_like(v), torch.empty_like(lse)
    bwd = (qk.data_ptr(), 2 * D, qk.data_ptr() + 2 * D, 2 * D, v.data_ptr(), D, o.data_ptr(), D, do.data_ptr(), D,
           lse.data_ptr(), delta.data_ptr(), dqk.data_ptr(), 2 * D, dqk.data_ptr() + 2 * D, 2 * D, dv.data_ptr(), D,
           B, H, T, DH, 1.0 / math.sqrt(DH), L._stream())
    assert L.lib().rtdetr_attn_bwd_seg(*bwd, None) != 0
    assert b"seg" in L.lib().moe_last_error()
    ids = [0, 0, 1, -1, -1, 1, 0]
    for bad in (torch.tensor(ids, dtype=torch.int32),                    # on the CPU
                torch.tensor(ids, dtype=torch.int64, device=DEV),        # wrong dtype
                torch.tensor(ids + [0], dtype=torch.int32, device=DEV)):  # wrong length
        with pytest.raises(L.MoEKernelError):
            self_attention_hip(qk, v, H, bad)
    torch.cuda.synchronize()
