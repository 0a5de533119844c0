"""The HIP attention's C ABI (csrc/attn.hip: rtdetr_attn_fwd / _bwd and their
_seg instances, called raw through ctypes) against the float64 reference of
tests/attn_cases.py: any H, a padded row stride of its own for every operand,
q and k in separate buffers, five scales, peaked and ramped scores, exact
one-hot and uniform rows, segment ids at the tile edges, lse and delta as
outputs, and every refusal of attn_check that can be tried without leaving
the buffers.

Every launch here writes into buffers whose unused columns (>= 32 H), two
spare rows and spare lse / delta elements hold a NaN bit pattern, runs twice,
and is checked for: guards bitwise unchanged, q, k, v, o, dout bitwise
unchanged by the backward, the second run's bits equal to the first's.  A
misaddressed read lands on a NaN.

Tolerance of the statistical cases.  Each of o, dq, dk, dv, lse, delta is
compared with ref64 over the whole tensor and over every (image, head) slice,
as Frobenius error and as max error.  Limit = MARGIN x emul64's figure for the
same case, slice and measure + an absolute floor per element: half a bf16 ulp
of the slice's max |ref| for the bf16 outputs, 4 fp32 ulp of it for lse and
delta, plus, for dq and dk, zero_bounds (below).  MARGIN = 4 is assumed, as in
test_gpu_criterion_edges.py: emul64 has the kernels' roundings, and the
kernels add the online-softmax rescale and another fp32 summation order.

zero_bounds, used as the whole limit where dq and dk vanish in exact math (the
one-hot rows): dP = dout . v is a 32-term fp32 dot product on the MFMA and
delta = dout . o another on the vector unit; with faithful rounding (unit
2^-23; the MFMA's internal rounding is not documented as round-to-nearest)
each is off by at most 32 x 2^-23 x sum |terms|.  P <= 1 + 2^-15 multiplies
the difference, bf16 rounding of dS adds a factor 1 + 2^-9, so
  |dq_i| <= |scale| (1 + 2^-8) sum_j P_ij 2^-18 (|dout_i|.|v_j| + |dout_i|.|o_i|) |k_j|
and the same with q_i summed over i for dk_j.  For the one-hot table this is
about 1e-4 against gradients that would be O(10) if P, delta or the key
permutation were wrong.

Measured on an MI355X: largest kernel figure / limit over all slices and both
measures, per case and output (ATTN_REPORT=<file> writes these lines):

  case                     o     dq     dk     dv    lse  delta
  layout_B1H1L1         0.00   0.00   0.00   0.00   0.13   0.08
  layout_B3H3L15        0.21   0.22   0.23   0.22   0.11   0.25
  layout_B1H8L16        0.20   0.22   0.22   0.21   0.20   0.25
  layout_B3H1L17        0.19   0.22   0.22   0.21   0.09   0.25
  layout_B1H3L63        0.21   0.22   0.21   0.21   0.12   0.25
  layout_B3H8L64        0.21   0.22   0.22   0.22   0.15   0.25
  layout_B1H1L65        0.17   0.21   0.21   0.20   0.14   0.25
  layout_B3H3L127       0.21   0.21   0.32   0.22   0.18   0.34
  layout_B1H8L128       0.20   0.25   0.24   0.22   0.13   0.27
  layout_B3H1L129       0.21   0.22   0.21   0.22   0.14   0.26
  layout_B1H3L193       0.20   0.21   0.22   0.21   0.17   0.25
  scale_rsqrt32         0.20   0.23   0.20   0.22   0.16   0.26
  scale_one             0.20   0.23   0.23   0.21   0.17   0.25
  scale_2^-5            0.21   0.22   0.21   0.21   0.15   0.25
  scale_-0.5            0.20   0.22   0.22   0.21   0.13   0.26
  scale_zero            0.20   0.00   0.00   0.20   0.00   0.25
  peaked_x4_L65         0.20   0.23   0.23   0.20   0.14   0.25
  peaked_x8_L129        0.20   0.28   0.28   0.21   0.15   0.29
  peaked_x8_L193        0.20   0.23   0.24   0.18   0.18   0.25
  ramp_up               0.22   0.27   0.18   0.21   0.12   0.34
  ramp_down             0.22   0.24   0.20   0.22   0.12   0.25
  ramp_last             0.10   0.25   0.09   0.19   0.15   0.25
  seg_distinct          0.00   0.01   0.01   0.00   0.11   0.11
  seg_special           0.20   0.23   0.23   0.21   0.14   0.28
  seg_late              0.20   0.22   0.22   0.21   0.08   0.25
  seg_shared            0.21   0.22   0.22   0.22   0.16   0.26

0.25 is a kernel figure equal to emul64's own.  The worst row, delta of ramp_up
and of layout_B3H3L127, is at 0.34 of its limit: 1.4 x emul64's error against a
margin of 4.  One-hot rows: |dq|, |dk| <= 1.4e-6 against bounds of 3.7e-4 to
4.6e-4; o, dv and lse exact.
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN16 = 0x7FB7        # a bf16 NaN: guard columns and rows
NAN32 = 0x7FB7A5A5    # an fp32 NaN: spare lse / delta elements
GUARD_ROWS = 2
SPARE = 8


class _Buf:
    """rows x cols bf16 at row stride ld, two guard rows behind; everything NAN16 until written."""

    def __init__(self, rows, cols, ld, data=None):
        assert ld >= cols
        self.rows, self.cols, self.ld = rows, cols, ld
        self.raw = torch.full(((rows + GUARD_ROWS) * ld,), NAN16, dtype=torch.int16, device=DEV)
        if data is not None:
            self.logical().copy_(data.reshape(rows, cols).contiguous().view(torch.int16))

    def logical(self):
        return self.raw[:self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    def ptr(self, col=0):
        return self.raw.data_ptr() + 2 * col

    def read(self, B, L, col, d):
        return self.logical()[:, col:col + d].cpu().contiguous().view(torch.bfloat16).reshape(B, L, d)

    def guards_intact(self):
        t = self.raw.clone()
        t[:self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = NAN16
        return bool((t == NAN16).all())

    def untouched(self):
        return bool((self.raw == NAN16).all())


class _Setup:
    """Device buffers of one case: ``at[name] = (buffer, first column)`` for
    each of attn_cases.BUFFERS, lse and delta [B H L + SPARE] fp32, seg."""

    def __init__(self, case, packed=False, lds=None):
        B, H, L = case.shape
        d = ac.DH * H
        rows = B * L
        self.case, self.B, self.H, self.L, self.d = case, B, H, L, d
        self.lds = dict(ac.packed_lds(H) if packed else (lds or case.lds))
        ld = self.lds
        if packed:
            qk = _Buf(rows, 2 * d, 2 * d, torch.cat([case.q, case.k], -1))
            dqk = _Buf(rows, 2 * d, 2 * d)
            self.at = dict(q=(qk, 0), k=(qk, d), dq=(dqk, 0), dk=(dqk, d))
        else:
            self.at = dict(q=(_Buf(rows, d, ld["q"], case.q), 0), k=(_Buf(rows, d, ld["k"], case.k), 0),
                           dq=(_Buf(rows, d, ld["dq"]), 0), dk=(_Buf(rows, d, ld["dk"]), 0))
        self.at.update(v=(_Buf(rows, d, ld["v"], case.v), 0), do=(_Buf(rows, d, ld["do"], case.dout), 0),
                       o=(_Buf(rows, d, ld["o"]), 0), dv=(_Buf(rows, d, ld["dv"]), 0))
        self.n = B * H * L
        self.lse = torch.full((self.n + SPARE,), NAN32, dtype=torch.int32, device=DEV)
        self.delta = torch.full((self.n + SPARE,), NAN32, dtype=torch.int32, device=DEV)
        self.seg = None if case.seg is None else torch.tensor(case.seg, dtype=torch.int32, device=DEV)

    def ptr(self, name, off=0):
        if name in ("lse", "delta"):
            return getattr(self, name).data_ptr() + off
        buf, col = self.at[name]
        return buf.ptr(col) + off

    def fwd_args(self, off=None, **over):
        from src.moe import _lib

        p = lambda n: self.ptr(n, (off or {}).get(n, 0))  # noqa: E731
        ld = dict(self.lds, **over.get("lds", {}))
        return (p("q"), ld["q"], p("k"), ld["k"], p("v"), ld["v"], p("o"), ld["o"], p("lse"),
                over.get("B", self.B), over.get("H", self.H), over.get("L", self.L), over.get("head_dim", ac.DH),
                over.get("scale", self.case.scale), _lib._stream())

    def bwd_args(self, off=None, **over):
        from src.moe import _lib

        p = lambda n: self.ptr(n, (off or {}).get(n, 0))  # noqa: E731
        ld = dict(self.lds, **over.get("lds", {}))
        return (p("q"), ld["q"], p("k"), ld["k"], p("v"), ld["v"], p("o"), ld["o"], p("do"), ld["do"], p("lse"),
                p("delta"), p("dq"), ld["dq"], p("dk"), ld["dk"], p("dv"), ld["dv"],
                over.get("B", self.B), over.get("H", self.H), over.get("L", self.L), over.get("head_dim", ac.DH),
                over.get("scale", self.case.scale), _lib._stream())

    def buffers(self):
        return {id(b): b for b, _ in self.at.values()}.values()

    def outputs_untouched(self):
        outs = {id(self.at[n][0]): self.at[n][0] for n in ("o", "dq", "dk", "dv")}.values()
        return all(b.untouched() for b in outs) and bool((self.lse == NAN32).all() and (self.delta == NAN32).all())

    def read(self, name):
        if name in ("lse", "delta"):
            return getattr(self, name)[:self.n].cpu().view(torch.float32).reshape(self.B, self.H, self.L)
        buf, col = self.at[name]
        return buf.read(self.B, self.L, col, self.d)


def _launch(case, packed=False, masked=None):
    """One forward and one backward through the raw entry points (the _seg ones
    when the case has ids, unless masked=False) -> {output: CPU tensor}, after
    the guard and read-only checks of this launch."""
    from src.moe import _lib

    lib = _lib.lib()
    s = _Setup(case, packed)
    masked = (case.seg is not None) if masked is None else masked
    tail = (s.seg.data_ptr(),) if masked else ()
    fwd, bwd = (lib.rtdetr_attn_fwd_seg, lib.rtdetr_attn_bwd_seg) if masked else (lib.rtdetr_attn_fwd,
                                                                                    lib.rtdetr_attn_bwd)
    _lib._check(fwd(*s.fwd_args(), *tail), "forward")
    torch.cuda.synchronize()
    before = {n: s.at[n][0].raw.clone() for n in ("q", "k", "v", "o", "do")}
    lse_before = s.lse.clone()
    _lib._check(bwd(*s.bwd_args(), *tail), "backward")
    torch.cuda.synchronize()
    for n, t in before.items():
        assert torch.equal(s.at[n][0].raw, t), f"{case.name}: the backward wrote into {n}"
    assert torch.equal(s.lse, lse_before), f"{case.name}: the backward wrote into lse"
    for n in ac.BUFFERS:
        assert s.at[n][0].guards_intact(), f"{case.name}: guard columns / rows of {n} were written"
    for n in ("lse", "delta"):
        assert bool((getattr(s, n)[s.n:] == NAN32).all()), f"{case.name}: spare elements of {n} were written"
    return {n: s.read(n) for n in ac.OUTPUTS}


def _same_bits(a, b, what, names=ac.OUTPUTS):
    for n in names:
        x, y = a[n], b[n]
        if x.dtype == torch.bfloat16:
            x, y = x.view(torch.int16), y.view(torch.int16)
        else:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), f"{what}: {n} differs"


_RESULTS = {}


def _run(case, packed=False, masked=None):
    """_launch twice, the same bits both times; one result per (case, layout) for the module."""
    key = (case.name, packed, masked)
    if key not in _RESULTS:
        first = _launch(case, packed, masked)
        _same_bits(first, _launch(case, packed, masked), f"{case.name}: second launch")
        _RESULTS[key] = first
    return _RESULTS[key]


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


# ---------------------------------------------------------------------------
# statistical cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.STATISTICAL_NAMES)
def test_outputs_match_fp64(hip_lib, name):
    case = ac.cases()[name]
    B, H, L = case.shape
    got = _run(case)
    ref, efig, lim = ac.case_reference(name)
    fig = ac.figures(tuple(got[n] for n in ac.OUTPUTS), ref, B, H)
    ratio = ac.worst_ratio(fig, lim)
    rel = ac.relative(fig, ref)
    ac.report({"case": name, "side": "kernel", "ratio": {n: ratio[n][0] for n in ac.OUTPUTS},
               "where": {n: ratio[n][1] for n in ac.OUTPUTS}, "relative": rel})
    print(name, {n: f"{ratio[n][0]:.2f} ({ratio[n][1]})" for n in ac.OUTPUTS}, "relative", rel)
    for n in ac.OUTPUTS:
        assert ratio[n][0] <= 1.0, f"{name} {n}: kernel error {ratio[n][0]:.2f} x its limit at {ratio[n][1]}"


# ---------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.names_of("onehot"))
def test_onehot_rows_are_exact(hip_lib, name):
    case = ac.cases()[name]
    B, H, L = case.shape
    pi = list(case.pi)
    got = _run(case)
    assert torch.equal(_bits(got["o"]), _bits(case.v[:, pi])), "o[i] != v[pi(i)]"
    assert torch.equal(_bits(got["dv"][:, pi]), _bits(case.dout)), "dv[pi(i)] != dout[i]"
    # lse = the fp32 product of the (integer) score and the fp32 product scale * log2(e); log2f(1) = 0
    want = np.float32(2048.0) * (np.float32(case.scale) * np.float32(ac.LOG2E))
    lse = got["lse"].numpy()
    assert lse.dtype == np.float32 and (lse == want).all(), (float(want), float(lse.min()), float(lse.max()))
    ref = ac.ref64(*case.operands())
    zq, zk = ac.zero_bounds(*case.operands())
    assert float(zq.max()) < 1e-3 and float(zk.max()) < 1e-3
    dq, dk = got["dq"].double().abs(), got["dk"].double().abs()
    print(name, "dq", float(dq.max()), "bound", float(zq.max()), "dk", float(dk.max()), "bound", float(zk.max()))
    assert bool((dq <= zq).all()), f"|dq| up to {float(dq.max()):.3e}, bound {float(zq.max()):.3e}"
    assert bool((dk <= zk).all()), f"|dk| up to {float(dk.max()):.3e}, bound {float(zk.max()):.3e}"
    # delta: the fp32 dot product dout . o with o = v[pi] exact
    bound = ac.GAMMA32 * (ac.heads(case.dout.double()).abs() * ac.heads(ref[0]).abs()).sum(-1)
    assert bool(((got["delta"].double() - ref[5]).abs() <= bound).all())
    ac.report({"case": name, "side": "kernel", "dq_max": float(dq.max()), "dq_bound": float(zq.max()),
               "dk_max": float(dk.max()), "dk_bound": float(zk.max())})


def _ulp_bf16(t):
    """Elementwise bf16 ulp of |t| (float64), 0 at 0."""
    a = t.abs()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp(min=1e-300))) - 7), torch.zeros_like(a))


@pytest.mark.parametrize("name", ac.names_of("uniform"))
def test_uniform_rows(hip_lib, name):
    case = ac.cases()[name]
    B, H, L = case.shape
    got = _run(case)
    lse = got["lse"].double()
    assert float((lse - math.log2(L)).abs().max()) <= ac.F32_FLOOR_ULPS * ac.ulp_f32(math.log2(L))
    if case.scale == 0.0:
        assert float(got["dq"].float().abs().max()) == 0.0 and float(got["dk"].float().abs().max()) == 0.0
        return
    want = ac.bf16r(case.v.double().sum(1, keepdim=True) / L).expand(B, L, -1)
    assert bool(((got["o"].double() - want).abs() <= _ulp_bf16(want)).all()), "o: padding keys counted?"
    assert float(got["dk"].float().abs().max()) == 0.0  # q = 0


def test_distinct_segments_copy_their_own_row(hip_lib):
    case = ac.cases()["seg_distinct"]
    got = _run(case)
    assert torch.equal(_bits(got["o"]), _bits(case.v)) and torch.equal(_bits(got["dv"]), _bits(case.dout))
    zq, zk = ac.zero_bounds(*case.operands())
    assert bool((got["dq"].double().abs() <= zq).all() and (got["dk"].double().abs() <= zk).all())


def test_all_shared_is_bitwise_the_unmasked_attention(hip_lib):
    """At padded strides and H = 3."""
    case = ac.cases()["seg_shared"]
    assert case.shape[1] == 3 and all(i < 0 for i in case.seg)
    _same_bits(_run(case), _run(case, masked=False), "all-shared vs unmasked")


# ---------------------------------------------------------------------------
# addressing does not change the arithmetic
# ---------------------------------------------------------------------------
EQUIVALENCE = ["layout_B3H8L64", "layout_B1H3L193", "layout_B3H1L129", "scale_rsqrt32", "seg_special", "seg_late"]


@pytest.mark.parametrize("name", EQUIVALENCE)
def test_binding_packed_and_padded_give_the_same_bits(hip_lib, name):
    from src.rtdetr_moe.linear import self_attention_hip

    case = ac.cases()[name]
    assert case.scale == ac.SCALE0  # the binding's scale
    B, H, L = case.shape
    d = ac.DH * H
    padded, packed = _run(case), _run(case, packed=True)
    _same_bits(padded, packed, f"{name}: padded vs packed")
    qk = torch.cat([case.q, case.k], -1).to(DEV).requires_grad_(True)
    v = case.v.to(DEV).requires_grad_(True)
    seg = None if case.seg is None else torch.tensor(case.seg, dtype=torch.int32, device=DEV)
    o = self_attention_hip(qk, v, H, seg)
    o.backward(case.dout.to(DEV))
    torch.cuda.synchronize()
    bound = dict(o=o.detach().cpu(), dq=qk.grad[..., :d].cpu(), dk=qk.grad[..., d:].cpu(), dv=v.grad.cpu())
    _same_bits(bound, packed, f"{name}: self_attention_hip vs raw", names=ac.BF16_OUTPUTS)


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def _refusal_case():
    return ac.cases()["layout_B3H3L15"]


def _roomy_lds(case):
    """Strides 8 elements above the case's: a launch at any stride passed below stays inside."""
    return {n: ld + 8 for n, ld in case.lds.items()}


FWD_PTRS = ("q", "k", "v", "o", "lse")
BWD_PTRS = ("q", "k", "v", "o", "do", "lse", "delta", "dq", "dk", "dv")
FWD_LDS = ("q", "k", "v", "o")
# (id, overrides, word of the message).  Were a check missing: head_dim is not
# used by the kernels; B < 0 is tried with L = 0, L < 0 and H < 0 with B = 0, which
# then return before the launch; H = 0 makes an empty grid, which cannot launch.
REFUSED_SHAPES = [("head_dim16", dict(head_dim=16), "head_dim"), ("head_dim64", dict(head_dim=64), "head_dim"),
                  ("B<0", dict(B=-1, L=0), "bad B"), ("L<0", dict(L=-1, B=0), "bad B"),
                  ("H=0", dict(H=0), "bad B"), ("H<0", dict(H=-1, B=0), "bad B")]


def _refused(fn, args, setup, word, entry):
    from src.moe import _lib

    before = _lib.launch_counts().get("attention", 0)
    rc = fn(*args)
    torch.cuda.synchronize()
    msg = _lib.lib().moe_last_error() or b""
    assert rc != 0, f"{entry}: accepted"
    assert entry.encode() + b":" in msg and word.encode() in msg, msg
    assert _lib.launch_counts().get("attention", 0) == before, f"{entry}: launched"
    assert setup.outputs_untouched(), f"{entry}: wrote its outputs"


def _entries(masked):
    from src.moe import _lib

    lib = _lib.lib()
    return ((lib.rtdetr_attn_fwd_seg, lib.rtdetr_attn_bwd_seg, "rtdetr_attn_fwd_seg", "rtdetr_attn_bwd_seg") if masked
            else (lib.rtdetr_attn_fwd, lib.rtdetr_attn_bwd, "rtdetr_attn_fwd", "rtdetr_attn_bwd"))


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "seg"])
def test_refusals(hip_lib, masked):
    case = _refusal_case()
    B, H, L = case.shape
    s = _Setup(case, lds=_roomy_lds(case))
    seg = torch.full((L,), -1, dtype=torch.int32, device=DEV)
    tail = (seg.data_ptr(),) if masked else ()
    fwd, bwd, fname, bname = _entries(masked)
    for _, over, word in REFUSED_SHAPES:
        _refused(fwd, s.fwd_args(**over) + tail, s, word, fname)
        _refused(bwd, s.bwd_args(**over) + tail, s, word, bname)
    for n in ac.BUFFERS:
        for bad in (case.lds[n] + 4, ac.DH * H - 8):  # not a multiple of 8; below 32 H
            assert bad <= s.lds[n]
            if n in FWD_LDS:
                _refused(fwd, s.fwd_args(lds={n: bad}) + tail, s, "row strides", fname)
            _refused(bwd, s.bwd_args(lds={n: bad}) + tail, s, "row strides", bname)
    for n in BWD_PTRS:  # 8 bytes off a 16-byte boundary; the guard rows and spare elements hold the overhang
        assert s.ptr(n) % 16 == 0
        if n in FWD_PTRS:
            _refused(fwd, s.fwd_args(off={n: 8}) + tail, s, "16-B aligned", fname)
        _refused(bwd, s.bwd_args(off={n: 8}) + tail, s, "16-B aligned", bname)


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "seg"])
def test_empty_batch_and_empty_sequence_are_no_ops(hip_lib, masked):
    from src.moe import _lib

    case = _refusal_case()
    s = _Setup(case)
    seg = torch.full((case.shape[2],), -1, dtype=torch.int32, device=DEV)
    tail = (seg.data_ptr(),) if masked else ()
    fwd, bwd, _, _ = _entries(masked)
    before = _lib.launch_counts().get("attention", 0)
    for over in (dict(B=0), dict(L=0), dict(B=0, L=0)):
        assert fwd(*s.fwd_args(**over), *tail) == 0
        assert bwd(*s.bwd_args(**over), *tail) == 0
    torch.cuda.synchronize()
    assert _lib.launch_counts().get("attention", 0) == before
    assert s.outputs_untouched()


# ---------------------------------------------------------------------------
# the Python binding
# ---------------------------------------------------------------------------
def test_binding_refuses_other_head_dims(hip_lib):
    from src.rtdetr_moe.linear import self_attention_hip

    for d, H in ((64, 4), (64, 1), (96, 2), (32, 2)):  # head dims 16, 64, 48, 16
        qk = torch.zeros(1, 4, 2 * d, dtype=torch.bfloat16, device=DEV)
        v = torch.zeros(1, 4, d, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(ValueError):
            self_attention_hip(qk, v, H)


def _bound(qk, v, do, H):
    from src.rtdetr_moe.linear import self_attention_hip

    a, b = qk.detach().requires_grad_(True), v.detach().requires_grad_(True)
    o = self_attention_hip(a, b, H)
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), a.grad, b.grad


def test_binding_takes_fp32_and_non_contiguous_inputs(hip_lib):
    """fp32 inputs with values beyond bf16 and transposed (non-contiguous) inputs
    give the bits of their contiguous bf16 copies; gradients in the input dtype."""
    B, H, L = 2, 3, 65
    d = ac.DH * H
    g = torch.Generator().manual_seed(77)
    qk32 = (torch.randn(L, B, 2 * d, generator=g) * 1.5).to(DEV).transpose(0, 1)  # [B, L, 2d], not contiguous
    v32 = torch.randn(L, B, d, generator=g).to(DEV).transpose(0, 1)
    do32 = torch.randn(L, B, d, generator=g).to(DEV).transpose(0, 1)
    assert not qk32.is_contiguous() and not v32.is_contiguous() and not do32.is_contiguous()
    assert not torch.equal(qk32, qk32.to(torch.bfloat16).float())  # rounding does happen
    qk16, v16, do16 = (t.to(torch.bfloat16).contiguous() for t in (qk32, v32, do32))
    o0, dqk0, dv0 = _bound(qk16, v16, do16, H)
    assert dqk0.dtype == torch.bfloat16 and dv0.dtype == torch.bfloat16
    o1, dqk1, dv1 = _bound(qk32, v32, do32, H)
    assert o1.dtype == torch.bfloat16 and dqk1.dtype == torch.float32 and dv1.dtype == torch.float32
    assert torch.equal(o1, o0) and torch.equal(dqk1, dqk0.float()) and torch.equal(dv1, dv0.float())
    nc = lambda t: t.transpose(0, 1).contiguous().transpose(0, 1)  # noqa: E731  (same values, other strides)
    o2, dqk2, dv2 = _bound(nc(qk16), nc(v16), nc(do16), H)
    assert not nc(qk16).is_contiguous()
    assert torch.equal(o2, o0) and torch.equal(dqk2, dqk0) and torch.equal(dv2, dv0)
