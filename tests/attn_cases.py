"""Reference and case table of the HIP attention's edge tests
(tests/test_attn_cases_cpu.py, tests/test_gpu_attn_edges.py).  No GPU import:
everything here runs on the CPU.

``ref64`` is softmax(scale q k^T) v and its gradients in float64 on the bf16
operands, with lse2 (row max + log2 of the row sum of the base-2 softmax, as
include/moe_hip.h defines lse) and delta = rowsum(dout * o) of the exact o.
``emul64`` is the same operation with the roundings csrc/attn.hip documents
(fp32 scores, P and dS rounded to bf16 before the second products, delta from
the bf16 o, bf16 outputs) in one pass over whole rows: no tiles, no running
max, no lane order.  Its error against ``ref64`` is what those roundings cost
on a case; the kernels are allowed ``MARGIN`` times that plus an absolute
floor (``limits``).

Operands are logical tensors [B, L, 32 H] (heads concatenated, the layout of
the projection outputs); strides and guard bytes are the GPU test's business,
``Case.lds`` only names the row stride of every buffer."""
from __future__ import annotations

import functools
import json
import math
import os
from dataclasses import dataclass

import numpy as np
import torch

DH = 32
LOG2E = 1.4426950408889634
MARGIN = 4.0        # kernel error allowed, in units of emul64's error of the same case, slice and measure
F32_FLOOR_ULPS = 4  # lse, delta: absolute floor in fp32 ulp of the slice's max |ref|
# error factor of a 32-term fp32 dot product in any order under faithful rounding
# (unit 2^-23: the MFMA's internal rounding is not documented as round-to-nearest)
GAMMA32 = 32 * 2.0 ** -23
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
OUTPUTS = ("o", "dq", "dk", "dv", "lse", "delta")
BF16_OUTPUTS = OUTPUTS[:4]
BUFFERS = ("q", "k", "v", "o", "do", "dq", "dk", "dv")


def f32(x) -> float:
    """x rounded to fp32: the C ABI takes ``scale`` as a float."""
    return float(np.float32(x))


def bf16r(t):
    """float64 -> the nearest bf16 (ties to even), as float64.  Exact in two
    steps for the values met here: they are far from fp32's range limits and
    a double rounding through fp32 needs a tie at bit 29 of the fraction."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def f32r(t):
    return t.to(torch.float32).to(torch.float64)


def heads(t):
    """[B, L, 32 H] -> [B, H, L, 32]"""
    B, L, HD = t.shape
    return t.reshape(B, L, HD // DH, DH).transpose(1, 2)


def unheads(t):
    """[B, H, L, 32] -> [B, L, 32 H]"""
    B, H, L, _ = t.shape
    return t.transpose(1, 2).reshape(B, L, H * DH)


def visible(seg, L):
    """bool [L query, L key]: seg[k] < 0 or seg[k] == seg[q]; all True without seg."""
    if seg is None:
        return torch.ones(L, L, dtype=torch.bool)
    seg = torch.as_tensor(seg).long()
    return (seg[None, :] < 0) | (seg[None, :] == seg[:, None])


def _backward(p_left, ds_left, qh, kh, doh, scale):
    return (unheads(scale * (ds_left @ kh)), unheads(scale * (ds_left.transpose(-1, -2) @ qh)),
            unheads(p_left.transpose(-1, -2) @ doh))


def ref64(q, k, v, dout, scale, seg=None):
    """(o, dq, dk, dv [B, L, 32 H], lse2, delta [B, H, L]) in float64, exact on the bf16 operands."""
    qh, kh, vh, doh = (heads(t.detach().cpu().double()) for t in (q, k, v, dout))
    L = qh.shape[2]
    s2 = (qh @ kh.transpose(-1, -2)) * (scale * LOG2E)
    s2 = s2.masked_fill(~visible(seg, L), float("-inf"))
    m = s2.amax(-1, keepdim=True)
    lse2 = m + torch.log2(torch.exp2(s2 - m).sum(-1, keepdim=True))
    p = torch.exp2(s2 - lse2)
    o = p @ vh
    delta = (doh * o).sum(-1, keepdim=True)
    ds = p * (doh @ vh.transpose(-1, -2) - delta)
    dq, dk, dv = _backward(p, ds, qh, kh, doh, scale)
    return unheads(o), dq, dk, dv, lse2.squeeze(-1), delta.squeeze(-1)


def emul64(q, k, v, dout, scale, seg=None):
    """ref64's outputs under attn.hip's stated roundings.  Scores and dP are
    fp32 accumulators (here: torch's fp32 matmul on the CPU, one more summation
    order) scaled by the fp32 product scale * log2(e); P~ = exp2(s - m) is
    rounded to bf16 before P~ V; o = (P~ V) / sum(P~) with the unrounded sum,
    then bf16; lse is fp32.  Backward: P = exp2(s - lse) and dS = P (dP - delta)
    are rounded to bf16 before the second products, delta (fp32) comes from the
    bf16 o, and dq, dk, dv are rounded to bf16."""
    q, k, v, dout = (t.detach().cpu() for t in (q, k, v, dout))
    qf, kf, vf, dof = (heads(t.float()) for t in (q, k, v, dout))
    qh, kh, vh, doh = (t.double() for t in (qf, kf, vf, dof))
    L = qh.shape[2]
    sl2 = torch.tensor(np.float32(scale) * np.float32(LOG2E), dtype=torch.float32)
    s2 = ((qf @ kf.transpose(-1, -2)) * sl2).double()
    s2 = s2.masked_fill(~visible(seg, L), float("-inf"))
    m = s2.amax(-1, keepdim=True)
    pt = torch.exp2(s2 - m)
    lsum = pt.sum(-1, keepdim=True)
    o = bf16r((bf16r(pt) @ vh) / lsum)
    lse = f32r(m + torch.log2(lsum))
    p = torch.exp2(s2 - lse)
    dp = (dof @ vf.transpose(-1, -2)).double()
    delta = f32r((doh * o).sum(-1, keepdim=True))
    ds = bf16r(p * (dp - delta))
    dq, dk, dv = _backward(bf16r(p), ds, qh, kh, doh, scale)
    return unheads(o), bf16r(dq), bf16r(dk), bf16r(dv), lse.squeeze(-1), delta.squeeze(-1)


def zero_bounds(q, k, v, dout, scale, seg=None):
    """(|dq|, |dk|) bounds [B, L, 32 H] on what fp32 rounding alone puts into dq
    and dk: dP (a 32-term fp32 dot product) and delta (another) each carry an
    error of at most GAMMA32 sum |terms|, so dS = P (dP - delta) is off by at most
        e[i, j] = P[i, j] GAMMA32 (|dout_i| . |v_j| + |dout_i| . |o_i|),
    which bf16 rounding of dS grows by 1 + 2^-8 at the most, and
        |dq_i| <= |scale| (1 + 2^-8) sum_j e[i, j] |k_j|,
        |dk_j| <= |scale| (1 + 2^-8) sum_i e[i, j] |q_i|.
    Where dS vanishes in exact math (one visible key: one-hot rows, L = 1,
    all-distinct segments) this bounds the outputs themselves; elsewhere it
    joins the absolute floor."""
    qh, kh, vh, doh = (heads(t.detach().cpu().double()) for t in (q, k, v, dout))
    o, _, _, _, lse2, _ = ref64(q, k, v, dout, scale, seg)
    L = qh.shape[2]
    s2 = (qh @ kh.transpose(-1, -2)) * (scale * LOG2E)
    p = torch.exp2(s2.masked_fill(~visible(seg, L), float("-inf")) - lse2.unsqueeze(-1))
    e = p * GAMMA32 * (doh.abs() @ vh.abs().transpose(-1, -2)
                       + (doh.abs() * heads(o).abs()).sum(-1, keepdim=True))
    c = abs(scale) * (1 + 2.0 ** -8)
    return unheads(c * (e @ kh.abs())), unheads(c * (e.transpose(-1, -2) @ qh.abs()))


# ---------------------------------------------------------------------------
# error measures and limits
# ---------------------------------------------------------------------------
def half_ulp_bf16(x: float) -> float:
    return 0.0 if x <= 0 else 2.0 ** (math.floor(math.log2(x)) - 8)


def ulp_f32(x: float) -> float:
    return 0.0 if x <= 0 else 2.0 ** (math.floor(math.log2(x)) - 23)


def slices(name, t, B, H):
    """("all", t) and every (image, head) slice of an output."""
    yield "all", t
    for b in range(B):
        for h in range(H):
            yield f"b{b}h{h}", (t[b, h] if name in ("lse", "delta") else t[b, :, DH * h:DH * (h + 1)])


def _abs_err(got, ref):
    d = (torch.as_tensor(got).detach().cpu().double() - ref).abs()
    if not bool(torch.isfinite(d).all()):
        return float("inf"), float("inf")
    return float(d.norm()), float(d.max())


def figures(got, ref, B, H):
    """{output: {slice: (Frobenius |got - ref|, max |got - ref|)}}"""
    return {n: {s: _abs_err(g, r) for (s, g), (_, r) in zip(slices(n, got[i], B, H), slices(n, ref[i], B, H))}
            for i, n in enumerate(OUTPUTS)}


def limits(emul_fig, ref, zb, B, H):
    """The same structure: MARGIN x emul64's figure + the absolute floor.  Floor
    per element: half a bf16 ulp of the slice's max |ref| for o, dq, dk, dv
    (plus zero_bounds for dq, dk), F32_FLOOR_ULPS fp32 ulp of it for lse and
    delta; the Frobenius limit takes the floor on every element."""
    out = {}
    for i, n in enumerate(OUTPUTS):
        out[n] = {}
        zs = dict(slices(n, zb[n], B, H)) if n in zb else {}
        for s, r in slices(n, ref[i], B, H):
            top = float(r.abs().max())
            fl = half_ulp_bf16(top) if n in BF16_OUTPUTS else F32_FLOOR_ULPS * ulp_f32(top)
            zf, zm = (float(zs[s].norm()), float(zs[s].max())) if zs else (0.0, 0.0)
            ef, em = emul_fig[n][s]
            out[n][s] = (MARGIN * ef + fl * r.numel() ** 0.5 + zf, MARGIN * em + fl + zm)
    return out


def worst_ratio(fig, lim):
    """{output: (largest figure / limit over slices and measures, where)}; a
    zero limit met by a zero figure counts as 0."""
    out = {}
    for n in fig:
        worst, where = 0.0, ""
        for s in fig[n]:
            for j, meas in enumerate(("fro", "max")):
                a, b = fig[n][s][j], lim[n][s][j]
                r = 0.0 if a == 0.0 else (a / b if b > 0 else float("inf"))
                if r >= worst:
                    worst, where = r, f"{s}/{meas}"
        out[n] = (worst, where)
    return out


def relative(fig, ref):
    """Whole-tensor figures in relative terms: (relative Frobenius error,
    max error / max |ref|); None where the reference vanishes."""
    out = {}
    for i, n in enumerate(OUTPUTS):
        nr, top = float(ref[i].norm()), float(ref[i].abs().max())
        ef, em = fig[n]["all"]
        out[n] = (ef / nr if nr > 0 else None, em / top if top > 0 else None)
    return out


def report(record):
    """With ATTN_REPORT=<file>: append one JSON line per call."""
    path = os.environ.get("ATTN_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    kind: str                 # layout | scale | peaked | ramp | segments | onehot | uniform
    q: torch.Tensor           # bf16 [B, L, 32 H]
    k: torch.Tensor
    v: torch.Tensor
    dout: torch.Tensor
    scale: float              # already an fp32 value
    lds: dict                 # row stride in elements of each of BUFFERS
    seg: tuple | None = None  # L segment ids
    pi: tuple | None = None   # one-hot: query i's key

    @property
    def shape(self):
        B, L, HD = self.q.shape
        return B, HD // DH, L

    def operands(self):
        return self.q, self.k, self.v, self.dout, self.scale, self.seg


SCALE0 = f32(1.0 / math.sqrt(DH))


def padded_lds(H):
    """A stride of its own for every buffer: 32 H + 8 ... 32 H + 56, k's 64 H + 72."""
    d = DH * H
    return dict(q=d + 8, k=2 * d + 72, v=d + 24, o=d + 40, do=d + 16, dq=d + 56, dk=d + 32, dv=d + 48)


def packed_lds(H):
    """self_attention_hip's layout: q | k rows of one [B L, 2 d] buffer, everything else [B L, d]."""
    d = DH * H
    return dict(q=2 * d, k=2 * d, v=d, o=d, do=d, dq=2 * d, dk=2 * d, dv=d)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 3) * 7919 ** i * int(x) for i, x in enumerate(key)) % (2 ** 31))


def _randn(g, B, L, H, std=1.0):
    return (torch.randn(B, L, DH * H, generator=g) * std).to(torch.bfloat16)


def _random_case(name, kind, B, H, L, scale=SCALE0, std=1.5, seg=None, seed=0):
    g = _gen(B, H, L, seed)
    return Case(name, kind, _randn(g, B, L, H, std), _randn(g, B, L, H, std), _randn(g, B, L, H),
                _randn(g, B, L, H), f32(scale), padded_lds(H), None if seg is None else tuple(seg))


LAYOUT_ROWS = [(1, 1, 1), (3, 3, 15), (1, 8, 16), (3, 1, 17), (1, 3, 63), (3, 8, 64), (1, 1, 65), (3, 3, 127),
               (1, 8, 128), (3, 1, 129), (1, 3, 193)]  # (B, H, L)
SCALE_ROWS = [("rsqrt32", SCALE0, 1, 2, 129), ("one", 1.0, 3, 2, 65), ("2^-5", 2.0 ** -5, 1, 3, 17),
              ("-0.5", -0.5, 3, 1, 127), ("zero", 0.0, 1, 2, 64)]  # (tag, scale, B, H, L)
PEAKED_ROWS = [(4.0, 3, 2, 65, 0.85), (8.0, 1, 2, 129, 0.95), (8.0, 1, 1, 193, 0.95)]  # (std, B, H, L, top p >)
RAMP_L = 193


def _ramp_case(name, variant):
    """k_j = (12 j / L) u + 0.3 randn, q = 6 u + 0.3 randn (u a unit vector per
    head): the scores rise by 72 scale = 12.7 over the keys, 4.2 per 64-key tile
    against a noise of 0.3, so the running max moves at every tile.  "down":
    the keys in reverse order (the max sits in tile 0 and every later tile is
    rescaled against it); "last": key L - 1, alone in the last partial tile,
    at twice the ramp's top."""
    B, H, L = 1, 2, RAMP_L
    g = _gen(B, H, L, {"up": 11, "down": 12, "last": 13}[variant])
    u = torch.randn(H, DH, generator=g)
    u = (u / u.norm(dim=-1, keepdim=True)).reshape(1, 1, H * DH)
    ramp = 12.0 * torch.arange(L).double() / L
    if variant == "down":
        ramp = ramp.flip(0)
    if variant == "last":
        ramp[L - 1] = 24.0
    k = (ramp.float()[None, :, None] * u + 0.3 * torch.randn(B, L, H * DH, generator=g)).to(torch.bfloat16)
    q = (6.0 * u + 0.3 * torch.randn(B, L, H * DH, generator=g)).to(torch.bfloat16)
    return Case(name, "ramp", q, k, _randn(g, B, L, H), _randn(g, B, L, H), SCALE0, padded_lds(H))


def onehot_codes(n, seed=5):
    """n distinct codes in {-1, +1}^32 with pairwise Hamming distance >= 6, by rejection."""
    g = torch.Generator().manual_seed(seed)
    codes = []
    while len(codes) < n:
        c = torch.randint(0, 2, (DH,), generator=g) * 2 - 1
        if all(int((c != d).sum()) >= 6 for d in codes):
            codes.append(c)
    return torch.stack(codes).float()


def onehot_perm(L):
    """Query i's key: i -> (37 i + 64) mod L when that is a permutation, which
    sends the first rows into the second tile and reaches the last partial one."""
    assert math.gcd(37, L) == 1
    return tuple((37 * i + 64) % L for i in range(L))


ONEHOT_ROWS = [(3, 1, 65), (1, 3, 130), (1, 2, 193)]  # (B, H, L)


def _onehot_case(B, H, L):
    g = _gen(B, H, L, 21)
    c = onehot_codes(L)
    pi = onehot_perm(L)
    k = (8.0 * c)[None, :, None, :].expand(B, L, H, DH).reshape(B, L, H * DH).to(torch.bfloat16)
    q = (8.0 * c[list(pi)])[None, :, None, :].expand(B, L, H, DH).reshape(B, L, H * DH).to(torch.bfloat16)
    return Case(f"onehot_L{L}", "onehot", q, k, _randn(g, B, L, H), _randn(g, B, L, H), SCALE0, padded_lds(H),
                pi=pi)


UNIFORM_ROWS = [(1, 3, 17), (3, 1, 65), (1, 2, 129), (1, 1, 193)]  # (B, H, L)


def _uniform_case(B, H, L):
    """q = 0: every score is 0 at any scale, P = 1 / L, o = sum(v) / L with
    integer v in [-8, 8] (the sum is exact in fp32), lse2 = log2 L, dk = 0."""
    g = _gen(B, H, L, 31)
    v = torch.randint(-8, 9, (B, L, H * DH), generator=g).to(torch.bfloat16)
    return Case(f"uniform_L{L}", "uniform", torch.zeros(B, L, H * DH, dtype=torch.bfloat16), _randn(g, B, L, H, 1.5),
                v, _randn(g, B, L, H), SCALE0, padded_lds(H))


def _seg_special():
    """L = 129 (two full tiles and one key): the user's ids -2, -3, INT32_MIN
    around the 63 | 64 tile edge and as the last key (next to the rows past L,
    which the kernels mark -2 and -3 themselves), INT32_MAX an ordinary group
    with a member on each side of the last edge."""
    ids = [i // 20 for i in range(129)]
    ids[62], ids[63], ids[64], ids[65] = -2, -3, INT32_MIN, INT32_MAX
    ids[126], ids[127], ids[128] = INT32_MAX, -3, -2
    ids[0], ids[1] = INT32_MIN, INT32_MAX
    return ids


def _seg_late():
    """L = 130.  Queries 64..79 are one wave.  Query 64 shares id 1 with key 0,
    so tile 0 is live for the wave; queries 65..79 have ids of their own and
    see nothing there (their running max stays -inf through a computed tile).
    Tile 1 holds their first key (themselves).  Key 129, in the last partial
    tile, is shared.  Rows 0..63 likewise: 1..63 see nothing of tile 1."""
    ids = [1000 + i for i in range(130)]
    ids[0] = ids[64] = 1
    ids[129] = -1
    return ids


SEG_ROWS = {"seg_distinct": (1, 130, list(range(130))), "seg_special": (3, 129, _seg_special()),
            "seg_late": (1, 130, _seg_late()), "seg_shared": (3, 65, [-1] * 65)}  # (B, L, ids); H = 3


@functools.lru_cache(maxsize=None)
def cases():
    """Every case by name, in table order."""
    out = [_random_case(f"layout_B{B}H{H}L{L}", "layout", B, H, L) for B, H, L in LAYOUT_ROWS]
    out += [_random_case(f"scale_{tag}", "scale", B, H, L, scale=s, seed=1) for tag, s, B, H, L in SCALE_ROWS]
    out += [_random_case(f"peaked_x{std:g}_L{L}", "peaked", B, H, L, std=std, seed=2)
            for std, B, H, L, _ in PEAKED_ROWS]
    out += [_ramp_case(f"ramp_{v}", v) for v in ("up", "down", "last")]
    out += [_random_case(n, "segments", B, 3, L, seg=ids, seed=3) for n, (B, L, ids) in SEG_ROWS.items()]
    out += [_onehot_case(*r) for r in ONEHOT_ROWS]
    out += [_uniform_case(*r) for r in UNIFORM_ROWS]
    out.append(_random_case("uniform_scale0", "uniform", 1, 2, 65, scale=0.0, seed=4))
    return {c.name: c for c in out}


STATISTICAL = ("layout", "scale", "peaked", "ramp", "segments")
CASE_NAMES = list(cases())
STATISTICAL_NAMES = [n for n, c in cases().items() if c.kind in STATISTICAL]


def names_of(kind):
    return [n for n, c in cases().items() if c.kind == kind]


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(ref64, emul64's figures, limits) of a table case, computed once."""
    c = cases()[name]
    B, H, _ = c.shape
    ref = ref64(*c.operands())
    fig = figures(emul64(*c.operands()), ref, B, H)
    zq, zk = zero_bounds(*c.operands())
    return ref, fig, limits(fig, ref, {"dq": zq, "dk": zk}, B, H)


def top_probability(c: Case):
    """Mean over rows of the largest softmax probability."""
    _, _, _, _, lse2, _ = ref64(*c.operands())
    s2 = (heads(c.q.double()) @ heads(c.k.double()).transpose(-1, -2)) * (c.scale * LOG2E)
    s2 = s2.masked_fill(~visible(c.seg, c.shape[2]), float("-inf"))
    return float(torch.exp2(s2 - lse2.unsqueeze(-1)).amax(-1).mean())


def tile_maxima(c: Case):
    """[B, H, L, tiles]: the largest score of every query in each 64-key tile."""
    s = (heads(c.q.double()) @ heads(c.k.double()).transpose(-1, -2)) * c.scale
    return torch.stack([t.amax(-1) for t in s.split(64, dim=-1)], -1)
