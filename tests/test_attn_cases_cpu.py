"""The reference and the case table of the HIP attention's edge tests
(tests/attn_cases.py), checked without a GPU: ref64 is float64
scaled_dot_product_attention (output, autograd gradients, logsumexp) under
linear.segment_mask, and every table has the property its GPU test relies on.
With ATTN_REPORT=<file> every case appends one JSON line with emul64's error
against ref64 -- the reference's side of the GPU tests' tolerance."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_cases as ac
from src.rtdetr_moe.linear import segment_mask

# float64 on both sides, sums of at most 193 terms of magnitude <= 1e3: 1e-11
# relative to the output's largest element leaves four digits of room
SAME_MATH_FP64 = 1e-11


def _close(got, want, what):
    top = float(want.abs().max())
    err = float((got - want).abs().max())
    assert err <= SAME_MATH_FP64 * max(top, 1.0), f"{what}: {err:.3e} vs max |ref| {top:.3e}"


@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_ref64_is_scaled_dot_product_attention(name):
    c = ac.cases()[name]
    B, H, L = c.shape
    q, k, v = (ac.heads(t.double()).clone().requires_grad_(True) for t in (c.q, c.k, c.v))
    mask = None
    if c.seg is not None:
        mask = segment_mask(torch.tensor(c.seg, dtype=torch.int32))
        assert torch.equal(mask, ac.visible(c.seg, L))
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=c.scale)
    dq, dk, dv = torch.autograd.grad(o, [q, k, v], ac.heads(c.dout.double()))
    ref = ac.ref64(*c.operands())
    for got, want, what in zip(ref[:4], (o.detach(), dq, dk, dv), ac.BF16_OUTPUTS):
        _close(got, ac.unheads(want), what)
    s = (q.detach() @ k.detach().transpose(-1, -2)) * c.scale
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    _close(ref[4], torch.logsumexp(s, -1) / math.log(2.0), "lse2")
    _close(ref[5], (ac.heads(c.dout.double()) * o.detach()).sum(-1), "delta")
    zq, zk = ac.zero_bounds(*c.operands())
    assert bool(torch.isfinite(zq).all() and torch.isfinite(zk).all() and (zq >= 0).all() and (zk >= 0).all())


def test_table_covers_the_tile_edges_layouts_and_scales():
    cs = ac.cases()
    lay = [cs[n] for n in ac.names_of("layout")]
    assert {c.shape[2] for c in lay} == {1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193}
    assert {c.shape[1] for c in lay} == {1, 3, 8} and {c.shape[0] for c in lay} == {1, 3}
    assert {c.scale for c in cs.values() if c.kind == "scale"} == {ac.SCALE0, 1.0, 2.0 ** -5, -0.5, 0.0}
    for c in cs.values():
        B, H, L = c.shape
        assert L in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 193) and B in (1, 3), c.name
        assert c.scale == ac.f32(c.scale)
        lds = c.lds
        assert set(lds) == set(ac.BUFFERS) and len(set(lds.values())) == len(lds), c.name  # all different
        assert all(ld % 8 == 0 and ld > ac.DH * H for ld in lds.values()), c.name
        for t in (c.q, c.k, c.v, c.dout):
            assert t.dtype == torch.bfloat16 and t.shape == (B, L, ac.DH * H)
    assert all(cs[n].shape[1] == 3 for n in ac.names_of("segments"))


@pytest.mark.parametrize("row", ac.PEAKED_ROWS, ids=lambda r: f"x{r[0]:g}_L{r[3]}")
def test_peaked_cases_are_peaked(row):
    std, B, H, L, floor = row
    top = ac.top_probability(ac.cases()[f"peaked_x{std:g}_L{L}"])
    print(row, "mean top probability", top)
    assert top >= floor
    assert ac.top_probability(ac.cases()["layout_B1H3L193"]) < 0.5  # what randn * 1.5 reaches


def test_ramp_cases_move_the_running_max():
    """ramp_up: every row's max rises in tiles 1 and 2, and in the one-key tile 3
    for some rows; ramp_last: in all of 1, 2, 3 for every row, and key L - 1
    takes nearly all the mass; ramp_down: tile 0 holds every row's max."""
    cs = ac.cases()
    up, down, last = (ac.tile_maxima(cs[f"ramp_{v}"]) for v in ("up", "down", "last"))
    assert up.shape[-1] == 4
    run = up.cummax(-1).values
    assert bool((up[..., 1:3] > run[..., 0:2]).all())
    assert bool((up[..., 3] > run[..., 2]).any())
    run = last.cummax(-1).values
    assert bool((last[..., 1:] > run[..., :-1]).all())
    assert ac.top_probability(cs["ramp_last"]) > 0.99
    assert bool((down[..., 0:1] > down[..., 1:]).all())
    for v in ("up", "down"):  # spread over the row: a rescale that is skipped shows in o
        assert ac.top_probability(cs[f"ramp_{v}"]) < 0.6


@pytest.mark.parametrize("name", ac.names_of("onehot"))
def test_onehot_cases_are_exactly_one_hot_in_fp32(name):
    c = ac.cases()[name]
    B, H, L = c.shape
    pi = torch.tensor(c.pi)
    assert sorted(c.pi) == list(range(L))
    tiles = {(i // 64, int(p) // 64) for i, p in enumerate(c.pi)}
    nt = (L + 63) // 64
    full = range(L // 64)
    assert {(a, b) for a in full for b in full if a != b} <= tiles  # every full tile to every other
    assert L % 64 != 0                                              # the last, partial one: in and out
    assert any(b == nt - 1 and a != b for a, b in tiles) and any(a == nt - 1 and a != b for a, b in tiles)
    codes = ac.onehot_codes(L)
    ham = (codes[:, None, :] != codes[None, :, :]).sum(-1)
    assert int((ham + 64 * torch.eye(L, dtype=torch.long)).min()) >= 6
    sl2 = torch.tensor(np.float32(c.scale) * np.float32(ac.LOG2E))
    s = ac.heads(c.q.float()) @ ac.heads(c.k.float()).transpose(-1, -2)  # exact integers
    assert torch.equal(s, s.round()) and float(s.max()) == 2048.0
    s2 = s * sl2
    top2 = s2.topk(2, -1).values
    assert bool((s2.argmax(-1) == pi).all())
    assert float((top2[..., 0] - top2[..., 1]).min()) >= 150.0
    p = torch.exp2(s2 - s2.amax(-1, keepdim=True))
    assert torch.equal(p, F.one_hot(pi, L).float().expand(B, H, L, L))
    print(name, "row max", float(s2.max()), "gap", float((top2[..., 0] - top2[..., 1]).min()))
    assert 522.2 < float(s2.max()) < 522.4
    ref = ac.ref64(*c.operands())
    assert torch.equal(ref[0], c.v.double()[:, list(c.pi)])
    assert float(ref[1].abs().max()) < 1e-40 and float(ref[2].abs().max()) < 1e-40


@pytest.mark.parametrize("name", ac.names_of("uniform"))
def test_uniform_cases_have_exact_sums(name):
    c = ac.cases()[name]
    B, H, L = c.shape
    ref = ac.ref64(*c.operands())
    assert L % 64 != 0
    _close(ref[4], torch.full((B, H, L), math.log2(L), dtype=torch.float64), "lse2")
    if c.scale == 0.0:
        assert float(ref[1].abs().max()) == 0.0 and float(ref[2].abs().max()) == 0.0
        return
    assert float(c.q.abs().max()) == 0.0 and float(ref[2].abs().max()) == 0.0
    v = c.v.float()
    assert torch.equal(v, v.round()) and float(v.abs().max()) <= 8
    total = v.sum(1)  # fp32, any order: integers below 2^24
    assert torch.equal(total.double(), c.v.double().sum(1)) and float(total.abs().max()) < 2 ** 24
    _close(ref[0], (c.v.double().sum(1, keepdim=True) / L).expand(B, L, -1), "o")


@pytest.mark.parametrize("name", ac.names_of("segments"))
def test_segment_cases(name):
    c = ac.cases()[name]
    B, H, L = c.shape
    vis = ac.visible(c.seg, L)
    assert len(c.seg) == L and bool(vis.diagonal().all())  # each query sees itself
    seen = vis.sum(-1)
    if name == "seg_distinct":
        assert bool((seen == 1).all())
    if name == "seg_shared":
        assert bool(vis.all())
    if name == "seg_special":
        ids = set(c.seg)
        assert {-2, -3, ac.INT32_MIN, ac.INT32_MAX} <= ids
        assert c.seg[L - 1] == -2 and L % 64 == 1 and c.seg[63] < -1 and c.seg[64] < -1
        for i in range(L):  # the user's negative ids are shared keys
            if c.seg[i] < 0:
                assert bool(vis[:, i].all())
        big = [i for i in range(L) if c.seg[i] == ac.INT32_MAX]
        assert len(big) >= 2 and not bool(vis[2, big[0]])
    if name == "seg_late":
        first = vis.float().argmax(-1)
        wave = range(64, 80)
        assert int(first[64]) == 0 and all(int(first[i]) == i for i in wave if i != 64)
        assert not bool(vis[65:80, :64].any()) and bool(vis[:, 129].all())


@pytest.mark.parametrize("name", ac.STATISTICAL_NAMES)
def test_emul64_figures(name):
    """emul64's error against ref64 is finite, and non-zero wherever rounding
    can act: not where a query sees one key only (o = v and dv = dout are
    exact then), not on lse, which can be an exact fp32 number (log2 64)."""
    c = ac.cases()[name]
    B, H, L = c.shape
    ref, fig, lim = ac.case_reference(name)
    single = bool((ac.visible(c.seg, L).sum(-1) == 1).all())
    for n, r in zip(ac.OUTPUTS, ref):
        assert bool(torch.isfinite(r).all())
        for s, (ef, em) in fig[n].items():
            assert math.isfinite(ef) and math.isfinite(em), (n, s)
            assert all(math.isfinite(x) and x >= 0 for x in lim[n][s])
        if n != "lse" and float(r.abs().max()) > 0 and not (single and n in ("o", "dv")):
            assert fig[n]["all"][0] > 0, n
    rel = ac.relative(fig, ref)
    ac.report({"case": name, "side": "emul64", **{n: rel[n] for n in ac.OUTPUTS}})
    print(name, rel)
