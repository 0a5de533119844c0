"""The HIP router with a per-context selection bias (moe_router_topk_fwd_selctx;
an -albc spec, src/moe/balance.py) against the CPU statement of the rule,
eager.route(..., sel_bias [C, E]), and the layer built on it against
moe_ffn_eager.

Shapes, inputs and bounds are those of tests/test_gpu_router_balance.py: x =
n/8 in bf16, wg = n/16, ctx_bias = n/64 and sel_bias[c, e] = n/128 with small
integers n, so every product and partial sum is representable, the logits and
keys are the same in any summation order and the index comparisons need no
exclusions.  fp32 outputs: 2e-6 absolute (lse: times max(1, |lse|)) -- nothing
in that path changed."""
from __future__ import annotations

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# T, d, E, k, tpi, n_ctx: a partial last block, E not a power of two, both wave layouts (E <= 32 / 64), three row
# chunks (d 384), the largest Wg (E d 4 = 64 KiB)
SHAPES = [(1, 128, 1, 1, 1, 1), (17, 128, 3, 2, 17, 2), (40, 256, 8, 2, 10, 6), (33, 384, 5, 3, 11, 6),
          (48, 256, 16, 2, 16, 6), (36, 256, 32, 4, 12, 6), (20, 256, 64, 8, 10, 6), (35, 1024, 16, 2, 7, 6)]
NAMES = ("idx", "w", "probs", "lse", "local_rank", "block_counts", "aux_partials")


def _ints(g, lo, hi, shape, div):
    return torch.randint(lo, hi + 1, shape, generator=g).float() / div


@functools.lru_cache(maxsize=None)
def _case(T, d, E, k, tpi, n_ctx, seed=0):
    """Exact router inputs on the CPU (fp32; x also representable in bf16).  The
    first draws are test_gpu_router_balance.py's; the [n_ctx, E] table follows."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * T + E)
    c = dict(x=_ints(g, -8, 8, (T, d), 8), wg=_ints(g, -4, 4, (E, d), 16), cb=_ints(g, -64, 64, (n_ctx, E), 64),
             sb=_ints(g, -256, 256, (E,), 128), ci=torch.randint(0, n_ctx, (T // tpi,), generator=g).int())
    c["sbc"] = _ints(g, -256, 256, (n_ctx, E), 128)
    return c


@functools.lru_cache(maxsize=None)
def _reference(T, d, E, k, tpi, n_ctx, normalize=True, biased=True, seed=0):
    from src.moe.eager import route

    c = _case(T, d, E, k, tpi, n_ctx, seed)
    return route(c["x"], c["wg"], c["cb"], c["ci"], tpi, k, normalize, c["sbc"] if biased else None)


def _gpu(c):
    return (c["x"].to(torch.bfloat16).to(DEV), c["wg"].to(DEV), c["cb"].to(DEV), c["ci"].to(DEV))


def _close(got, want, what, scale=1.0):
    err = float((got.detach().float().cpu() - want).abs().max())
    print(f"{what}: max abs error {err:.3e} (bound {2e-6 * scale:.3e})")
    assert err <= 2e-6 * scale, what


@pytest.mark.parametrize("T,d,E,k,tpi,n_ctx", SHAPES)
def test_kernel_against_reference(hip_lib, T, d, E, k, tpi, n_ctx):
    from src.moe import _lib as L

    c = _case(T, d, E, k, tpi, n_ctx)
    probs_r, lse_r, idx_r, w_r = _reference(T, d, E, k, tpi, n_ctx)
    idx_plain = _reference(T, d, E, k, tpi, n_ctx, biased=False)[2]
    x, wg, cb, ci = _gpu(c)
    sb = c["sbc"].to(DEV)
    idx, w, probs, lse, lrank, bcnt, auxp = L.router_topk_fwd(x, wg, cb, ci, tpi, k, True, sel_bias=sb)
    pos, tok, hist, offsets, _, _, _ = L.route_dispatch(bcnt, idx, lrank, w, auxp, T, E, 0, T * k)
    torch.cuda.synchronize()
    changed = int((idx_r != idx_plain).any(1).sum())
    print(f"tokens whose selection the bias changes: {changed} of {T}")
    assert changed >= 1 or E == 1  # the bias matters in this draw
    assert torch.equal(idx.cpu().long(), idx_r)
    assert torch.equal(hist.cpu().long(), torch.bincount(idx_r.reshape(-1), minlength=E))
    _close(probs, probs_r, "probs")
    _close(lse, lse_r, "lse", max(1.0, float(lse_r.abs().max())))
    _close(w, w_r, "w")
    # normalize=False: the gate is, bit for bit, the unbiased probability the same call wrote
    idx2, w2, probs2, *_ = L.router_topk_fwd(x, wg, cb, ci, tpi, k, False, sel_bias=sb)
    torch.cuda.synchronize()
    assert torch.equal(idx2, idx)
    assert torch.equal(w2, probs2.gather(1, idx2.long()))


@pytest.mark.parametrize("T,d,E,k,tpi,n_ctx", SHAPES)
def test_equal_rows_are_the_per_expert_entry(hip_lib, T, d, E, k, tpi, n_ctx):
    """A table whose rows are all one row: every output bit-identical to
    moe_router_topk_fwd_sel with that row."""
    from src.moe import _lib as L

    c = _case(T, d, E, k, tpi, n_ctx)
    x, wg, cb, ci = _gpu(c)
    row = c["sb"].to(DEV)
    one = L.router_topk_fwd(x, wg, cb, ci, tpi, k, True, sel_bias=row)
    tab = L.router_topk_fwd(x, wg, cb, ci, tpi, k, True, sel_bias=row.expand(n_ctx, E).contiguous())
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, one, tab):
        assert torch.equal(a, b), name


def _run_idx(c, tpi, k, sb):
    from src.moe import _lib as L
    from src.moe.eager import route

    x, wg, cb, ci = _gpu(c)
    idx = L.router_topk_fwd(x, wg, cb, ci, tpi, k, True, sel_bias=None if sb is None else sb.to(DEV))[0]
    torch.cuda.synchronize()
    ref = route(c["x"], c["wg"], c["cb"], c["ci"], tpi, k, True, sb)[2]
    return idx.cpu().long(), ref


def test_tie_made_by_one_contexts_bias(hip_lib):
    """Equal router rows a < b whose context biases differ by 0.5; row c0 of the
    selection bias differs by -0.5 (different logits, equal keys: the lower id
    goes first in c0's images), every other row is zero (their images select as
    without a bias: b, the larger logit, first)."""
    shape = (40, 256, 8, 2, 10, 6)
    T, d, E, k, tpi, n_ctx = shape
    c = {n: v.clone() for n, v in _case(*shape, seed=2).items()}
    a, b = 2, 5
    c["wg"][b] = c["wg"][a]
    c["cb"][:, b] = c["cb"][:, a] + 0.5
    c["ci"] = torch.tensor([1, 4, 1, 0], dtype=torch.int32)
    c0 = 1
    sb = torch.zeros(n_ctx, E)
    sb[c0, b] = -0.5
    idx, ref = _run_idx(c, tpi, k, sb)
    plain = _run_idx(c, tpi, k, None)[0]
    assert torch.equal(idx, ref)
    in_c0 = (c["ci"] == c0).repeat_interleave(tpi)
    assert int(in_c0.sum()) == 2 * tpi
    has_a, has_b = (ref == a).any(1), (ref == b).any(1)
    assert not (has_b & ~has_a)[in_c0].any() and int((has_a & ~has_b)[in_c0].sum()) > 0  # the tie -> the lower id
    both = has_a & has_b & in_c0
    assert bool(((ref == a).float().argmax(1) < (ref == b).float().argmax(1))[both].all())
    assert torch.equal(idx[~in_c0], plain[~in_c0])  # the other images: the unbiased selection
    assert not ((plain == a).any(1) & ~(plain == b).any(1)).any()  # ... where b's larger logit goes first
    assert not torch.equal(idx[in_c0], plain[in_c0])


@pytest.mark.parametrize("T,d,E,k,tpi,n_ctx", [SHAPES[4], SHAPES[5], SHAPES[6]])
def test_rounding_order(hip_lib, T, d, E, k, tpi, n_ctx):
    """One row of the table near 2^17: the add rounds to 1/64 there, so the
    order of the keys is the reference's only if the kernel forms
    fl(fl(dot + ctx) + sel) with that row."""
    c = _case(T, d, E, k, tpi, n_ctx)
    big = int(c["ci"][1])  # the second image's context: in these draws the rounding changes 1 or 2 of its tokens
    sb = c["sbc"].clone()
    sb[big] += 131072.0
    idx, ref = _run_idx(c, tpi, k, sb)
    small = _reference(T, d, E, k, tpi, n_ctx)[2]
    in_big = (c["ci"] == big).repeat_interleave(tpi)
    changed = int((ref != small).any(1).sum())
    print(f"tokens whose selection the rounding changes: {changed} of {int(in_big.sum())} in context {big}")
    assert changed > 0 and torch.equal(ref[~in_big], small[~in_big])
    assert torch.equal(idx, ref)


def test_table_beyond_the_lds_cap_is_refused(hip_lib):
    """n_ctx 64, E 64, d 256: Wg 64 KiB + two 16 KiB tables + 1.5 KiB > 96 KiB.
    The entry returns an error and launches nothing: the outputs keep their
    fill.  One context fewer rows fits and runs."""
    from src.moe import _lib as L

    T, d, E, k, tpi, n_ctx = 20, 256, 64, 8, 10, 64
    g = torch.Generator().manual_seed(0)
    x = _ints(g, -8, 8, (T, d), 8).to(torch.bfloat16).to(DEV)
    wg, cb = _ints(g, -4, 4, (E, d), 16).to(DEV), _ints(g, -64, 64, (n_ctx, E), 64).to(DEV)
    sb = _ints(g, -256, 256, (n_ctx, E), 128).to(DEV)
    ci = torch.tensor([63, 5], dtype=torch.int32, device=DEV)
    with pytest.raises(L.MoEKernelError, match="LDS"):
        L.router_topk_fwd(x, wg, cb, ci, tpi, k, True, sel_bias=sb)
    nblk = L.router_num_blocks(T)
    idx = torch.full((T, k), -7, dtype=torch.int32, device=DEV)
    lrank, bcnt = torch.full_like(idx, -7), torch.full((nblk, k, E), -7, dtype=torch.int32, device=DEV)
    w, probs = torch.full((T, k), -7.0, device=DEV), torch.full((T, E), -7.0, device=DEV)
    lse, auxp = torch.full((T,), -7.0, device=DEV), torch.full((nblk, E + 1), -7.0, device=DEV)
    rc = hip_lib.moe_router_topk_fwd_selctx(x.data_ptr(), wg.data_ptr(), cb.data_ptr(), ci.data_ptr(), n_ctx, tpi, T, d,
                                            E, k, 1, sb.data_ptr(), idx.data_ptr(), w.data_ptr(), probs.data_ptr(),
                                            lse.data_ptr(), lrank.data_ptr(), bcnt.data_ptr(), auxp.data_ptr(),
                                            L._stream())
    torch.cuda.synchronize()
    assert rc != 0
    for t in (idx, lrank, bcnt, w, probs, lse, auxp):
        assert bool((t == -7).all())
    # 40 contexts: 64 KiB + 2 x 10 KiB + 1.5 KiB fits, and equals the reference
    from src.moe.eager import route

    n2 = 40
    ci2 = torch.tensor([39, 5], dtype=torch.int32)
    got = L.router_topk_fwd(x, wg, cb[:n2].contiguous(), ci2.to(DEV), tpi, k, True, sel_bias=sb[:n2].contiguous())[0]
    torch.cuda.synchronize()
    ref = route(x.float().cpu(), wg.cpu(), cb[:n2].cpu(), ci2, tpi, k, True, sb[:n2].cpu())[2]
    assert torch.equal(got.cpu().long(), ref)


def test_dispatch_on_the_bias_rank(hip_lib, monkeypatch):
    """None and a 1-D bias still call the two old entries; a 2-D one the new."""
    from src.moe import _lib as L

    calls = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name.startswith("moe_router_topk_fwd"):
                calls.append(name)
            return getattr(self._lib, name)

    monkeypatch.setattr(L, "_LIB", Spy(hip_lib))
    x, wg, cb, ci = _gpu(_case(*SHAPES[2]))
    L.router_topk_fwd(x, wg, cb, ci, 10, 2, True)
    L.router_topk_fwd(x, wg, cb, ci, 10, 2, True, sel_bias=torch.zeros(8, device=DEV))
    L.router_topk_fwd(x, wg, cb, ci, 10, 2, True, sel_bias=torch.zeros((6, 8), device=DEV))
    torch.cuda.synchronize()
    assert calls == ["moe_router_topk_fwd", "moe_router_topk_fwd_sel", "moe_router_topk_fwd_selctx"]


def test_wrong_arguments(hip_lib):
    from src.moe import _lib as L

    x, wg, cb, ci = _gpu(_case(*SHAPES[2]))
    for bad in (torch.zeros((6, 8), dtype=torch.float64, device=DEV), torch.zeros((6, 8)),
                torch.zeros((5, 8), device=DEV), torch.zeros((6, 9), device=DEV), torch.zeros((1, 6, 8), device=DEV)):
        with pytest.raises(L.MoEKernelError):
            L.router_topk_fwd(x, wg, cb, ci, 10, 2, True, sel_bias=bad)
    with pytest.raises(L.MoEKernelError):  # no context: nothing to index by
        L.router_topk_fwd(x, wg, None, None, 10, 2, True, sel_bias=torch.zeros((6, 8), device=DEV))


# ---------------------------------------------------------------------------
# the layer
# ---------------------------------------------------------------------------
def _rel(a, ref):
    a, ref = a.detach().float().cpu(), ref.detach().float().cpu()
    return float((a - ref).norm() / ref.norm().clamp(min=1e-30))


LAYERS = [(40, 256, 8, 256, 2, 10, 0.0, "bf16"), (36, 256, 32, 256, 4, 12, 1.25, "fp8")]
GRADS = ("x", "wg", "cb", "w1", "b1", "w2", "b2")


@pytest.mark.parametrize("T,d,E,F,k,tpi,cf,expert_dtype", LAYERS)
def test_layer_forward_backward(hip_lib, T, d, E, F, k, tpi, cf, expert_dtype):
    """MoEFFN with a [C, E] table that changes selections against
    moe_ffn_eager with the same table: hist, last_topk_idx and last_ctx exact;
    y and every gradient at most twice as far from the eager layer as the same
    layer with no bias is from the unbiased eager layer, measured here on the
    same inputs (the bound of test_gpu_router_balance.py: both pairs run the
    same kernels, the bias only picks other rows)."""
    from src.moe.config import MoEConfig
    from src.moe.eager import moe_ffn_eager
    from src.moe.layer import MoEFFN

    c = _case(T, d, E, k, tpi, 6)
    B = T // tpi
    g = torch.Generator().manual_seed(7)
    dy = torch.randn(T, d, generator=g).to(torch.bfloat16).float()

    def layer(rate):
        torch.manual_seed(0)
        m = MoEFFN(d, MoEConfig(num_experts=E, top_k=k, hidden=F, capacity_factor=cf, expert_dtype=expert_dtype,
                                balance_rate=rate, balance_per_context=True))
        with torch.no_grad():
            m.wg.copy_(c["wg"])
            m.ctx_bias.copy_(c["cb"])
            for p in (m.w1, m.b1, m.w2, m.b2):
                p.copy_(p.to(torch.bfloat16).float())
            if rate > 0:
                m.sel_bias.copy_(c["sbc"])
        return m

    errs, hists = {}, {}
    for tag, rate in (("biased", 0.25), ("unbiased", 0.0)):
        m = layer(rate)
        cap = m.cfg.capacity(T)
        names = dict(x=None, wg=m.wg, cb=m.ctx_bias, w1=m.w1, b1=m.b1, w2=m.w2, b2=m.b2)
        # eager reference on the CPU, from the layer's own parameters
        pr = {n: v.detach().clone().requires_grad_(True) for n, v in names.items() if v is not None}
        pr["x"] = c["x"].clone().requires_grad_(True)
        sink = []
        yr, lb, z, hr = moe_ffn_eager(pr["x"], pr["wg"], pr["cb"], pr["w1"], pr["b1"], pr["w2"], pr["b2"], c["ci"], tpi,
                                      k, True, cap, expert_dtype, sel_bias=m.sel_bias, idx_sink=sink)
        ((yr.float() * dy).sum() + m.cfg.lb_coef * lb + m.cfg.z_coef * z).backward()
        # the layer on the GPU
        m = m.to(DEV)
        xg = c["x"].to(torch.bfloat16).to(DEV).requires_grad_(True)
        y = m(xg.view(B, tpi, d), c["ci"].to(DEV)).view(T, d)
        ((y.float() * dy.to(DEV)).sum() + m.aux_loss()).backward()
        torch.cuda.synchronize()
        assert torch.equal(m.last_hist.cpu(), hr), tag
        if rate > 0:
            assert m.last_topk_idx.dtype == torch.int32 and torch.equal(m.last_topk_idx.cpu().long(), sink[0]), tag
            assert torch.equal(m.last_ctx.cpu(), c["ci"]), tag
        else:
            assert m.sel_bias is None and m.last_topk_idx is None and m.last_ctx is None
        got = dict(y=y, dx=xg.grad, dwg=m.wg.grad, dcb=m.ctx_bias.grad, dw1=m.w1.grad, db1=m.b1.grad, dw2=m.w2.grad,
                   db2=m.b2.grad)
        ref = dict(y=yr, **{"d" + n: pr[n].grad for n in GRADS})
        errs[tag] = {n: _rel(got[n], ref[n]) for n in got}
        hists[tag] = hr
    assert not torch.equal(hists["biased"], hists["unbiased"])  # the table moves assignments
    for n in errs["biased"]:
        print(f"{expert_dtype} E{E} {n}: relative Frobenius error biased {errs['biased'][n]:.3e}, "
              f"unbiased {errs['unbiased'][n]:.3e}")
    for n in errs["biased"]:
        assert errs["biased"][n] <= 2.0 * errs["unbiased"][n], n


def test_ep_layer_routes_like_the_plain_layer(hip_lib, monkeypatch):
    """An -ep1 layer (no process group) with a per-context table selects the
    same experts as the non-EP layer with the same weights, and keeps the same
    indices for the balancer."""
    from src.moe import _lib as L
    from src.moe.config import MoEConfig
    from src.moe.layer import MoEFFN

    seen = []
    real = L.router_topk_fwd

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((out[0].clone(), kw.get("sel_bias", a[7] if len(a) > 7 else None)))
        return out

    monkeypatch.setattr(L, "router_topk_fwd", spy)
    T, d, E, k, tpi, n_ctx = SHAPES[2]
    c = _case(T, d, E, k, tpi, n_ctx)
    layers = []
    for ep in (False, True):
        torch.manual_seed(0)
        m = MoEFFN(d, MoEConfig(num_experts=E, top_k=k, hidden=256, balance_rate=0.25, balance_per_context=True,
                                expert_parallel=ep)).to(DEV)
        with torch.no_grad():
            m.wg.copy_(c["wg"])
            m.ctx_bias.copy_(c["cb"])
            m.sel_bias.copy_(c["sbc"])
        m(c["x"].to(torch.bfloat16).to(DEV).view(T // tpi, tpi, d), c["ci"].to(DEV))
        layers.append(m)
    torch.cuda.synchronize()
    assert len(seen) == 2 and all(sb is not None and sb.dim() == 2 for _, sb in seen)
    assert torch.equal(seen[0][0], seen[1][0])
    assert torch.equal(seen[0][0].cpu().long(), _reference(T, d, E, k, tpi, n_ctx)[2])
    assert torch.equal(layers[0].last_hist, layers[1].last_hist)
    for m in layers:
        assert torch.equal(m.last_topk_idx, seen[0][0]) and torch.equal(m.last_ctx.cpu(), c["ci"])
