"""The HIP router with a selection bias (moe_router_topk_fwd_sel; loss-free
load balancing, src/moe/balance.py) against the CPU statement of the rule,
eager.route(..., sel_bias), and the layer built on it against moe_ffn_eager.

Router inputs are exact: x = n/8 in bf16, wg = n/16, ctx_bias = n/64,
sel_bias = n/128 with small integers n, so every product and partial sum is
representable and the logits and keys are the same in any summation order --
the index comparisons need no exclusions.  fp32 outputs: 2e-6 absolute, the
bound of tests/test_gpu_kernels.py (lse: times max(1, |lse|))."""
from __future__ import annotations

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# T, d, E, k, tpi, n_ctx: a partial last block, E not a power of two, both wave layouts (E <= 32 / 64), three row
# chunks (d 384), the LDS limit (E d 4 = 64 KiB)
SHAPES = [(1, 128, 1, 1, 1, 1), (17, 128, 3, 2, 17, 2), (40, 256, 8, 2, 10, 6), (33, 384, 5, 3, 11, 6),
          (48, 256, 16, 2, 16, 6), (36, 256, 32, 4, 12, 6), (20, 256, 64, 8, 10, 6), (35, 1024, 16, 2, 7, 6)]


def _ints(g, lo, hi, shape, div):
    return torch.randint(lo, hi + 1, shape, generator=g).float() / div


@functools.lru_cache(maxsize=None)
def _case(T, d, E, k, tpi, n_ctx, seed=0):
    """Exact router inputs on the CPU (fp32; x also representable in bf16)."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * T + E)
    return dict(x=_ints(g, -8, 8, (T, d), 8), wg=_ints(g, -4, 4, (E, d), 16), cb=_ints(g, -64, 64, (n_ctx, E), 64),
                sb=_ints(g, -256, 256, (E,), 128), ci=torch.randint(0, n_ctx, (T // tpi,), generator=g).int())


@functools.lru_cache(maxsize=None)
def _reference(T, d, E, k, tpi, n_ctx, normalize=True, biased=True, seed=0):
    from src.moe.eager import route

    c = _case(T, d, E, k, tpi, n_ctx, seed)
    return route(c["x"], c["wg"], c["cb"], c["ci"], tpi, k, normalize, c["sb"] if biased else None)


def _gpu(c):
    return (c["x"].to(torch.bfloat16).to(DEV), c["wg"].to(DEV), c["cb"].to(DEV), c["ci"].to(DEV))


def _close(got, want, what, scale=1.0):
    err = float((got.detach().float().cpu() - want).abs().max())
    print(f"{what}: max abs error {err:.3e} (bound {2e-6 * scale:.3e})")
    assert err <= 2e-6 * scale, what


def _check_ranks(idx, lrank, bcnt, E):
    """local_rank / block_counts restated from idx (16-token router blocks)."""
    from src.moe import _lib as L

    idx, lrank, bcnt = idx.cpu().long(), lrank.cpu().long(), bcnt.cpu().long()
    T, k = idx.shape
    B = L.ROUTER_BLOCK_TOKENS
    for b in range(bcnt.shape[0]):
        blk = idx[b * B:(b + 1) * B]
        for j in range(k):
            assert torch.equal(bcnt[b, j], torch.bincount(blk[:, j], minlength=E))
            seen = {}
            for t in range(blk.shape[0]):
                e = int(blk[t, j])
                assert int(lrank[b * B + t, j]) == seen.get(e, 0)
                seen[e] = seen.get(e, 0) + 1


@pytest.mark.parametrize("T,d,E,k,tpi,n_ctx", SHAPES)
def test_kernel_against_reference(hip_lib, T, d, E, k, tpi, n_ctx):
    from src.moe import _lib as L

    c = _case(T, d, E, k, tpi, n_ctx)
    probs_r, lse_r, idx_r, w_r = _reference(T, d, E, k, tpi, n_ctx)
    idx_plain = _reference(T, d, E, k, tpi, n_ctx, biased=False)[2]
    x, wg, cb, ci = _gpu(c)
    sb = c["sb"].to(DEV)
    idx, w, probs, lse, lrank, bcnt, auxp = L.router_topk_fwd(x, wg, cb, ci, tpi, k, True, sel_bias=sb)
    pos, tok, hist, offsets, _, _, _ = L.route_dispatch(bcnt, idx, lrank, w, auxp, T, E, 0, T * k)
    torch.cuda.synchronize()
    changed = int((idx_r != idx_plain).any(1).sum())
    print(f"tokens whose selection the bias changes: {changed} of {T}")
    assert changed > 0 or E == 1  # the bias matters in this draw
    assert torch.equal(idx.cpu().long(), idx_r)
    assert torch.equal(hist.cpu().long(), torch.bincount(idx_r.reshape(-1), minlength=E))
    _check_ranks(idx, lrank, bcnt, E)
    _close(probs, probs_r, "probs")
    _close(lse, lse_r, "lse", max(1.0, float(lse_r.abs().max())))
    _close(w, w_r, "w")
    # normalize=False: the gate is, bit for bit, the unbiased probability the same call wrote
    idx2, w2, probs2, *_ = L.router_topk_fwd(x, wg, cb, ci, tpi, k, False, sel_bias=sb)
    torch.cuda.synchronize()
    assert torch.equal(idx2, idx)
    assert torch.equal(w2, probs2.gather(1, idx2.long()))


@pytest.mark.parametrize("T,d,E,k,tpi,n_ctx", SHAPES)
def test_zero_bias_and_none(hip_lib, T, d, E, k, tpi, n_ctx):
    from src.moe import _lib as L

    x, wg, cb, ci = _gpu(_case(T, d, E, k, tpi, n_ctx))
    old = L.router_topk_fwd(x, wg, cb, ci, tpi, k, True)
    zero = L.router_topk_fwd(x, wg, cb, ci, tpi, k, True, sel_bias=torch.zeros(E, device=DEV))
    none = L.router_topk_fwd(x, wg, cb, ci, tpi, k, True, sel_bias=None)
    torch.cuda.synchronize()
    names = ("idx", "w", "probs", "lse", "local_rank", "block_counts", "aux_partials")
    for name, a, z, n in zip(names, old, zero, none):
        assert torch.equal(a, n), name  # None is the old entry
        if a.dtype == torch.int32:
            assert torch.equal(a, z), name
        else:
            _close(z, a.cpu(), name + " (zero bias)")


def test_none_calls_the_old_entry(hip_lib, monkeypatch):
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
    torch.cuda.synchronize()
    assert calls == ["moe_router_topk_fwd", "moe_router_topk_fwd_sel"]


def _run_idx(c, tpi, k, sb):
    from src.moe import _lib as L
    from src.moe.eager import route

    x, wg, cb, ci = _gpu(c)
    idx = L.router_topk_fwd(x, wg, cb, ci, tpi, k, True, sel_bias=sb.to(DEV))[0]
    torch.cuda.synchronize()
    ref = route(c["x"], c["wg"], c["cb"], c["ci"], tpi, k, True, sb)[2]
    return idx.cpu().long(), ref


@pytest.mark.parametrize("shape,pairs", [((40, 256, 8, 2, 10, 6), ((0, 1), (6, 7))),
                                         ((20, 256, 64, 8, 10, 6), ((0, 1), (30, 47), (62, 63)))])
def test_ties_go_to_the_lower_id(hip_lib, shape, pairs):
    """Duplicated router rows with equal biases: equal keys at a low and a high
    expert id, inside the selection and across the rank-k boundary."""
    T, d, E, k, tpi, n_ctx = shape
    c = {n: v.clone() for n, v in _case(*shape, seed=1).items()}
    for a, b in pairs:
        c["wg"][b] = c["wg"][a]
        c["cb"][:, b] = c["cb"][:, a]
        c["sb"][b] = c["sb"][a]
    idx, ref = _run_idx(c, tpi, k, c["sb"])
    assert torch.equal(idx, ref)
    inside = boundary = 0
    for a, b in pairs:
        has_a, has_b = (ref == a).any(1), (ref == b).any(1)
        assert not (has_b & ~has_a).any()  # never the higher id alone
        inside += int((has_a & has_b).sum())
        boundary += int((has_a & ~has_b).sum())  # the pair straddles rank k: the lower id is in, its twin out
        both = has_a & has_b
        pa = (ref == a).float().argmax(1)
        pb = (ref == b).float().argmax(1)
        assert bool((pa[both] < pb[both]).all())  # descending key, ties in id order
    print(f"ties inside the selection {inside}, across the rank-k boundary {boundary}")
    assert inside > 0 and boundary > 0


def test_tie_made_by_the_bias_alone(hip_lib):
    """Equal router rows a < b whose context biases differ by 0.5 and whose
    selection biases differ by -0.5: different logits, equal keys."""
    shape = (40, 256, 8, 2, 10, 6)
    T, d, E, k, tpi, n_ctx = shape
    c = {n: v.clone() for n, v in _case(*shape, seed=2).items()}
    a, b = 2, 5
    c["wg"][b] = c["wg"][a]
    c["cb"][:, b] = c["cb"][:, a] + 0.5
    c["sb"][b] = c["sb"][a] - 0.5
    idx, ref = _run_idx(c, tpi, k, c["sb"])
    assert torch.equal(idx, ref)
    has_a, has_b = (ref == a).any(1), (ref == b).any(1)
    assert not (has_b & ~has_a).any() and int((has_a & ~has_b).sum()) > 0
    # without the selection bias the larger logit, b's, goes first
    plain = _run_idx(c, tpi, k, torch.zeros(E))[0]
    assert not ((plain == a).any(1) & ~(plain == b).any(1)).any()


@pytest.mark.parametrize("T,d,E,k,tpi,n_ctx", [SHAPES[4], SHAPES[5], SHAPES[6]])
def test_rounding_order(hip_lib, T, d, E, k, tpi, n_ctx):
    """sel_bias near 2^17: the add rounds to 1/64, so the order of the keys is
    that of the reference only if the kernel forms fl(fl(dot + ctx) + sel).
    In these draws the rounding changes the selection of 2 or 3 tokens."""
    c = _case(T, d, E, k, tpi, n_ctx)
    sb = 131072.0 + c["sb"]
    idx, ref = _run_idx(c, tpi, k, sb)
    small = _reference(T, d, E, k, tpi, n_ctx)[2]
    changed = int((ref != small).any(1).sum())
    print(f"tokens whose selection the rounding changes: {changed} of {T}")
    assert changed > 0
    assert torch.equal(idx, ref)


def test_wrong_arguments(hip_lib):
    from src.moe import _lib as L

    x, wg, cb, ci = _gpu(_case(*SHAPES[2]))
    for bad in (torch.zeros(8, dtype=torch.float64, device=DEV), torch.zeros(8), torch.zeros(9, device=DEV),
                torch.zeros((1, 8), device=DEV)):
        with pytest.raises(L.MoEKernelError):
            L.router_topk_fwd(x, wg, cb, ci, 10, 2, True, sel_bias=bad)


# ---------------------------------------------------------------------------
# the layer
# ---------------------------------------------------------------------------
def _rel(a, ref):
    a, ref = a.detach().float().cpu(), ref.detach().float().cpu()
    return float((a - ref).norm() / ref.norm().clamp(min=1e-30))


LAYERS = [(40, 256, 8, 256, 2, 10, 0.0), (36, 256, 32, 256, 4, 12, 1.25)]
GRADS = ("x", "wg", "cb", "w1", "b1", "w2", "b2")


@pytest.mark.parametrize("expert_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("T,d,E,F,k,tpi,cf", LAYERS)
def test_layer_forward_backward(hip_lib, T, d, E, F, k, tpi, cf, expert_dtype):
    """moe_ffn_hip(..., sel_bias) against moe_ffn_eager(..., sel_bias): hist and
    pos exact; y and every gradient at most twice as far from the eager layer
    as the unbiased GPU layer is from the unbiased eager layer on the same
    inputs -- both pairs run the same kernels, the bias only picks other rows."""
    import math

    from src.moe import _lib as L
    from src.moe.eager import moe_ffn_eager, route_dispatch_eager
    from src.moe.ops import moe_ffn_hip

    c = _case(T, d, E, k, tpi, 6)
    cap = 0 if cf <= 0 else int(math.ceil(cf * T * k / E))
    g = torch.Generator().manual_seed(7)
    bf = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    w1 = bf((torch.rand(E, F, d, generator=g) * 2 - 1) / math.sqrt(d))
    b1 = bf((torch.rand(E, F, generator=g) * 2 - 1) / math.sqrt(d))
    w2 = bf((torch.rand(E, d, F, generator=g) * 2 - 1) / math.sqrt(F))
    b2 = bf((torch.rand(E, d, generator=g) * 2 - 1) / math.sqrt(F))
    dy = bf(torch.randn(T, d, generator=g))
    base = dict(x=c["x"], wg=c["wg"], cb=c["cb"], w1=w1, b1=b1, w2=w2, b2=b2)

    def run(dev, sb):
        p = {n: v.clone().to(dev).requires_grad_(True) for n, v in base.items()}
        if dev != "cpu":
            p["x"] = base["x"].to(torch.bfloat16).to(dev).requires_grad_(True)
        fn = moe_ffn_eager if dev == "cpu" else moe_ffn_hip
        sbd = None if sb is None else sb.to(dev)
        y, lb, z, hist = fn(p["x"], p["wg"], p["cb"], p["w1"], p["b1"], p["w2"], p["b2"], c["ci"].to(dev), tpi, k,
                            True, cap, expert_dtype, sel_bias=sbd)
        ((y.float() * dy.to(dev)).sum() + 0.7 * lb + 0.3 * z).backward()
        if dev != "cpu":
            torch.cuda.synchronize()
        return dict(y=y, hist=hist, **{"d" + n: p[n].grad for n in GRADS})

    errs = {}
    for tag, sb in (("biased", c["sb"]), ("unbiased", None)):
        got, ref = run(DEV, sb), run("cpu", sb)
        assert torch.equal(got["hist"].cpu(), ref["hist"]), tag
        errs[tag] = {n: _rel(got[n], ref[n]) for n in ["y"] + ["d" + n for n in GRADS]}
        # pos, from the layer's two routing launches
        x, wg, cb, ci = _gpu(c)
        idx, w, probs, lse, lrank, bcnt, auxp = L.router_topk_fwd(x, wg, cb, ci, tpi, k, True,
                                                                   sel_bias=None if sb is None else sb.to(DEV))
        rows = T * k if cap <= 0 else min(T * k, E * cap)
        pos = L.route_dispatch(bcnt, idx, lrank, w, auxp, T, E, cap, rows)[0]
        pos_r = route_dispatch_eager(c["x"], c["wg"], c["cb"], c["ci"], tpi, k, True, cap, sel_bias=sb)[4]
        assert torch.equal(pos.cpu().long(), pos_r), tag
    assert not torch.equal(run("cpu", c["sb"])["hist"], run("cpu", None)["hist"])  # the bias moves assignments
    for n in errs["biased"]:
        print(f"{expert_dtype} E{E} {n}: relative Frobenius error biased {errs['biased'][n]:.3e}, "
              f"unbiased {errs['unbiased'][n]:.3e}")
    for n in errs["biased"]:
        assert errs["biased"][n] <= 2.0 * errs["unbiased"][n], n


def test_ep_layer_routes_like_the_plain_layer(hip_lib, monkeypatch):
    """An -ep1 layer (no process group) with a selection bias selects the same
    experts as the non-EP layer with the same weights."""
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
        m = MoEFFN(d, MoEConfig(num_experts=E, top_k=k, hidden=256, balance_rate=0.25, expert_parallel=ep)).to(DEV)
        with torch.no_grad():
            m.wg.copy_(c["wg"])
            m.ctx_bias.copy_(c["cb"])
            m.sel_bias.copy_(c["sb"])
        m(c["x"].to(torch.bfloat16).to(DEV).view(T // tpi, tpi, d), c["ci"].to(DEV))
        layers.append(m)
    torch.cuda.synchronize()
    assert len(seen) == 2 and all(sb is not None for _, sb in seen)
    assert torch.equal(seen[0][0], seen[1][0])
    assert torch.equal(seen[0][0].cpu().long(), _reference(T, d, E, k, tpi, n_ctx)[2])
    assert torch.equal(layers[0].last_hist, layers[1].last_hist)
    assert torch.equal(layers[0].last_hist.cpu().long(), torch.bincount(seen[0][0].reshape(-1).cpu(), minlength=E))
