"""moe_balance_step_ctx (csrc/balance.hip), the per-context selection biases'
update of every MoE layer in one launch, bit for bit against its statement in
torch ops: balance.context_counts for the counting and balance_reference on
the [L * C, E] rows for the rule.  Integer counts, integer sums and
comparisons, one fp32 add and one subtraction per bias, one double division
per row: nothing depends on an order, so the comparison is exact."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
RATE = 1e-3
BATCHES = ("mixed", "single", "out_of_range")


def _table(idxs, biases, ctxs, tpis):
    """idxs None: NULL topk_idx pointers (the apply after a sum over ranks)."""
    from src.moe.balance import _REC_CTX

    rec = np.zeros(len(biases), dtype=_REC_CTX)
    for i, b in enumerate(biases):
        rec[i]["topk_idx"] = 0 if idxs is None or idxs[i] is None else idxs[i].data_ptr()
        rec[i]["bias"] = b.data_ptr()
        rec[i]["ctx_img"] = ctxs[i].data_ptr()
        rec[i]["T"] = ctxs[i].numel() * tpis[i]
        rec[i]["tokens_per_image"] = tpis[i]
    return torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)


def _draw(L, C, E, k, batch, seed):
    """Per layer: tokens per image 7 / 10 and 3 / 5 images alternately, three
    rounds of top-k indices, the images' contexts, a starting bias and a
    pre-seeded load.  `mixed`: contexts drawn from 0 .. C-2, so the last one is
    absent (C > 1); `single`: every image in context C-1; `out_of_range`:
    mixed with the first image's id set to C (counted nowhere).  L = 7 adds
    the special layers: 1 a load of 3e9 per expert in context 0 (64-bit sums),
    3 no preset load and, at k = 1, one expert with everything, 4 a NULL
    topk_idx pointer in every round and a preset load of 5 everywhere (its
    rows sit exactly at the mean: sign 0, only the recentring acts)."""
    g = torch.Generator().manual_seed(seed)
    tpis = [7 if l % 2 == 0 else 10 for l in range(L)]
    Bs = [3 if l % 2 == 0 else 5 for l in range(L)]
    idxs = [[torch.rand((Bs[l] * tpis[l], E), generator=g).argsort(1)[:, :k].int().contiguous() for l in range(L)]
            for _ in range(3)]
    ctxs = []
    for l in range(L):
        ci = torch.randint(0, max(1, C - 1), (Bs[l],), generator=g).int()
        if batch == "single":
            ci = torch.full((Bs[l],), C - 1, dtype=torch.int32)
        elif batch == "out_of_range":
            ci[0] = C
        ctxs.append(ci)
    bias = torch.randint(-256, 257, (L, C, E), generator=g).float() / 128
    load = torch.randint(0, 50, (L, C, E), generator=g)
    null = set()
    if L == 7:
        load[1, 0] = 3 * 10**9
        load[3] = 0
        if k == 1:
            for r in range(3):
                idxs[r][3].fill_(E - 1)
        load[4] = 5
        null.add(4)
    if C > 1 and batch != "single":
        load[:, C - 1] = 0           # the absent context: a row without load
    return tpis, idxs, ctxs, bias, load, null


CASES = [(L, C, E, k) for L in (1, 7) for C in (1, 6) for E in (1, 5, 8, 64) for k in (1, 2, 8) if k <= E]


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("L,C,E,k", CASES)
def test_accumulate_then_apply(hip_lib, L, C, E, k, batch):
    from src.moe import _lib as lib
    from src.moe.balance import balance_reference, context_counts

    tpis, idxs, ctxs, bias, load, null = _draw(L, C, E, k, batch, 1000 * L + 100 * C + 10 * E + k)
    live = [l for l in range(L) if l not in null]
    # reference
    load_r, bias_r = load.clone(), bias.clone()
    for r in range(3):
        for l in live:
            load_r[l] += context_counts(idxs[r][l], ctxs[l], tpis[l], C, E)
    sums = load_r.clone()
    maxvio_r = balance_reference(load_r.view(-1, E), bias_r.view(-1, E), RATE).view(L, C)
    per_round = sum(int(ctxs[l].numel()) * tpis[l] * k for l in live)
    counted = int((sums - load).sum())
    if batch == "out_of_range":
        assert counted == 3 * (per_round - sum(tpis[l] * k for l in live))  # one image per layer counted nowhere
    else:
        assert counted == 3 * per_round
    if L == 7:
        assert int(sums[1, 0].sum()) > 2**31
    if C > 1 and batch != "single":
        assert int(sums[:, C - 1].sum()) == 0  # a row without load
    # kernel: three accumulating launches, then the apply with NULL topk_idx pointers (the data-parallel form)
    load_g, bias_g = load.to(DEV), bias.to(DEV)
    biases = [bias_g[l] for l in range(L)]
    cg = [c.to(DEV) for c in ctxs]
    maxvio = torch.full((L, C), -1.0, device=DEV)
    for r in range(3):
        ig = [None if l in null else idxs[r][l].to(DEV) for l in range(L)]
        lib.balance_step_ctx(_table(ig, biases, cg, tpis), L, C, E, k, load_g, RATE, False, maxvio)
        torch.cuda.synchronize()  # ig and the table live until the launch is done
    assert torch.equal(load_g.cpu(), sums) and torch.equal(bias_g.cpu(), bias)  # nothing applied yet
    assert bool((maxvio == -1.0).all())
    lib.balance_step_ctx(_table(None, biases, cg, tpis), L, C, E, k, load_g, RATE, True, maxvio)
    torch.cuda.synchronize()
    assert torch.equal(bias_g.cpu(), bias_r)
    assert torch.equal(maxvio.cpu(), maxvio_r)
    assert int(load_g.abs().sum()) == 0 and int(load_r.abs().sum()) == 0
    empty = sums.sum(2) == 0
    assert torch.equal(bias_g.cpu()[empty], bias[empty]) and float(maxvio.cpu()[empty].abs().sum()) == 0.0  # untouched
    assert float(bias_g.cpu()[~empty].min(1).values.abs().max()) == 0.0  # recentred: each updated row's minimum is 0
    if L == 7:
        at_mean = ~empty[4]  # layer 4: every loaded row exactly at the mean
        assert bool(at_mean.any())
        want = bias[4] - bias[4].min(1, keepdim=True).values
        assert torch.equal(bias_g[4].cpu()[at_mean], want[at_mean]) and float(maxvio[4].abs().sum()) == 0.0
        if k == 1 and batch == "single":  # layer 3: the last expert took everything
            assert float(maxvio[3, C - 1]) == float(E - 1)


@pytest.mark.parametrize("E,k", [(5, 2), (64, 8)])
def test_add_and_apply_in_one_launch(hip_lib, E, k):
    """apply=1 with topk_idx pointers: the single-process form of a step without accumulation."""
    from src.moe import _lib as lib
    from src.moe.balance import balance_reference, context_counts

    L, C = 7, 6
    tpis, idxs, ctxs, bias, load, null = _draw(L, C, E, k, "mixed", 99 + E)
    load_r, bias_r = load.clone(), bias.clone()
    for l in range(L):
        if l not in null:
            load_r[l] += context_counts(idxs[0][l], ctxs[l], tpis[l], C, E)
    maxvio_r = balance_reference(load_r.view(-1, E), bias_r.view(-1, E), 0.25).view(L, C)
    load_g, bias_g = load.to(DEV), bias.to(DEV)
    ig, cg = [None if l in null else t.to(DEV) for l, t in enumerate(idxs[0])], [c.to(DEV) for c in ctxs]
    maxvio = torch.empty((L, C), device=DEV)
    lib.balance_step_ctx(_table(ig, [bias_g[l] for l in range(L)], cg, tpis), L, C, E, k, load_g, 0.25, True, maxvio)
    torch.cuda.synchronize()
    assert torch.equal(bias_g.cpu(), bias_r) and torch.equal(maxvio.cpu(), maxvio_r)
    assert int(load_g.abs().sum()) == 0


def test_expert_ids_out_of_range_count_nowhere(hip_lib):
    from src.moe import _lib as lib
    from src.moe.balance import context_counts

    L, C, E, k, tpi = 1, 2, 5, 2, 7
    g = torch.Generator().manual_seed(4)
    idx = torch.randint(-2, E + 3, (3 * tpi, k), generator=g).int()
    ci = torch.tensor([1, 0, 1], dtype=torch.int32)
    want = context_counts(idx, ci, tpi, C, E)
    assert 0 < int(want.sum()) < idx.numel()
    load = torch.zeros((L, C, E), dtype=torch.int64, device=DEV)
    bias = torch.zeros((C, E), device=DEV)
    ig, cg = idx.to(DEV), ci.to(DEV)
    lib.balance_step_ctx(_table([ig], [bias], [cg], [tpi]), L, C, E, k, load, RATE, False)
    torch.cuda.synchronize()
    assert torch.equal(load[0].cpu(), want)


def test_per_expert_entry_is_unchanged(hip_lib):
    """moe_balance_step now shares the row update with the per-context kernel:
    one of test_gpu_balance_step.py's cases (L 7, E 8) gives what it gave."""
    from src.moe import _lib as lib
    from src.moe.balance import _REC, balance_reference

    L, E = 7, 8
    g = torch.Generator().manual_seed(10 * L + E)
    hists = [[torch.randint(0, 1000, (E,), generator=g).int() for _ in range(L)] for _ in range(3)]
    bias = torch.randint(-256, 257, (L, E), generator=g).float() / 128
    load = torch.randint(0, 50, (L, E), generator=g)
    for r in range(3):
        hists[r][1] = torch.full((E,), 7 + r, dtype=torch.int32)
        hists[r][2] = torch.zeros(E, dtype=torch.int32)
    load[1], load[2], load[3] = 5, 0, 3 * 10**9
    load_r, bias_r = load.clone(), bias.clone()
    for r in range(3):
        for l in range(L):
            load_r[l] += hists[r][l].long()
    maxvio_r = balance_reference(load_r, bias_r, RATE)
    load_g, bias_g = load.to(DEV), bias.to(DEV)
    maxvio = torch.full((L,), -1.0, device=DEV)

    def table(hs):
        rec = np.zeros(L, dtype=_REC)
        for i in range(L):
            rec[i]["hist"] = 0 if hs is None else hs[i].data_ptr()
            rec[i]["bias"] = bias_g[i].data_ptr()
        return torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)

    for r in range(3):
        hg = [h.to(DEV) for h in hists[r]]
        lib.balance_step(table(hg), L, E, load_g, RATE, False, maxvio)
        torch.cuda.synchronize()
    lib.balance_step(table(None), L, E, load_g, RATE, True, maxvio)
    torch.cuda.synchronize()
    assert torch.equal(bias_g.cpu(), bias_r) and torch.equal(maxvio.cpu(), maxvio_r) and int(load_g.abs().sum()) == 0
    assert torch.equal(bias_g[2].cpu(), bias[2]) and float(maxvio[2]) == 0.0 and float(maxvio[1]) == 0.0


def test_arguments(hip_lib):
    from src.moe import _lib as lib

    C, E, k, tpi = 6, 8, 2, 7
    bias = torch.zeros((2, C, E), device=DEV)
    load = torch.zeros((2, C, E), dtype=torch.int64, device=DEV)
    ci = torch.zeros(3, dtype=torch.int32, device=DEV)
    tab = _table(None, [bias[0], bias[1]], [ci, ci], [tpi, tpi])
    s = lib._stream()
    f = hip_lib.moe_balance_step_ctx
    assert f(tab.data_ptr(), 2, C, 0, 1, load.data_ptr(), 0.1, 1, None, s) != 0
    assert f(tab.data_ptr(), 2, C, 65, 2, load.data_ptr(), 0.1, 1, None, s) != 0
    assert f(tab.data_ptr(), 2, C, E, 9, load.data_ptr(), 0.1, 1, None, s) != 0
    assert f(tab.data_ptr(), 2, C, 2, 3, load.data_ptr(), 0.1, 1, None, s) != 0
    assert f(tab.data_ptr(), 2, 0, E, k, load.data_ptr(), 0.1, 1, None, s) != 0
    assert f(tab.data_ptr(), -1, C, E, k, load.data_ptr(), 0.1, 1, None, s) != 0
    assert f(None, 2, C, E, k, load.data_ptr(), 0.1, 1, None, s) != 0
    assert f(None, 0, C, E, k, None, 0.1, 1, None, s) == 0  # no layers: nothing to launch
    with pytest.raises(lib.MoEKernelError):
        lib.balance_step_ctx(tab, 2, C, E, k, load.int(), 0.1, True)
    with pytest.raises(lib.MoEKernelError):
        lib.balance_step_ctx(tab, 2, C, E, k, load.view(2, C * E), 0.1, True)
    with pytest.raises(lib.MoEKernelError):  # table too short
        lib.balance_step_ctx(tab, 3, C, E, k, torch.zeros((3, C, E), dtype=torch.int64, device=DEV), 0.1, True)
    lib.balance_step_ctx(tab, 2, C, E, k, load, 0.1, True)  # maxvio is optional
    torch.cuda.synchronize()
    assert float(bias.abs().sum()) == 0.0  # total 0: nothing moved
