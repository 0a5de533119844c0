"""moe_balance_step (csrc/balance.hip), the selection biases' update of every
MoE layer in one launch, bit for bit against its statement in torch ops,
src/moe/balance.py::balance_reference (integer sums and comparisons, one fp32
add and one subtraction per bias, one double division per layer: nothing in
it depends on an order, so the comparison is exact)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
RATE = 1e-3


def _table(hists, biases):
    from src.moe.balance import _REC

    rec = np.zeros(len(biases), dtype=_REC)
    for i, b in enumerate(biases):
        rec[i]["hist"] = 0 if hists is None or hists[i] is None else hists[i].data_ptr()
        rec[i]["bias"] = b.data_ptr()
    return torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)


def _draw(L, E, seed):
    """Three rounds of hist per layer, a starting bias and a pre-seeded load.
    L = 7 adds the special layers: 1 every expert at the mean (sign 0), 2 no
    load at all, 3 a load of 3e9 per expert and round (64-bit sums), 4 one
    expert with everything, 5 a NULL hist pointer (its seeded load stays)."""
    g = torch.Generator().manual_seed(seed)
    hists = [[torch.randint(0, 1000, (E,), generator=g).int() for _ in range(L)] for _ in range(3)]
    bias = torch.randint(-256, 257, (L, E), generator=g).float() / 128
    load = torch.randint(0, 50, (L, E), generator=g)
    null = set()
    if L == 7:
        for r in range(3):
            hists[r][1] = torch.full((E,), 7 + r, dtype=torch.int32)
            hists[r][2] = torch.zeros(E, dtype=torch.int32)
            hists[r][4] = torch.zeros(E, dtype=torch.int32)
            hists[r][4][E - 1] = 123
        load[1] = 5
        load[2] = 0
        load[3] = 3 * 10**9
        load[4] = 0
        null.add(5)
    return hists, bias, load, null


@pytest.mark.parametrize("E", [1, 5, 8, 64])
@pytest.mark.parametrize("L", [1, 7])
def test_accumulate_then_apply(hip_lib, L, E):
    from src.moe import _lib as lib
    from src.moe.balance import balance_reference

    hists, bias, load, null = _draw(L, E, 10 * L + E)
    # reference
    load_r, bias_r = load.clone(), bias.clone()
    for r in range(3):
        for l in range(L):
            if l not in null:
                load_r[l] += hists[r][l].long()
    sums = load_r.clone()
    maxvio_r = balance_reference(load_r, bias_r, RATE)
    if L == 7:
        assert int(sums[3].sum()) > 2**31 and int(sums[2].sum()) == 0 and len(set(sums[1].tolist())) == 1
    # kernel: three accumulating launches, then the apply with NULL hist pointers (the data-parallel form)
    load_g, bias_g = load.to(DEV), bias.to(DEV)
    biases = [bias_g[l] for l in range(L)]
    maxvio = torch.full((L,), -1.0, device=DEV)
    for r in range(3):
        hg = [None if l in null else hists[r][l].to(DEV) for l in range(L)]
        lib.balance_step(_table(hg, biases), L, E, load_g, RATE, False, maxvio)
        torch.cuda.synchronize()  # hg and the table live until the launch is done
    assert torch.equal(load_g.cpu(), sums) and torch.equal(bias_g.cpu(), bias)  # nothing applied yet
    assert bool((maxvio == -1.0).all())
    lib.balance_step(_table(None, biases), L, E, load_g, RATE, True, maxvio)
    torch.cuda.synchronize()
    assert torch.equal(bias_g.cpu(), bias_r)
    assert torch.equal(maxvio.cpu(), maxvio_r)
    assert int(load_g.abs().sum()) == 0 and int(load_r.abs().sum()) == 0
    if L == 7:
        assert torch.equal(bias_g[2].cpu(), bias[2]) and float(maxvio[2]) == 0.0  # no load: untouched
        assert torch.equal(bias_g[1].cpu(), bias[1] - bias[1].min()) and float(maxvio[1]) == 0.0  # sign 0
        assert float(maxvio[4]) == float(E - 1)
    assert float(bias_g.min(1).values.abs().max()) == 0.0 or L == 7  # recentred: each layer's minimum is 0


@pytest.mark.parametrize("E", [5, 64])
def test_add_and_apply_in_one_launch(hip_lib, E):
    """apply=1 with hist pointers: the single-process form of a step without accumulation."""
    from src.moe import _lib as lib
    from src.moe.balance import balance_reference

    L = 7
    hists, bias, load, null = _draw(L, E, 99 + E)
    load_r, bias_r = load.clone(), bias.clone()
    for l in range(L):
        if l not in null:
            load_r[l] += hists[0][l].long()
    maxvio_r = balance_reference(load_r, bias_r, 0.25)
    load_g, bias_g = load.to(DEV), bias.to(DEV)
    hg = [None if l in null else hists[0][l].to(DEV) for l in range(L)]
    maxvio = torch.empty(L, device=DEV)
    lib.balance_step(_table(hg, [bias_g[l] for l in range(L)]), L, E, load_g, 0.25, True, maxvio)
    torch.cuda.synchronize()
    assert torch.equal(bias_g.cpu(), bias_r) and torch.equal(maxvio.cpu(), maxvio_r)
    assert int(load_g.abs().sum()) == 0


def test_arguments(hip_lib):
    from src.moe import _lib as lib

    bias = torch.zeros((2, 8), device=DEV)
    load = torch.zeros((2, 8), dtype=torch.int64, device=DEV)
    tab = _table(None, [bias[0], bias[1]])
    s = lib._stream()
    assert hip_lib.moe_balance_step(tab.data_ptr(), 2, 0, load.data_ptr(), 0.1, 1, None, s) != 0
    assert hip_lib.moe_balance_step(tab.data_ptr(), 2, 65, load.data_ptr(), 0.1, 1, None, s) != 0
    assert hip_lib.moe_balance_step(tab.data_ptr(), -1, 8, load.data_ptr(), 0.1, 1, None, s) != 0
    assert hip_lib.moe_balance_step(None, 2, 8, load.data_ptr(), 0.1, 1, None, s) != 0
    assert hip_lib.moe_balance_step(None, 0, 8, None, 0.1, 1, None, s) == 0  # no layers: nothing to launch
    with pytest.raises(lib.MoEKernelError):
        lib.balance_step(tab, 2, 8, load.int(), 0.1, True)
    with pytest.raises(lib.MoEKernelError):
        lib.balance_step(tab, 3, 8, torch.zeros((3, 8), dtype=torch.int64, device=DEV), 0.1, True)  # table too short
    lib.balance_step(tab, 2, 8, load, 0.1, True)  # maxvio is optional
    torch.cuda.synchronize()
    assert float(bias.abs().sum()) == 0.0  # total 0: nothing moved
