"""Loss-free expert load balancing on the CPU route (src/moe/balance.py, Wang
et al. 2024): the spec tokens, the selection rule of eager.route, the update
rule balance_reference on hand-worked numbers, and the plumbing -- TrainStep
(one update per optimizer step), checkpoints, the weight average and data
parallelism over gloo.  The reference (scaleoutsystems/multimodal-MoE) plans
"load-balancing terms" for its MoE (notes/MoE_in_ZOD_Thesis_Proposal_
revisedTimeline.txt:214-220) and has none yet."""
from __future__ import annotations

import functools
import os
import socket
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parents[1]
SPEC = "rtdetr-r18-moe4-top1-alb0.25"
NB = 2.0


# ---------------------------------------------------------------------------
# spec tokens
# ---------------------------------------------------------------------------
def test_spec_tokens():
    from src.moe.config import MoEConfig, parse_moe_spec

    assert MoEConfig().balance_rate == 0.0 and parse_moe_spec("rtdetr-r50-moe8-top2").moe.balance_rate == 0.0
    s = parse_moe_spec("rtdetr-r50-moe8-top2-alb")
    assert s.moe.balance_rate == 1e-3 and s.moe.lb_coef == 1e-2 and (s.moe.num_experts, s.moe.top_k) == (8, 2)
    assert parse_moe_spec("rtdetr-r50-moe8-top2-alb0.01").moe.balance_rate == 0.01
    assert parse_moe_spec("rtdetr-r50-moe8-top2-lb0").moe.lb_coef == 0.0
    assert parse_moe_spec("rtdetr-r50-moe8-top2-lb0.5").moe.lb_coef == 0.5
    assert parse_moe_spec("rtdetr-r18-alb").moe is not None  # implies a MoE config, as -top does
    assert parse_moe_spec("rtdetr-r18-lb0").moe is not None
    s = parse_moe_spec("rtdetr-r50-moe8-top2-alb-lb0-mosaic-ema")
    assert (s.moe.balance_rate, s.moe.lb_coef, s.mosaic, s.augment, s.ema_decay) == (1e-3, 0.0, 1.0, True, 0.9999)
    s = parse_moe_spec("rtdetr-r50-moe8-top2-aug-ema0.5-alb0.5-lb0")
    assert (s.moe.balance_rate, s.moe.lb_coef, s.mosaic, s.augment, s.ema_decay) == (0.5, 0.0, 0.0, True, 0.5)
    for bad in ("rtdetr-r50-moe8-top2-alb0", "rtdetr-r50-moe8-top2-albx", "rtdetr-r50-moe8-top2-lb-1",
                "rtdetr-r50-moe8-top2-lb", "rtdetr-r50-moe8-top2-lbx"):
        with pytest.raises(ValueError):
            parse_moe_spec(bad)


# ---------------------------------------------------------------------------
# the selection rule
# ---------------------------------------------------------------------------
def test_route_by_hand():
    """3 tokens, d 2, E 3.  logits = [[1, 0, .5], [0, 1, .5], [1, 1, 1]]."""
    from src.moe.eager import route

    x = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    wg = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.5, 0.5]])
    logits = torch.tensor([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [1.0, 1.0, 1.0]])
    probs_want = torch.softmax(logits, -1)

    def run(k, sb, normalize=True):
        return route(x, wg, None, None, 3, k, normalize, None if sb is None else torch.tensor(sb))

    probs, lse, idx, w = run(1, None)
    assert idx.tolist() == [[0], [1], [0]]  # token 2: a three-way tie -> the lowest id
    base = (probs, lse, idx, w)
    for got, want in zip(run(1, [0.0, 0.0, 0.0]), base):  # a zero bias changes nothing
        assert torch.equal(got, want)
    # expert 2 lifted by 0.75: keys [1, 0, 1.25], [0, 1, 1.25], [1, 1, 1.75] -> expert 2 everywhere
    probs, lse, idx, w = run(1, [0.0, 0.0, 0.75])
    assert idx.tolist() == [[2], [2], [2]]
    assert torch.equal(probs, base[0]) and torch.equal(lse, base[1])  # softmax and lse never see the bias
    torch.testing.assert_close(probs, probs_want)
    assert torch.equal(w, probs[:, 2:3])  # the gate is the UNBIASED probability of the chosen expert
    # lifted by exactly 0.5: keys [1, 0, 1], [0, 1, 1], [1, 1, 1.5]: tokens 0 and 1 have ties made by the
    # bias alone -> the lower id wins
    assert run(1, [0.0, 0.0, 0.5])[2].tolist() == [[0], [1], [2]]
    # k = 2, keys with bias [0, 0.25, 0.75]: [1, .25, 1.25], [0, 1.25, 1.25], [1, 1.25, 1.75]
    probs, lse, idx, w = run(2, [0.0, 0.25, 0.75])
    assert idx.tolist() == [[2, 0], [1, 2], [2, 1]]
    psel = probs.gather(1, idx)
    assert torch.equal(w, psel / psel.sum(-1, keepdim=True))  # renormalised unbiased probabilities
    assert torch.equal(run(2, [0.0, 0.25, 0.75], normalize=False)[3], psel)
    # no gradient reaches the bias; the gates' gradient reaches the router weights as before
    sb = torch.tensor([0.0, 0.25, 0.75], requires_grad=True)
    wgr = wg.clone().requires_grad_(True)
    route(x, wgr, None, None, 3, 2, True, sb)[3].sum().backward()
    assert sb.grad is None and wgr.grad is not None


def test_dispatch_and_layer_take_the_bias():
    from src.moe.eager import moe_ffn_eager, route_dispatch_eager

    torch.manual_seed(0)
    T, d, E, F, k = 12, 8, 4, 16, 2
    x, wg = torch.randn(T, d), torch.randn(E, d)
    w1, b1, w2, b2 = torch.randn(E, F, d), torch.randn(E, F), torch.randn(E, d, F), torch.randn(E, d)
    sb = torch.tensor([0.0, 0.0, 0.0, 100.0])  # every token takes expert 3 first
    hist = route_dispatch_eager(x, wg, None, None, T, k, True, 0, sel_bias=sb)[5]
    assert int(hist[3]) == T and int(hist.sum()) == T * k
    y0, _, _, h0 = moe_ffn_eager(x, wg, None, w1, b1, w2, b2, None, T, k, True, 0)
    y1, _, _, h1 = moe_ffn_eager(x, wg, None, w1, b1, w2, b2, None, T, k, True, 0, sel_bias=sb)
    assert int(h1[3]) == T and not torch.equal(h0, h1) and not torch.equal(y0, y1)
    y2, _, _, h2 = moe_ffn_eager(x, wg, None, w1, b1, w2, b2, None, T, k, True, 0, sel_bias=None)
    assert torch.equal(y0, y2) and torch.equal(h0, h2)


# ---------------------------------------------------------------------------
# the update rule
# ---------------------------------------------------------------------------
def test_balance_reference_by_hand():
    from src.moe.balance import balance_reference

    load = torch.tensor([[1, 4, 8, 3],      # total 16, mean 4: signs +, 0, -, +
                         [0, 0, 0, 0],      # no load: nothing moves
                         [2, 2, 2, 2],      # every load is the mean: only the recentring acts
                         [3 * 10**9, 10**9, 0, 0]], dtype=torch.int64)  # sums past 2^31
    bias = torch.tensor([[0.0, 0.0, 0.0, 0.0], [0.1, 0.2, 0.3, 0.4], [1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.0, 0.0]])
    start = bias.clone()
    maxvio = balance_reference(load, bias, 0.25)
    # layer 0: [.25, 0, -.25, .25] recentred by its minimum -.25
    assert bias[0].tolist() == [0.5, 0.25, 0.0, 0.5] and float(maxvio[0]) == (4 * 8 - 16) / 16
    assert torch.equal(bias[1], start[1]) and float(maxvio[1]) == 0.0  # not even recentred
    assert bias[2].tolist() == [0.0, 1.0, 2.0, 3.0] and float(maxvio[2]) == 0.0
    # layer 3: mean 1e9: signs -, 0, +, + -> [-.25, 0, .25, .25] + .25; max violation 3e9 / 1e9 - 1 = 2
    assert bias[3].tolist() == [0.0, 0.25, 0.5, 0.5] and float(maxvio[3]) == 2.0
    assert maxvio.dtype == torch.float32 and int(load.abs().sum()) == 0  # the load is spent
    # the rate is rounded to fp32 first, and the sum once more: fl32(fl32(1) + fl32(1e-3))
    b = torch.ones(1, 2)
    balance_reference(torch.tensor([[0, 2]]), b, 1e-3)
    r32 = torch.tensor(1e-3, dtype=torch.float32)
    want = torch.stack([torch.ones(()) + r32, torch.ones(()) - r32])
    assert torch.equal(b[0], want - want.min())


# ---------------------------------------------------------------------------
# TrainStep, the weight average, checkpoints
# ---------------------------------------------------------------------------
def _batches():
    from src.rtdetr_moe.data import SyntheticZOD

    return [SyntheticZOD(batch=1, img_h=128, img_w=128, seed=s).sample() for s in (3, 4)]


def _biases(step):
    return torch.stack([m.sel_bias.detach().clone() for m in step.balancer.layers])


def _hists(step):
    return torch.stack([m.last_hist.detach().to(torch.int64) for m in step.balancer.layers])


@functools.lru_cache(maxsize=None)
def _scenario():
    """Two calls of a CPU step with accumulate=2 and a weight average."""
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.step import TrainStep

    torch.manual_seed(0)
    model = RTDETRMoE(SPEC + "-ema0.5")
    b1, b2 = _batches()
    step = TrainStep(model, SetCriterion(num_classes=1), b1[0], b1[2], graphs=False, lr=1e-3, accumulate=2)
    r = {"step": step, "model": model, "bias0": _biases(step)}
    r["shadow0"] = {k: v.clone() for k, v in step.ema.shadow.items() if k.endswith("sel_bias")}
    step(b1[0], b1[2], b1[1], NB)
    r["bias1"], r["hist1"], r["load1"] = _biases(step), _hists(step), step.balancer.load.clone()
    r["counters1"] = (step.micro_steps, step.opt_steps, step.ema.updates)
    step(b2[0], b2[2], b2[1], NB)
    r["bias2"], r["hist2"], r["load2"] = _biases(step), _hists(step), step.balancer.load.clone()
    r["counters2"] = (step.micro_steps, step.opt_steps, step.ema.updates)
    r["maxvio2"] = step.balancer.maxvio.clone()
    r["shadow2"] = {k: v.clone() for k, v in step.ema.shadow.items() if k.endswith("sel_bias")}
    return r


def test_train_step_updates_once_per_optimizer_step():
    from src.moe.balance import balance_reference

    r = _scenario()
    step = r["step"]
    assert step.balancer is not None and step.balancer.L == 4 and step.balancer.E == 4  # AIFI + 3 decoder layers
    assert int(r["bias0"].abs().sum()) == 0
    # inside the cycle: the load is held, nothing moves
    assert torch.equal(r["bias1"], r["bias0"]) and torch.equal(r["load1"], r["hist1"])
    assert r["counters1"] == (1, 0, 0)
    # the optimizer step: one update on the two micro-steps' summed load
    assert r["counters2"] == (2, 1, 1)
    load, want = r["hist1"] + r["hist2"], r["bias0"].clone()
    maxvio = balance_reference(load, want, 0.25)
    assert torch.equal(r["bias2"], want) and torch.equal(r["maxvio2"], maxvio)
    assert not torch.equal(r["bias2"], r["bias0"]) and int(r["load2"].abs().sum()) == 0
    assert all(float(m.last_maxvio) == float(v) for m, v in zip(step.balancer.layers, maxvio))


def test_weight_average_blends_the_bias():
    from src.rtdetr_moe.ema import _blend_, ema_decay_at

    r = _scenario()
    names = [k for k in r["model"].state_dict() if k.endswith("sel_bias")]
    assert len(names) == 4 and set(r["shadow2"]) == set(names)
    live = r["model"].state_dict()
    for k in names:
        want = r["shadow0"][k].clone()
        _blend_(want, live[k], ema_decay_at(1, 0.5, 2000.0))
        assert torch.equal(r["shadow2"][k], want), k
        assert float(want.abs().sum()) > 0
    assert all(torch.equal(r["step"].ema.state_dict()[k], r["shadow2"][k]) for k in names)


def test_engine_reports_the_violation():
    from src.rtdetr_moe.engine import _moe_stats
    from src.rtdetr_moe.model import RTDETRMoE

    r = _scenario()
    stats = _moe_stats(r["model"])
    assert [float(v) for v in r["maxvio2"]] == [stats[f"moe/l{i}_maxvio"] for i in range(4)]
    assert not any(k.endswith("_maxvio") for k in _moe_stats(RTDETRMoE("rtdetr-r18-moe4-top1-dec1")))


def test_checkpoint_round_trip(tmp_path):
    from src.rtdetr_moe.engine import load_model, save_checkpoint

    r = _scenario()
    model = r["model"]
    save_checkpoint(tmp_path / "ck.pt", model, 0, 0.0)
    ck = torch.load(tmp_path / "ck.pt", map_location="cpu", weights_only=True)
    assert ck["moe_cfg"]["balance_rate"] == 0.25
    back = load_model(tmp_path / "ck.pt")
    want = {k: v for k, v in model.state_dict().items() if k.endswith("sel_bias")}
    got = {k: v for k, v in back.state_dict().items() if k.endswith("sel_bias")}
    assert len(want) == 4 and set(got) == set(want)
    assert all(torch.equal(got[k], want[k]) and got[k].dtype == torch.float32 for k in want)
    assert any(float(v.abs().sum()) > 0 for v in want.values())


def test_off_without_the_token():
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.step import TrainStep

    torch.manual_seed(0)
    model = RTDETRMoE("rtdetr-r18-moe4-top1-dec1")
    b1 = _batches()[0]
    step = TrainStep(model, SetCriterion(num_classes=1), b1[0], b1[2], graphs=False)
    assert step.balancer is None and not any("sel_bias" in k for k in model.state_dict())
    assert all(m.sel_bias is None and m.last_maxvio is None for m in model.moe_layers())


# ---------------------------------------------------------------------------
# data parallelism: two ranks over gloo, one image each
# ---------------------------------------------------------------------------
DP_SPEC = "rtdetr-r18-moe4-top2-dec1-alb0.25"


def _dp_model():
    from src.rtdetr_moe.model import RTDETRMoE

    torch.manual_seed(0)
    m = RTDETRMoE(DP_SPEC)
    for mod in m.modules():  # eval-mode BN: per-rank batch statistics would differ from the full batch
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eval()
    return m


def _dp_batch():
    from src.rtdetr_moe.data import SyntheticZOD

    return SyntheticZOD(batch=2, img_h=128, img_w=128, seed=5).sample()


def _dp_worker(rank, world, port, out):
    for p in (str(ROOT / "multimodal-moe_amd"), str(ROOT)):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.step import TrainStep

    images, targets, ctx = _dp_batch()
    sl = slice(rank, rank + 1)
    step = TrainStep(_dp_model(), SetCriterion(num_classes=1), images[sl], ctx[sl], graphs=False, world=world, lr=1e-3)
    assert step.ddp is not None and step.balancer.world == world
    step(images[sl], ctx[sl], targets[sl], NB)
    torch.save({"bias": _biases(step), "hist": _hists(step), "load": step.balancer.load.clone()}, out / f"r{rank}.pt")
    dist.destroy_process_group()


@pytest.mark.slow
def test_gloo_two_ranks_share_one_update(tmp_path):
    from src.moe.balance import balance_reference
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.step import TrainStep

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_dp_worker, args=(2, port, tmp_path), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"r{i}.pt", weights_only=True) for i in range(2))
    assert torch.equal(r0["bias"], r1["bias"]) and float(r0["bias"].abs().sum()) > 0
    assert not torch.equal(r0["hist"], r1["hist"])  # two different images
    assert int(r0["load"].abs().sum()) == 0 and int(r1["load"].abs().sum()) == 0
    # one process on the two-image batch: the same tokens, so the same load, so the same biases
    images, targets, ctx = _dp_batch()
    step = TrainStep(_dp_model(), SetCriterion(num_classes=1), images, ctx, graphs=False, lr=1e-3)
    step(images, ctx, targets, NB)
    assert torch.equal(_hists(step), r0["hist"] + r1["hist"])
    assert torch.equal(_biases(step), r0["bias"])
    want = torch.zeros_like(r0["bias"])
    balance_reference(r0["hist"] + r1["hist"], want, 0.25)
    assert torch.equal(want, r0["bias"])
