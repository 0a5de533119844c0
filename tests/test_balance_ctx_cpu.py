"""Per-context loss-free load balancing on the CPU route (an -albc spec;
src/moe/balance.py): the spec tokens, eager.route with a [C, E] selection bias
on hand-worked numbers, LoadBalancer's per-context counting and update, and
the plumbing -- checkpoints, the weight average, data parallelism over gloo.
The update rule itself is balance_reference's, checked in test_balance_cpu.py;
here it is applied to the [L * C, E] rows."""
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
SPEC = "rtdetr-r18-moe4-top2-dec1-albc0.25"
NB = 2.0


# ---------------------------------------------------------------------------
# spec tokens
# ---------------------------------------------------------------------------
def test_spec_tokens():
    from src.moe.config import MoEConfig, parse_moe_spec

    assert MoEConfig().balance_per_context is False
    s = parse_moe_spec("rtdetr-r50-moe8-top2-albc")
    assert (s.moe.balance_rate, s.moe.balance_per_context, s.moe.lb_coef) == (1e-3, True, 1e-2)
    assert (s.moe.num_experts, s.moe.top_k) == (8, 2)
    s = parse_moe_spec("rtdetr-r50-moe8-top2-albc0.01")
    assert (s.moe.balance_rate, s.moe.balance_per_context) == (0.01, True)
    s = parse_moe_spec("rtdetr-r50-moe8-top2-albc-lb0")
    assert (s.moe.balance_rate, s.moe.balance_per_context, s.moe.lb_coef) == (1e-3, True, 0.0)
    assert parse_moe_spec("rtdetr-r18-albc").moe is not None  # implies a MoE config, as -alb does
    for bad in ("rtdetr-r50-moe8-top2-albc-noctx", "rtdetr-r50-moe8-top2-noctx-albc", "rtdetr-r50-moe8-top2-albc0",
                "rtdetr-r50-moe8-top2-albcx"):
        with pytest.raises(ValueError):
            parse_moe_spec(bad)
    # -alb is parsed as before
    s = parse_moe_spec("rtdetr-r50-moe8-top2-alb")
    assert (s.moe.balance_rate, s.moe.balance_per_context) == (1e-3, False)
    s = parse_moe_spec("rtdetr-r50-moe8-top2-alb0.01-lb0")
    assert (s.moe.balance_rate, s.moe.balance_per_context, s.moe.lb_coef) == (0.01, False, 0.0)
    assert parse_moe_spec("rtdetr-r50-moe8-top2").moe.balance_per_context is False


# ---------------------------------------------------------------------------
# the selection rule
# ---------------------------------------------------------------------------
X = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 1.0]])  # two images of two tokens
WG = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.5, 0.5]])
LOGITS = torch.tensor([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [1.0, 0.0, 0.5], [0.0, 1.0, 0.5]])


def test_route_by_hand_one_image_flips():
    """Image 0 has context 1, image 1 context 0.  Row 1 of the bias lifts expert
    2 by 0.75 (keys [1, 0, 1.25] and [0, 1, 1.25]: expert 2), row 0 is zero."""
    from src.moe.eager import route

    ci = torch.tensor([1, 0], dtype=torch.int32)
    sb = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 0.75]])
    base = route(X, WG, None, ci, 2, 1, True, None)
    assert base[2].tolist() == [[0], [1], [0], [1]]
    probs, lse, idx, w = route(X, WG, None, ci, 2, 1, True, sb)
    assert idx.tolist() == [[2], [2], [0], [1]]  # image 0 flipped, image 1 as without a bias
    assert torch.equal(probs, base[0]) and torch.equal(lse, base[1])  # softmax and lse never see the bias
    # the other way round: the same table, the images' contexts swapped
    assert route(X, WG, None, torch.tensor([0, 1], dtype=torch.int32), 2, 1, True, sb)[2].tolist() == \
        [[0], [1], [2], [2]]
    with pytest.raises(ValueError):
        route(X, WG, None, None, 2, 1, True, sb)  # a [C, E] bias needs the contexts


def test_route_by_hand_gates_are_unbiased():
    """k = 2, row 1 = [0, 0.25, 0.75]: keys [1, .25, 1.25] -> (2, 0), [0, 1.25, 1.25] -> (1, 2) (a tie made by
    the bias: the lower id first); row 0 = [0, 2, 0]: keys [1, 2, .5] -> (1, 0), [0, 3, .5] -> (1, 2)."""
    from src.moe.eager import route

    ci = torch.tensor([1, 0], dtype=torch.int32)
    sb = torch.tensor([[0.0, 2.0, 0.0], [0.0, 0.25, 0.75]])
    probs, lse, idx, w = route(X, WG, None, ci, 2, 2, True, sb)
    assert idx.tolist() == [[2, 0], [1, 2], [1, 0], [1, 2]]
    want = torch.softmax(LOGITS, -1)
    torch.testing.assert_close(probs, want)
    psel = probs.gather(1, idx)
    assert torch.equal(w, psel / psel.sum(-1, keepdim=True))  # renormalised UNBIASED probabilities
    assert torch.equal(route(X, WG, None, ci, 2, 2, False, sb)[3], psel)
    sbr = sb.clone().requires_grad_(True)
    wgr = WG.clone().requires_grad_(True)
    route(X, wgr, None, ci, 2, 2, True, sbr)[3].sum().backward()
    assert sbr.grad is None and wgr.grad is not None


def test_equal_rows_are_the_per_expert_bias():
    from src.moe.eager import route

    g = torch.Generator().manual_seed(3)
    T, d, E, k, tpi, C = 40, 16, 8, 2, 10, 6
    x, wg, cb = torch.randn(T, d, generator=g), torch.randn(E, d, generator=g), torch.randn(C, E, generator=g)
    ci = torch.randint(0, C, (T // tpi,), generator=g).int()
    sb = torch.randn(E, generator=g)
    one = route(x, wg, cb, ci, tpi, k, True, sb)
    tab = route(x, wg, cb, ci, tpi, k, True, sb.expand(C, E).contiguous())
    assert not torch.equal(one[2], route(x, wg, cb, ci, tpi, k, True, None)[2])  # the bias matters in this draw
    for a, b in zip(one, tab):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# LoadBalancer
# ---------------------------------------------------------------------------
def _batch(seed, batch=2):
    from src.rtdetr_moe.data import SyntheticZOD

    return SyntheticZOD(batch=batch, img_h=128, img_w=128, seed=seed).sample()


def _biases(step):
    return torch.stack([m.sel_bias.detach().clone() for m in step.balancer.layers])


def _hists(step):
    return torch.stack([m.last_hist.detach().to(torch.int64) for m in step.balancer.layers])


def _counts(step):
    """[L, C, E] restated from the layers' last_topk_idx / last_ctx with bincount per context."""
    out = []
    for m in step.balancer.layers:
        idx, ci = m.last_topk_idx.long(), m.last_ctx.long()
        C, E = m.sel_bias.shape
        tpi = idx.shape[0] // ci.numel()
        rows = []
        for c in range(C):
            tok = (ci == c).repeat_interleave(tpi)
            rows.append(torch.bincount(idx[tok].reshape(-1), minlength=E))
        out.append(torch.stack(rows))
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def _scenario():
    """Two calls of a CPU step with accumulate=2 and a weight average."""
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.step import TrainStep

    torch.manual_seed(0)
    model = RTDETRMoE(SPEC + "-ema0.5")
    b1, b2 = _batch(5), _batch(6)
    step = TrainStep(model, SetCriterion(num_classes=1), b1[0], b1[2], graphs=False, lr=1e-3, accumulate=2)
    r = {"step": step, "model": model, "bias0": _biases(step), "ctx": (b1[2].clone(), b2[2].clone())}
    r["shadow0"] = {k: v.clone() for k, v in step.ema.shadow.items() if k.endswith("sel_bias")}
    step(b1[0], b1[2], b1[1], NB)
    r["bias1"], r["hist1"], r["cnt1"], r["load1"] = _biases(step), _hists(step), _counts(step), step.balancer.load.clone()
    r["counters1"] = (step.micro_steps, step.opt_steps, step.ema.updates)
    step(b2[0], b2[2], b2[1], NB)
    r["bias2"], r["hist2"], r["cnt2"], r["load2"] = _biases(step), _hists(step), _counts(step), step.balancer.load.clone()
    r["counters2"] = (step.micro_steps, step.opt_steps, step.ema.updates)
    r["maxvio2"] = step.balancer.maxvio.clone()
    r["shadow2"] = {k: v.clone() for k, v in step.ema.shadow.items() if k.endswith("sel_bias")}
    return r


def test_load_is_the_per_context_bincount():
    r = _scenario()
    b = r["step"].balancer
    assert b.per_context and (b.L, b.C, b.E, b.k) == (2, 6, 4, 2)  # AIFI + one decoder layer
    assert tuple(r["bias0"].shape) == (2, 6, 4) and float(r["bias0"].abs().sum()) == 0.0
    assert torch.equal(r["load1"], r["cnt1"])                      # after a forward: bincount per context
    assert torch.equal(r["load1"].sum(1), r["hist1"])              # over the contexts: the layer's hist
    assert torch.equal((r["cnt1"] + r["cnt2"]).sum(1), r["hist1"] + r["hist2"])
    for m in b.layers:
        assert m.last_topk_idx.dtype == torch.int32 and m.last_ctx.dtype == torch.int32
        assert tuple(m.last_topk_idx.shape) == (m.last_tokens, 2)


def test_one_update_per_optimizer_step_and_absent_contexts():
    from src.moe.balance import balance_reference

    r = _scenario()
    step = r["step"]
    assert torch.equal(r["bias1"], r["bias0"]) and r["counters1"] == (1, 0, 0)  # inside the cycle nothing moves
    assert r["counters2"] == (2, 1, 1)
    load, want = r["cnt1"] + r["cnt2"], r["bias0"].clone()
    maxvio = balance_reference(load.view(-1, 4), want.view(-1, 4), 0.25).view(2, 6)
    assert torch.equal(r["bias2"], want) and torch.equal(r["maxvio2"], maxvio)
    assert not torch.equal(r["bias2"], r["bias0"]) and int(r["load2"].abs().sum()) == 0
    seen = set(r["ctx"][0].tolist()) | set(r["ctx"][1].tolist())
    absent = [c for c in range(6) if c not in seen]
    assert absent and len(seen) >= 2
    for c in absent:  # a context without tokens in the optimizer step: row kept, maxvio 0
        assert torch.equal(r["bias2"][:, c], r["bias0"][:, c]) and float(r["maxvio2"][:, c].abs().sum()) == 0.0
    for c in seen:
        assert float(r["bias2"][:, c].abs().sum()) > 0 and float(r["bias2"][:, c].min()) == 0.0
    # the layer's reported violation is the maximum over its contexts
    assert all(float(m.last_maxvio) == float(maxvio[i].max()) for i, m in enumerate(step.balancer.layers))


def test_engine_reports_the_largest_violation():
    from src.rtdetr_moe.engine import _moe_stats

    r = _scenario()
    stats = _moe_stats(r["model"])
    assert [float(v) for v in r["maxvio2"].amax(1)] == [stats[f"moe/l{i}_maxvio"] for i in range(2)]


def test_absent_context_keeps_a_nonzero_row():
    """A row that already holds values is not even recentred when its context
    brings no tokens; out-of-range ids count nowhere."""
    from src.moe.balance import balance_reference, context_counts

    idx = torch.tensor([[0, 1], [1, 2], [1, 3], [7, 0], [2, 3], [3, -1]], dtype=torch.int32)
    ci = torch.tensor([2, 0, 9], dtype=torch.int32)  # image 2's context is out of range: ignored
    cnt = context_counts(idx, ci, 2, 3, 4)
    assert cnt.tolist() == [[1, 1, 0, 1], [0, 0, 0, 0], [1, 2, 1, 0]]  # expert 7 of token 3 counts nowhere
    bias = torch.tensor([[0.0, 0.0, 0.0, 0.0], [0.5, 0.25, 1.0, 0.75], [0.0, 0.0, 0.0, 0.0]])
    maxvio = balance_reference(cnt.clone(), bias, 0.25)
    assert bias[1].tolist() == [0.5, 0.25, 1.0, 0.75] and float(maxvio[1]) == 0.0
    assert bias[2].tolist() == [0.25, 0.0, 0.25, 0.5]  # total 4, mean 1: signs 0, -, 0, + ; recentred by -.25


def test_mixed_models_are_refused():
    from src.moe.balance import LoadBalancer
    from src.moe.config import MoEConfig
    from src.moe.layer import MoEFFN

    a = MoEFFN(16, MoEConfig(num_experts=4, hidden=16, balance_rate=0.1))
    b = MoEFFN(16, MoEConfig(num_experts=4, hidden=16, balance_rate=0.1, balance_per_context=True))
    assert tuple(a.sel_bias.shape) == (4,) and tuple(b.sel_bias.shape) == (6, 4)
    with pytest.raises(ValueError):
        LoadBalancer(torch.nn.ModuleList([a, b]), 0.1)
    with pytest.raises(ValueError):
        MoEFFN(16, MoEConfig(num_experts=4, hidden=16, balance_rate=0.1, balance_per_context=True, use_context=False))
    off = MoEFFN(16, MoEConfig(num_experts=4, hidden=16, balance_per_context=True))  # rate 0: no buffer at all
    assert off.sel_bias is None and "sel_bias" not in off.state_dict()


# ---------------------------------------------------------------------------
# the weight average, checkpoints
# ---------------------------------------------------------------------------
def test_weight_average_blends_the_table():
    from src.rtdetr_moe.ema import _blend_, ema_decay_at

    r = _scenario()
    names = [k for k in r["model"].state_dict() if k.endswith("sel_bias")]
    assert len(names) == 2 and set(r["shadow2"]) == set(names)
    live = r["model"].state_dict()
    for k in names:
        want = r["shadow0"][k].clone()
        _blend_(want, live[k], ema_decay_at(1, 0.5, 2000.0))
        assert tuple(want.shape) == (6, 4) and torch.equal(r["shadow2"][k], want), k
        assert float(want.abs().sum()) > 0


def test_checkpoint_round_trip(tmp_path):
    from src.rtdetr_moe.engine import load_model, save_checkpoint
    from src.rtdetr_moe.model import RTDETRMoE

    r = _scenario()
    model = r["model"]
    save_checkpoint(tmp_path / "ck.pt", model, 0, 0.0)
    ck = torch.load(tmp_path / "ck.pt", map_location="cpu", weights_only=True)
    assert ck["moe_cfg"]["balance_rate"] == 0.25 and ck["moe_cfg"]["balance_per_context"] is True
    back = load_model(tmp_path / "ck.pt")
    want = {k: v for k, v in model.state_dict().items() if k.endswith("sel_bias")}
    got = {k: v for k, v in back.state_dict().items() if k.endswith("sel_bias")}
    assert len(want) == 2 and set(got) == set(want)
    assert all(torch.equal(got[k], want[k]) and got[k].dtype == torch.float32 for k in want)
    assert any(float(v.abs().sum()) > 0 for v in want.values())
    # an -alb checkpoint does not fit an -albc model: the shapes differ, no conversion
    torch.manual_seed(0)
    per_expert = RTDETRMoE(SPEC.replace("albc", "alb"))
    with pytest.raises(RuntimeError):
        model.load_state_dict(per_expert.state_dict())


# ---------------------------------------------------------------------------
# data parallelism: two ranks over gloo, one image each
# ---------------------------------------------------------------------------
def _dp_model():
    from src.rtdetr_moe.model import RTDETRMoE

    torch.manual_seed(0)
    m = RTDETRMoE(SPEC)
    for mod in m.modules():  # eval-mode BN: per-rank batch statistics would differ from the full batch
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eval()
    return m


def _dp_worker(rank, world, port, out):
    for p in (str(ROOT / "multimodal-moe_amd"), str(ROOT)):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.step import TrainStep

    images, targets, ctx = _batch(5)
    sl = slice(rank, rank + 1)
    step = TrainStep(_dp_model(), SetCriterion(num_classes=1), images[sl], ctx[sl], graphs=False, world=world, lr=1e-3)
    assert step.ddp is not None and step.balancer.world == world and step.balancer.per_context
    step(images[sl], ctx[sl], targets[sl], NB)
    torch.save({"bias": _biases(step), "cnt": _counts(step), "load": step.balancer.load.clone()}, out / f"r{rank}.pt")
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
    assert tuple(r0["bias"].shape) == (2, 6, 4)
    assert torch.equal(r0["bias"], r1["bias"]) and float(r0["bias"].abs().sum()) > 0
    assert not torch.equal(r0["cnt"], r1["cnt"])  # two images of different contexts
    assert int(r0["load"].abs().sum()) == 0 and int(r1["load"].abs().sum()) == 0
    # one process on the two-image batch: the same tokens, so the same load, so the same biases
    images, targets, ctx = _batch(5)
    assert int(ctx[0]) != int(ctx[1])
    step = TrainStep(_dp_model(), SetCriterion(num_classes=1), images, ctx, graphs=False, lr=1e-3)
    step(images, ctx, targets, NB)
    assert torch.equal(_counts(step), r0["cnt"] + r1["cnt"])
    assert torch.equal(_biases(step), r0["bias"])
    want = torch.zeros_like(r0["bias"])
    balance_reference((r0["cnt"] + r1["cnt"]).view(-1, 4), want.view(-1, 4), 0.25)
    assert torch.equal(want, r0["bias"])
