"""Gradient accumulation through the training step on the GPU
(step.TrainStep(accumulate=2), the whole step as one hipGraph) and under the
sharded optimizer (optim.ShardedDPAdamW fed by optim.GradAccumulator, two
ranks sharing one GPU over gloo).  The reference's Ultralytics trainer
accumulates nbs / batch batches per optimizer step
(src/models/vision/rtdetr.py:82-94 trains through it).

Model, data and construction follow tests/test_gpu_ema_step.py.  The step's
masters are compared bit for bit with a twin FlatAdamW stepped on the torch
sum of the two micro-steps' gradients; the sharded optimizer against a
single-process FlatAdamW at rtol 2e-5 / atol 1e-7, the project's figure for
fp32 masters under a different operation order (tests/test_gpu_optim.py)."""
from __future__ import annotations

import functools
import os
import socket
import sys
import time
from datetime import timedelta
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parents[1]
SPEC = "rtdetr-r18-moe4-top2-dec2"
NB = 2.0


def _data(dev, seed):
    from src.rtdetr_moe.data import SyntheticZOD

    images, targets, ctx = SyntheticZOD(batch=1, img_h=256, img_w=256, seed=seed).sample(dev)
    images = images.contiguous(memory_format=torch.channels_last)
    return images, ctx, [{k: v.to(dev) for k, v in t.items()} for t in targets], NB


def _model(dev):
    from src.rtdetr_moe.model import RTDETRMoE

    torch.manual_seed(0)
    return RTDETRMoE(SPEC).to(dev).to(memory_format=torch.channels_last)


def _twin_of(opt):
    """A FlatAdamW over copies of ``opt``'s parameters: the same groups,
    hyper-parameters, layout and state."""
    from src.rtdetr_moe.optim import FlatAdamW

    clones = [torch.nn.Parameter(torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=p.device)
                                 .copy_(p.detach())) for p in opt.params]
    groups = [([c for c, g in zip(clones, opt.group_of) if g == gi], lr) for gi, lr in enumerate(opt.lrs)]
    twin = FlatAdamW(groups, weight_decay=opt.wd, betas=(opt.beta1, opt.beta2), eps=opt.eps, clip_norm=opt.clip_norm)
    assert twin.offsets == opt.offsets and twin.group_of == opt.group_of
    for k in ("master", "exp_avg", "exp_avg_sq", "tsteps"):
        getattr(twin, k).copy_(getattr(opt, k))
    return twin


def _weights(opt):
    from src.rtdetr_moe.optim import _storage_flat

    return [_storage_flat(p.detach()).clone() for p in opt.params if p.dtype == torch.bfloat16]


@functools.lru_cache(maxsize=None)
def _two_calls():
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.step import TrainStep

    dev = torch.device("cuda", 0)
    model = _model(dev)
    b1, b2 = _data(dev, 11), _data(dev, 12)
    step = TrainStep(model, SetCriterion(num_classes=1), b1[0], b1[1], graphs=True, lr=1e-3, targets=b1[2],
                     num_boxes=NB, ema_decay=0.5, ema_tau=1.0, accumulate=2)
    opt = step.opt
    assert step.stepper is not None and step.ema is not None and type(opt).__name__ == "FlatAdamW"
    r = {"has_acc": step.acc is not None}
    twin_sum, twin_g2 = _twin_of(opt), _twin_of(opt)  # cloned before the first call
    state = lambda: {k: getattr(opt, k).clone() for k in ("master", "exp_avg", "exp_avg_sq", "tsteps")}  # noqa: E731
    r["state0"], r["weights0"] = state(), _weights(opt)
    r["loss1"] = step(*b1).clone()
    torch.cuda.synchronize()
    r["state1"], r["weights1"] = state(), _weights(opt)
    r["counters1"] = (opt.steps, step.opt_steps, step.micro_steps, step.ema.updates)
    g1 = [p.grad.clone() for p in opt.params]
    r["loss2"] = step(*b2).clone()
    torch.cuda.synchronize()
    r["state2"], r["weights2"] = state(), _weights(opt)
    r["counters2"] = (opt.steps, step.opt_steps, step.micro_steps, step.ema.updates)
    g2 = [p.grad.clone() for p in opt.params]
    r["grads_differ"] = sum(int(not torch.equal(a, b)) for a, b in zip(g1, g2))
    r["n_bf16_grads"] = sum(int(g.dtype == torch.bfloat16) for g in g1)
    twin_sum.step([a.float() + b.float() for a, b in zip(g1, g2)], inv_world=0.5)
    twin_g2.step(g2, inv_world=1.0)
    torch.cuda.synchronize()
    r["twin_sum"] = {k: getattr(twin_sum, k).clone() for k in ("master", "exp_avg", "exp_avg_sq", "tsteps")}
    r["twin_g2"] = twin_g2.master.clone()
    r["rne"] = all(torch.equal(w, opt.master_of(p).to(torch.bfloat16))
                   for w, p in zip(r["weights2"], [p for p in opt.params if p.dtype == torch.bfloat16]))
    r["norms"] = (float(opt.grad_norm()), float(twin_sum.grad_norm()))
    return r


@pytest.mark.gpu
def test_first_call_of_a_cycle_leaves_the_weights(hip_lib):
    r = _two_calls()
    assert r["has_acc"]
    for k, v in r["state0"].items():
        assert torch.equal(v, r["state1"][k]), k
    assert all(torch.equal(a, b) for a, b in zip(r["weights0"], r["weights1"]))
    assert r["counters1"] == (0, 0, 1, 0)  # no optimizer step, no EMA update
    assert torch.isfinite(r["loss1"])


@pytest.mark.gpu
def test_second_call_steps_on_the_sum(hip_lib):
    r = _two_calls()
    assert r["counters2"] == (1, 1, 2, 1)  # one optimizer step, the weight average advanced once
    assert r["n_bf16_grads"] > 0 and r["grads_differ"] > 0  # two different batches, bf16 static gradients
    assert torch.isfinite(r["loss2"]) and not torch.equal(r["loss1"], r["loss2"])  # each call its own loss
    for k, v in r["twin_sum"].items():
        assert torch.equal(r["state2"][k], v), k
    assert not torch.equal(r["state2"]["master"], r["twin_g2"])   # not a step on the second batch alone
    assert not torch.equal(r["state2"]["master"], r["state0"]["master"])
    assert r["rne"]  # the bf16 weights are the RNE of the new masters
    assert r["norms"][0] == r["norms"][1] > 0.0  # the norm of the mean gradient


@pytest.mark.gpu
def test_accumulate_one_has_no_accumulator(hip_lib):
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.step import TrainStep

    dev = torch.device("cuda", 0)
    b1 = _data(dev, 11)
    for kw in ({}, {"accumulate": 1}):
        step = TrainStep(_model(dev), SetCriterion(num_classes=1), b1[0], b1[1], graphs=False, **kw)
        assert step.accumulate == 1 and step.acc is None
    with pytest.raises(ValueError):
        TrainStep(_model(dev), SetCriterion(num_classes=1), b1[0], b1[1], graphs=False, accumulate=0)


# ---------------------------------------------------------------------------
# data parallelism through the step: two ranks on one GPU over gloo, whole-step graph
# ---------------------------------------------------------------------------
def _dp_worker(rank, world, port, out, zero):
    os.environ["MOE_ZERO"] = "1" if zero else "0"  # read when step.py is imported (below)
    for p in (str(ROOT / "multimodal-moe_amd"), str(ROOT)):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.step import TrainStep

    dev = torch.device("cuda", 0)
    model = _model(dev)
    b1, b2 = _data(dev, 11 + rank), _data(dev, 21 + rank)  # four different images over ranks and micro-steps
    step = TrainStep(model, SetCriterion(num_classes=1), b1[0], b1[1], graphs=True, world=world, lr=1e-3,
                     targets=b1[2], num_boxes=NB, accumulate=2)
    assert (step.reducer is None) == zero and (type(step.opt).__name__ == "ShardedDPAdamW") == zero
    weights = lambda: torch.cat([p.detach().float().reshape(-1) for p in model.parameters()]).cpu()  # noqa: E731
    w0 = weights()
    step(*b1)
    torch.cuda.synchronize()
    res = {"still": bool(torch.equal(weights(), w0)), "steps1": (step.opt.steps, step.opt_steps)}
    step(*b2)
    torch.cuda.synchronize()
    res.update(w=weights(), moved=not torch.equal(weights(), w0), steps2=(step.opt.steps, step.opt_steps),
               coef=step.opt.coef.cpu().clone())
    torch.save(res, out / f"dp{rank}.pt")
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("zero", [True, False])
def test_data_parallel_step_exchanges_once_per_cycle(hip_lib, tmp_path, zero):
    """zero: optim.ShardedDPAdamW (the default at world > 1); else the flat
    all-reduce of the accumulated fp32 sums + FlatAdamW (MOE_ZERO=0).  The
    first call of a cycle runs no collective and moves nothing; after the
    second both ranks hold the same weights bit for bit, and the norm of the
    mean gradient (over 2 micro-steps x 2 ranks) is the same on both."""
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.step import TrainStep

    ctx = mp.start_processes(_dp_worker, args=(2, _port(), tmp_path, zero), nprocs=2, join=False,
                             start_method="spawn")
    deadline = time.monotonic() + 240
    while not ctx.join(timeout=2):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the data-parallel accumulation workers did not finish in time")
    r0, r1 = torch.load(tmp_path / "dp0.pt"), torch.load(tmp_path / "dp1.pt")
    for r in (r0, r1):
        assert r["still"] and r["steps1"] == (0, 0) and r["moved"] and r["steps2"] == (1, 1)
    assert torch.equal(r0["w"], r1["w"]), "ranks diverged"
    assert torch.equal(r0["coef"], r1["coef"])
    # one process accumulating the same four images: the same mean gradient up to the order of
    # three fp32 additions per element, and a norm summed in another order (per rank slice under
    # the sharded optimizer): 1e-4 relative, the project's figure for the norm against a
    # differently ordered sum (tests/test_gpu_optim.py)
    dev = torch.device("cuda", 0)
    batches = [_data(dev, s) for s in (11, 12, 21, 22)]
    step = TrainStep(_model(dev), SetCriterion(num_classes=1), batches[0][0], batches[0][1], graphs=True, lr=1e-3,
                     targets=batches[0][2], num_boxes=NB, accumulate=4)
    for b in batches:
        step(*b)
    torch.cuda.synchronize()
    assert step.opt_steps == 1
    want = float(step.opt.grad_norm())
    print(f"norm of the mean gradient: two ranks {float(r0['coef'][0])!r}, one process {want!r}")
    assert abs(float(r0["coef"][0]) - want) <= 1e-4 * want, (float(r0["coef"][0]), want)


# ---------------------------------------------------------------------------
# the sharded optimizer: two ranks on one GPU over gloo, no graph capture
# ---------------------------------------------------------------------------
def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


MICRO = 2


def _sharded_worker(rank, world, port, out):
    for p in (str(ROOT / "multimodal-moe_amd"), str(ROOT), str(ROOT / "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    from test_gpu_grad_accum import _grads, _params

    from src.rtdetr_moe.optim import GradAccumulator, ShardedDPAdamW

    ps = _params(0)
    grads = _grads(ps)[:MICRO]  # identical on both ranks
    opt = ShardedDPAdamW([(ps[:3], 1e-3), (ps[3:], 3e-4)], weight_decay=1e-2, clip_norm=0.05)
    acc = GradAccumulator(opt.params)
    for row in grads:
        acc.add(row)
    taken, count = acc.take()
    opt.step(taken, inv_world=1.0 / (world * count))
    torch.cuda.synchronize()
    res = {"count": count, "masters": [opt.master_of(p).cpu() for p in ps], "norm": float(opt.grad_norm()),
           "straddle": len({r for (_, _, _, r, _) in opt.pieces}) == world and len(opt.pieces) > len(ps) - 1}
    torch.save(res, out / f"acc{rank}.pt")
    dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_optimizer_on_accumulated_gradients(hip_lib, tmp_path):
    from test_gpu_grad_accum import NEVER, _grads, _params, _torch_sums

    from src.rtdetr_moe.optim import FlatAdamW

    ctx = mp.start_processes(_sharded_worker, args=(2, _port(), tmp_path), nprocs=2, join=False,
                             start_method="spawn")
    deadline = time.monotonic() + 240
    while not ctx.join(timeout=2):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the sharded accumulation workers did not finish in time")
    r0, r1 = torch.load(tmp_path / "acc0.pt"), torch.load(tmp_path / "acc1.pt")
    assert r0["count"] == r1["count"] == MICRO and r0["straddle"]
    assert all(torch.equal(a, b) for a, b in zip(r0["masters"], r1["masters"]))
    # single process: the same mean gradient (every rank held the same gradients)
    ps = _params(0)
    start = [p.detach().float().cpu().reshape(-1) for p in ps]
    sums = _torch_sums(ps, _grads(ps)[:MICRO])
    opt = FlatAdamW([(ps[:3], 1e-3), (ps[3:], 3e-4)], weight_decay=1e-2, clip_norm=0.05)
    opt.step(sums, inv_world=1.0 / MICRO)
    torch.cuda.synchronize()
    for i, (p, got) in enumerate(zip(ps, r0["masters"])):
        torch.testing.assert_close(got, opt.master_of(p).cpu(), rtol=2e-5, atol=1e-7)
        if i != NEVER and p.dim() == 1:
            assert not torch.equal(got, start[i]), i  # it moved
    assert abs(r0["norm"] - float(opt.grad_norm())) <= 1e-4 * float(opt.grad_norm())
