"""The weight average through the training step on the GPU (ema.ModelEMA
inside step.TrainStep, the whole step as one hipGraph) and under the sharded
optimizer (optim.ShardedDPAdamW, two ranks sharing one GPU over gloo, as
tests/test_gpu_dist_graphs.py rehearses them).  The reference's Ultralytics
trainer validates and checkpoints the averaged model
(src/models/vision/rtdetr.py:82-94 trains through it).

Reference and tolerance: tests/test_gpu_ema.py (the fp64 recurrence over the
optimizer's own masters / the live buffers; n 2^-22 A after n updates)."""
from __future__ import annotations

import functools
import math
import os
import socket
import sys
import time
from datetime import timedelta
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parents[1]
SPEC = "rtdetr-r18-moe4-top2-dec2"
NB = 2.0
DECAY, TAU = 0.5, 1.0


def _decay32(t, decay=DECAY, tau=TAU):
    d32 = np.float32(decay * (1.0 - math.exp(-t / tau)))
    return float(d32), float(np.float32(1.0) - d32)


def _data(dev):
    from src.rtdetr_moe.data import SyntheticZOD

    images, targets, ctx = SyntheticZOD(batch=1, img_h=256, img_w=256, seed=11).sample(dev)
    images = images.contiguous(memory_format=torch.channels_last)
    return images, [{k: v.to(dev) for k, v in t.items()} for t in targets], ctx


def _model(dev):
    from src.rtdetr_moe.model import RTDETRMoE

    torch.manual_seed(0)
    return RTDETRMoE(SPEC).to(dev).to(memory_format=torch.channels_last)


def _train_step(dev):
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.step import TrainStep

    model = _model(dev)
    images, targets, ctx = _data(dev)
    step = TrainStep(model, SetCriterion(num_classes=1), images, ctx, graphs=True, lr=1e-3, targets=targets,
                     num_boxes=NB, ema_decay=DECAY, ema_tau=TAU)
    assert step.stepper is not None and step.ema is not None and type(step.opt).__name__ == "FlatAdamW"
    return model, step, (images, ctx, targets, NB)


def _flat(t):
    from src.rtdetr_moe.optim import _storage_flat

    return _storage_flat(t.detach())


def _live(model, step):
    """{state-dict name: fp32 value, storage order} of every floating-point
    entry: the optimizer's master for its parameters, the live tensor else."""
    owned = {id(p) for p in step.opt.params}
    out = {}
    for k, v in model.state_dict(keep_vars=True).items():
        if v.is_floating_point():
            out[k] = (step.opt.master_of(v) if id(v) in owned else _flat(v).float()).clone()
    return out


@functools.lru_cache(maxsize=None)
def _three_steps():
    """Three whole-step-graph steps with the average on: the values averaged
    after each step, the average at the start and at the end, the losses."""
    dev = torch.device("cuda", 0)
    model, step, batch = _train_step(dev)
    start = {k: _flat(v).clone() for k, v in step.ema.state_dict().items()}
    lives, losses = [], []
    for _ in range(3):
        losses.append(step(*batch).clone())
        torch.cuda.synchronize()
        lives.append(_live(model, step))
    end = {k: _flat(v).clone() for k, v in step.ema.state_dict().items()}
    keys = list(model.state_dict())
    n_params = len(step.opt.params)
    return start, lives, end, losses, keys, n_params


@pytest.mark.gpu
def test_whole_step_graph_with_ema(hip_lib):
    start, lives, end, losses, keys, n_params = _three_steps()
    assert list(end) == keys and all(torch.isfinite(x) for x in losses)
    n_float = n_bufs = 0
    for k, live0 in lives[0].items():
        ref = start[k].double()
        A = float(ref.abs().max())
        for t, live in enumerate(lives, 1):
            d, omd = _decay32(t)
            ref = d * ref + omd * live[k].double()
            A = max(A, float(live[k].abs().max()), float(ref.abs().max()))
        assert end[k].dtype == torch.float32
        A = max(A, float(end[k].abs().max()))
        err = float((end[k].double() - ref).abs().max())
        assert err <= 3 * 2.0 ** -22 * A, (k, err, A)
        n_float += 1
        if "running_" in k and not torch.equal(lives[2][k], lives[0][k]):
            n_bufs += 1
            assert not torch.equal(end[k], lives[2][k]), k  # lags the live statistics
    assert n_float > n_params and n_bufs > 0  # the BatchNorm running statistics are averaged too
    moved = sum(int(not torch.equal(end[k], lives[2][k])) for k in lives[0])
    assert moved >= n_params // 2


def _eval_out(model, images, ctx):
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
        out = model(images, ctx)
    res = (out["pred_logits"].float().clone(), out["pred_boxes"].float().clone())
    model.train()
    return res


@pytest.mark.gpu
def test_applied_validates_the_average_and_restores_training(hip_lib):
    from src.rtdetr_moe.step import gemm_params

    _, _, _, twin_losses, _, _ = _three_steps()  # the twin run: never enters applied()
    dev = torch.device("cuda", 0)
    model, step, batch = _train_step(dev)
    images, ctx = batch[0], batch[1]
    losses = [step(*batch).clone() for _ in range(2)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(losses, twin_losses))

    def snapshot():
        snap = {"sd." + k: v.detach().clone() for k, v in model.state_dict(keep_vars=True).items()}
        for k in ("master", "exp_avg", "exp_avg_sq", "tsteps", "ema"):
            snap["opt." + k] = getattr(step.opt, k).clone()
        snap["rest_ema"] = step.ema.rest_ema.clone()
        return snap

    before = snapshot()
    ptrs = [p.data_ptr() for p in model.parameters()]
    raw = _eval_out(model, images, ctx)
    avg_sd = step.ema.state_dict()
    with step.ema.applied():
        assert [p.data_ptr() for p in model.parameters()] == ptrs  # written in place: captured graphs stay valid
        got = _eval_out(model, images, ctx)
    after = snapshot()
    for k, v in before.items():
        assert torch.equal(v, after[k]), k

    # a fresh model loaded from the averaged state dict, in the step's precision (bf16 GEMM / conv operands)
    fresh = _model(dev)
    fresh.load_state_dict(avg_sd)
    for p in gemm_params(fresh):
        p.data = p.data.to(torch.bfloat16)
    # the encoder caches its position embedding on first use, and its bf16 rounding depends on
    # whether that first use ran under autocast (here) or not (the training step): both models
    # read the trained model's, as a validation after training does
    fresh.encoder._pos_cache = dict(model.encoder._pos_cache)
    want, again = _eval_out(fresh, images, ctx), _eval_out(fresh, images, ctx)
    for g, w, a, r in zip(got, want, again, raw):
        spread = float((w - a).abs().max())
        if spread == 0.0:
            assert torch.equal(g, w)
        else:
            assert float((g - w).abs().max()) <= spread
        assert not torch.equal(g, r)  # the averaged model is not the raw one

    loss3 = step(*batch).clone()
    torch.cuda.synchronize()
    assert torch.equal(loss3, twin_losses[2])


# ---------------------------------------------------------------------------
# the sharded optimizer: two ranks on one GPU over gloo
# ---------------------------------------------------------------------------
def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


NO_GRAD = 4  # this tensor never has a gradient (the sharded optimizer wants a fixed pattern): still averaged


def _sharded_worker(rank, world, port, out):
    for p in (str(ROOT / "multimodal-moe_amd"), str(ROOT)):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    from test_gpu_ema import DECAY as D, STEPS, TAU as T, make_grads, make_params

    from src.rtdetr_moe.ema import ema_decay_at
    from src.rtdetr_moe.optim import ShardedDPAdamW, _storage_flat

    ps = make_params(0)
    opt = ShardedDPAdamW([(ps[:3], 1e-3), (ps[3:], 3e-4)], weight_decay=1e-2, clip_norm=0.0)
    opt.enable_ema()
    g = torch.Generator().manual_seed(1)
    res = {"start": [opt.master_of(p).cpu() for p in ps], "masters": [], "emas": []}
    for step in range(STEPS):
        grads = make_grads(ps, -1, g)  # identical on both ranks
        grads[NO_GRAD] = None
        opt.step(grads, ema_decay=ema_decay_at(step + 1, D, T))
        torch.cuda.synchronize()
        res["masters"].append([opt.master_of(p).cpu() for p in ps])
        res["emas"].append([opt.ema_of(p).cpu() for p in ps])
    # the rank's state, average included, survives a state_dict round trip
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    weights = [_storage_flat(p.detach()).clone() for p in ps]
    opt.ema.zero_()
    opt.master.add_(1.0)
    opt.load_state_dict(sd)
    res["roundtrip"] = bool(torch.equal(opt.ema, sd["ema"]) and torch.equal(opt.master, sd["master"]) and all(
        torch.equal(_storage_flat(p.detach()), w) for p, w in zip(ps, weights)))
    res["straddle"] = len({r for (_, _, _, r, _) in opt.pieces}) == world and len(opt.pieces) > len(ps)
    torch.save(res, out / f"ema{rank}.pt")
    dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_optimizer_ema(hip_lib, tmp_path):
    from test_gpu_ema import STEPS, reference_track

    ctx = mp.start_processes(_sharded_worker, args=(2, _port(), tmp_path), nprocs=2, join=False,
                             start_method="spawn")
    deadline = time.monotonic() + 240
    while not ctx.join(timeout=2):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the sharded EMA workers did not finish in time")
    r0, r1 = torch.load(tmp_path / "ema0.pt"), torch.load(tmp_path / "ema1.pt")
    assert r0["straddle"] and r0["roundtrip"] and r1["roundtrip"]  # tensors cut at the slice boundary
    for r in (r0, r1):
        refs, A = reference_track(r["masters"], r["start"])
        for n, (ref, got) in enumerate(zip(refs, r["emas"]), 1):
            for i, (a, b) in enumerate(zip(ref, got)):
                bound = n * 2.0 ** -22 * max(A[i], float(b.abs().max()))
                assert float((b.double() - a).abs().max()) <= bound, (n, i)
        assert torch.equal(r["masters"][-1][NO_GRAD], r["start"][NO_GRAD])
    for n in range(STEPS):
        assert all(torch.equal(a, b) for a, b in zip(r0["emas"][n], r1["emas"][n]))
    assert not torch.equal(r0["emas"][-1][0], r0["masters"][-1][0])
