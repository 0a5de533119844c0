"""Exponential moving average of the weights, CPU side (src/rtdetr_moe/ema.py;
the reference's Ultralytics trainer keeps a ModelEMA, validates it and writes
it into best.pt / last.pt): the spec tokens, the decay schedule, the torch
blend of a CPU TrainStep, and the checkpoints of an engine run."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

SPEC = "rtdetr-r18-moe4-top1-dec1"


def test_spec_tokens():
    from src.moe.config import parse_moe_spec

    s = parse_moe_spec("rtdetr-r18-moe4-top1")
    assert s.ema_decay == 0.0 and s.ema_tau == 2000.0
    s = parse_moe_spec("rtdetr-r18-moe4-top1-ema")
    assert s.ema_decay == 0.9999 and s.ema_tau == 2000.0
    s = parse_moe_spec("rtdetr-r50-ema0.999-ematau50")
    assert s.ema_decay == 0.999 and s.ema_tau == 50.0 and s.moe is None
    s = parse_moe_spec("rtdetr-r18-moe4-top2-ep2-ematau50-dn100")  # ematau alone: no average, ep still parsed
    assert s.ema_decay == 0.0 and s.ema_tau == 50.0 and s.moe.ep_size == 2 and s.num_denoising == 100
    for bad in ("rtdetr-r18-ema1", "rtdetr-r18-ema1.5", "rtdetr-r18-ematau0"):
        with pytest.raises(ValueError):
            parse_moe_spec(bad)


def test_decay_schedule():
    from src.rtdetr_moe.ema import ModelEMA, ema_decay_at

    ema = ModelEMA(torch.nn.Linear(2, 2))
    assert (ema.decay, ema.tau) == (0.9999, 2000.0)  # Ultralytics' defaults
    for t in (1, 2000, 10 ** 6):
        want = 0.9999 * (1.0 - math.exp(-t / 2000.0))
        assert ema.decay_at(t) == pytest.approx(want, rel=1e-15, abs=0.0)
    assert ema.decay_at(1) == pytest.approx(4.99825e-4, rel=1e-5)  # 0.9999 (1/2000 - 1/8e6 + ...)
    assert ema.decay_at(10 ** 6) == 0.9999
    assert ema_decay_at(3, 0.5, 1.0) == pytest.approx(0.5 * (1.0 - math.exp(-3.0)), rel=1e-15)
    with pytest.raises(ValueError):
        ModelEMA(torch.nn.Linear(2, 2), decay=1.0)


def _cpu_step(ema_decay, ema_tau=1.0):
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.data import SyntheticZOD
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.step import TrainStep

    torch.manual_seed(0)
    model = RTDETRMoE(SPEC)
    images, targets, ctx = SyntheticZOD(batch=1, img_h=128, img_w=128, seed=3).sample()
    step = TrainStep(model, SetCriterion(num_classes=1), images, ctx, graphs=False, lr=1e-3, ema_decay=ema_decay,
                     ema_tau=ema_tau)
    return model, step, (images, ctx, targets, 2.0)


def test_cpu_train_step_blend():
    """Two CPU steps: every floating-point entry of the state dict follows
    ema = d ema + (1 - d) value in fp32 from the initial weights; integer
    entries are the live ones.  The hand-rolled blend below is the recurrence
    in fp64 with the fp32 d and 1 - d; the torch blend rounds twice per step
    (at most 2^-23 A), so the bound is 2 steps x 2^-22 x A (tests/test_gpu_ema.py)."""
    model, step, batch = _cpu_step(0.5)
    assert step.ema is not None and step.ema.opt is None
    ref = {k: v.detach().clone().double() for k, v in model.state_dict().items() if v.is_floating_point()}
    for t in (1, 2):
        step(*batch)
        d32 = np.float32(0.5 * (1.0 - math.exp(-float(t))))
        omd = np.float32(1.0) - d32
        for k, v in model.state_dict().items():
            if v.is_floating_point():
                ref[k] = float(d32) * ref[k] + float(omd) * v.detach().double()
    assert step.ema.updates == 2
    sd, live = step.ema.state_dict(), model.state_dict()
    assert list(sd) == list(live)
    moved = 0
    for k, v in live.items():
        assert sd[k].shape == v.shape
        if not v.is_floating_point():
            assert torch.equal(sd[k], v), k
            continue
        assert sd[k].dtype == torch.float32
        A = max(float(ref[k].abs().max()), float(v.abs().max()), 1e-30)
        assert float((sd[k].double() - ref[k]).abs().max()) <= 2 * 2.0 ** -22 * A, k
        moved += int(not torch.equal(sd[k], v.float()))
    assert moved > 0  # the average lags the live weights


def test_cpu_train_step_without_ema_is_unchanged():
    _, step, batch = _cpu_step(0.0)
    assert step.ema is None
    assert torch.isfinite(step(*batch))


def test_cpu_applied_restores_the_live_model():
    model, step, batch = _cpu_step(0.5)
    step(*batch)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    avg = step.ema.state_dict()
    with step.ema.applied():
        inside = {k: v.detach().clone() for k, v in model.state_dict().items()}
    const = step.ema.constant  # frozen BatchNorm buffers: their value is their average
    assert const and all("backbone" in k for k in const)
    assert all(torch.equal(inside[k].float(), avg[k].float()) for k in avg)
    assert all(torch.equal(avg[k], before[k].float()) for k in const)
    assert any(not torch.equal(inside[k], before[k]) for k in before)
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())


def test_engine_checkpoints_carry_the_average(tmp_path):
    from src.rtdetr_moe.engine import TrainArgs, load_model, train

    def run(spec, name):
        res = train(TrainArgs(model=spec, data="synthetic:2", imgsz=128, epochs=1, batch=1, device="cpu",
                              project=str(tmp_path), name=name, workers=0, lr=1e-3))
        return res, torch.load(res.last, map_location="cpu", weights_only=True)

    res, ck = run(SPEC + "-ema0.5-ematau1", "ema")
    assert ck["ema"] == {"decay": 0.5, "tau": 1.0, "updates": 2}
    live = res.model.model.state_dict()
    assert list(ck["state_dict"]) == list(live)
    assert any(v.is_floating_point() and not torch.equal(ck["state_dict"][k], v.float()) for k, v in live.items())
    loaded = load_model(res.last)
    assert loaded.spec.ema_decay == 0.5
    for k, v in loaded.state_dict().items():
        assert torch.equal(v.float(), ck["state_dict"][k].float()), k
    assert torch.load(res.best, map_location="cpu", weights_only=True)["ema"]["updates"] == 2

    res, ck = run(SPEC, "raw")
    assert "ema" not in ck
    for k, v in res.model.model.state_dict().items():
        assert torch.equal(ck["state_dict"][k].float(), v.float()), k
