"""Loss-free load balancing through the training step on the GPU
(step.TrainStep on an -alb spec, the whole step as one hipGraph): the
selection biases move once per optimizer step, by src/moe/balance.py's rule on
the layers' expert histograms, outside the graph; the graph's router launches
read them by address.  Model, data and construction follow
tests/test_gpu_accumulate_step.py."""
from __future__ import annotations

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SPEC = "rtdetr-r18-moe4-top2-dec2"
RATE = 0.25
NB = 2.0


def _data(dev, seed):
    from src.rtdetr_moe.data import SyntheticZOD

    images, targets, ctx = SyntheticZOD(batch=1, img_h=256, img_w=256, seed=seed).sample(dev)
    images = images.contiguous(memory_format=torch.channels_last)
    return images, ctx, [{k: v.to(dev) for k, v in t.items()} for t in targets], NB


def _model(dev, spec):
    from src.rtdetr_moe.model import RTDETRMoE

    torch.manual_seed(0)
    return RTDETRMoE(spec).to(dev).to(memory_format=torch.channels_last)


def _step(spec, **kw):
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.step import TrainStep

    dev = torch.device("cuda", 0)
    b1 = _data(dev, 11)
    model = _model(dev, spec)
    step = TrainStep(model, SetCriterion(num_classes=1), b1[0], b1[1], graphs=True, lr=1e-3, targets=b1[2],
                     num_boxes=NB, **kw)
    assert step.stepper is not None
    return model, step


def _biases(step):
    torch.cuda.synchronize()
    return torch.stack([m.sel_bias.detach().clone() for m in step.balancer.layers]).cpu()


def _hists(step):
    torch.cuda.synchronize()
    return torch.stack([m.last_hist.detach().clone() for m in step.balancer.layers]).cpu().long()


@functools.lru_cache(maxsize=None)
def _three_steps():
    from src.moe.balance import balance_reference

    dev = torch.device("cuda", 0)
    model, step = _step(f"{SPEC}-alb{RATE}")
    r = {"L": step.balancer.L, "bias0": _biases(step), "load0": step.balancer.load.cpu().clone(), "got": [],
         "want": [], "hist": [], "maxvio": []}
    want = r["bias0"].clone()
    for seed in (11, 12, 13):
        step(*_data(dev, seed))
        h = _hists(step)
        mv = balance_reference(h.clone(), want, RATE)
        r["got"].append(_biases(step))
        r["want"].append(want.clone())
        r["hist"].append(h)
        r["maxvio"].append((step.balancer.maxvio.cpu().clone(), mv))
    r["counters"] = (step.micro_steps, step.opt_steps)
    # a no_grad evaluation forward uses the biases and moves nothing
    model.eval()
    b = _data(dev, 14)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
        model(b[0], b[1])
    model.train()
    r["bias_eval"], r["load_eval"] = _biases(step), step.balancer.load.cpu().clone()
    # 1000 into one layer's bias of expert 0, in place: the next replay must read it (by address)
    layer = step.balancer.layers[1]
    with torch.no_grad():
        layer.sel_bias[0] = 1000.0
    step(*_data(dev, 15))
    torch.cuda.synchronize()
    r["poked_hist"] = layer.last_hist.cpu().clone()
    r["poked_tokens"] = layer.last_tokens
    r["keys"] = [k for k in model.state_dict() if k.endswith("sel_bias")]
    return r


def test_capture_leaves_the_biases_alone(hip_lib):
    r = _three_steps()
    assert r["L"] == 3  # AIFI + two decoder layers
    assert float(r["bias0"].abs().sum()) == 0.0 and int(r["load0"].abs().sum()) == 0
    assert len(r["keys"]) == 3


def test_each_step_applies_the_reference_rule(hip_lib):
    r = _three_steps()
    assert r["counters"] == (3, 3)
    for i in range(3):
        assert torch.equal(r["got"][i], r["want"][i]), f"step {i}"
        assert torch.equal(*r["maxvio"][i]), f"step {i}"
        assert int(r["hist"][i].sum()) > 0
    assert not torch.equal(r["got"][0], r["bias0"]) and not torch.equal(r["got"][1], r["got"][0])


def test_evaluation_moves_nothing(hip_lib):
    r = _three_steps()
    assert torch.equal(r["bias_eval"], r["got"][2]) and int(r["load_eval"].abs().sum()) == 0


def test_replay_reads_the_bias_by_address(hip_lib):
    r = _three_steps()
    assert int(r["poked_hist"][0]) == r["poked_tokens"] > 0  # every token took expert 0


def test_accumulation_applies_once_per_cycle(hip_lib):
    from src.moe.balance import balance_reference

    dev = torch.device("cuda", 0)
    model, step = _step(f"{SPEC}-alb{RATE}", accumulate=2)
    b0 = _biases(step)
    step(*_data(dev, 11))
    h1, b1 = _hists(step), _biases(step)
    assert torch.equal(b1, b0) and torch.equal(step.balancer.load.cpu(), h1) and step.opt_steps == 0
    step(*_data(dev, 12))
    h2, b2 = _hists(step), _biases(step)
    want = b0.clone()
    balance_reference(h1 + h2, want, RATE)
    assert step.opt_steps == 1 and torch.equal(b2, want) and not torch.equal(b2, b0)
    assert not torch.equal(h1, h2) and int(step.balancer.load.abs().sum()) == 0


def test_off_without_the_token(hip_lib):
    model, step = _step(SPEC)
    assert step.balancer is None
    assert not any("sel_bias" in k for k in model.state_dict())
