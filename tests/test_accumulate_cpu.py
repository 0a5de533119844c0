"""Gradient accumulation and the learning-rate schedule on the CPU route
(step.TrainStep with torch.optim.AdamW; engine.train).  The reference trains
through Ultralytics' trainer (src/models/vision/rtdetr.py:82-94), which
accumulates nbs / batch batches per optimizer step and decays the rate.

Reference: a twin model on which the two backward passes are accumulated by
hand, divided by 2, clipped (clip_grad_norm_) and stepped with
torch.optim.AdamW.  Tolerance rtol 2e-5 / atol 1e-7: the project's figure for
fp32 weights against torch with a different operation order
(tests/test_gpu_optim.py)."""
from __future__ import annotations

import copy
import csv
import functools

import torch

SPEC = "rtdetr-r18-moe4-top2-dec2"
LR, LR_BB, WD, CLIP, NB = 1e-3, 1e-4, 1e-4, 0.1, 2.0


def _batches():
    from src.rtdetr_moe.data import SyntheticZOD

    return [SyntheticZOD(batch=1, img_h=128, img_w=128, seed=s).sample() for s in (3, 4)]


def _twin_step(model, batches):
    """One optimizer step of ``model`` on the mean gradient of ``batches``, by hand."""
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.step import FlatOutputs

    crit = SetCriterion(num_classes=1)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    bb = [p for n, p in named if n.startswith("backbone.")]
    rest = [p for n, p in named if not n.startswith("backbone.")]
    opt = torch.optim.AdamW([{"params": bb, "lr": LR_BB}, {"params": rest, "lr": LR}], lr=LR, weight_decay=WD)
    flat = FlatOutputs(model)
    for images, targets, ctx in batches:
        out, aux = FlatOutputs.unflatten(flat(images, ctx))
        (sum(crit(out, targets, NB).values()) + aux).backward()  # autograd sums into .grad
    params = [p for _, p in named if p.grad is not None]
    for p in params:
        p.grad.div_(len(batches))
    torch.nn.utils.clip_grad_norm_(params, CLIP)
    opt.step()


@functools.lru_cache(maxsize=None)
def _scenario():
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.step import TrainStep

    torch.manual_seed(0)
    model = RTDETRMoE(SPEC)
    twins = {k: copy.deepcopy(model) for k in ("both", "first", "second")}
    b1, b2 = _batches()
    step = TrainStep(model, SetCriterion(num_classes=1), b1[0], b1[2], graphs=False, lr=LR, lr_backbone=LR_BB,
                     weight_decay=WD, clip_norm=CLIP, accumulate=2)
    before = [p.detach().clone() for p in model.parameters()]
    loss1 = step(b1[0], b1[2], b1[1], NB)
    after1 = [p.detach().clone() for p in model.parameters()]
    counters1 = (step.micro_steps, step.opt_steps)
    loss2 = step(b2[0], b2[2], b2[1], NB)
    after2 = [p.detach().clone() for p in model.parameters()]
    counters2 = (step.micro_steps, step.opt_steps)
    _twin_step(twins["both"], [b1, b2])
    _twin_step(twins["first"], [b1])
    _twin_step(twins["second"], [b2])
    ref = {k: [p.detach().clone() for p in m.parameters()] for k, m in twins.items()}
    return dict(before=before, after1=after1, after2=after2, ref=ref, counters=(counters1, counters2),
                losses=(loss1, loss2), acc=step.acc)


def test_no_update_inside_a_cycle():
    s = _scenario()
    assert all(torch.equal(a, b) for a, b in zip(s["before"], s["after1"]))
    assert s["counters"][0] == (1, 0)
    assert all(torch.isfinite(x) for x in s["losses"]) and not torch.equal(*s["losses"])  # each call its own loss


def test_update_on_the_mean_gradient():
    s = _scenario()
    assert s["counters"][1] == (2, 1)
    assert s["acc"] is None  # the CPU route accumulates in .grad
    moved = 0
    for got, want, old in zip(s["after2"], s["ref"]["both"], s["before"]):
        torch.testing.assert_close(got, want, rtol=2e-5, atol=1e-7)
        moved += int(not torch.equal(got, old))
    assert moved >= len(s["before"]) // 2


def test_differs_from_a_step_on_either_batch_alone():
    s = _scenario()
    for k in ("first", "second"):
        differ = sum(int(not torch.allclose(got, want, rtol=2e-5, atol=1e-7))
                     for got, want in zip(s["after2"], s["ref"][k]))
        assert differ >= len(s["before"]) // 2, k


def test_set_lr_scale_and_default():
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.model import RTDETRMoE
    from src.rtdetr_moe.step import TrainStep

    torch.manual_seed(0)
    b1 = _batches()[0]
    step = TrainStep(RTDETRMoE(SPEC), SetCriterion(num_classes=1), b1[0], b1[2], graphs=False, lr=LR,
                     lr_backbone=LR_BB)
    assert step.accumulate == 1 and step.lrs() == [LR_BB, LR]
    step.set_lr_scale([0.5, 0.25])
    assert [g["lr"] for g in step.opt.param_groups] == [LR_BB * 0.5, LR * 0.25]
    step.set_lr_scale([1.0, 1.0])  # factors apply to the construction's rates, not to the current ones
    assert step.lrs() == [LR_BB, LR]
    # the spec's nominal batch size sets the count: round(nbs / (batch world))
    step = TrainStep(RTDETRMoE(SPEC + "-nbs3"), SetCriterion(num_classes=1), b1[0], b1[2], graphs=False)
    assert step.accumulate == 3


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def test_engine_schedule_and_columns(tmp_path):
    from src.rtdetr_moe.engine import TrainArgs, train
    from src.rtdetr_moe.schedule import lr_factor

    def run(spec, name):
        res = train(TrainArgs(model=spec, data="synthetic:4", imgsz=128, epochs=2, batch=1, device="cpu",
                              project=str(tmp_path), name=name, workers=0, lr=LR, lr_backbone=LR_BB))
        return _rows(res.save_dir / "results.csv")

    new = ("lr/pg0", "lr/pg1", "train/accumulate", "train/opt_steps")
    rows = run(SPEC + "-nbs2-lrf0.1", "sched")
    assert len(rows) == 2 and all(k in rows[0] for k in new)
    assert [int(r["train/opt_steps"]) for r in rows] == [2, 4]
    assert [int(r["train/accumulate"]) for r in rows] == [2, 2]
    for epoch, r in enumerate(rows):
        assert float(r["lr/pg1"]) == LR * lr_factor(epoch, 2, 0.1)
        assert float(r["lr/pg0"]) == LR_BB * lr_factor(epoch, 2, 0.1)
    assert float(rows[1]["lr/pg1"]) < float(rows[0]["lr/pg1"])
    plain = run(SPEC, "plain")
    assert len(plain) == 2 and not any(k in plain[0] for k in new)
    assert [k for k in rows[0] if k not in new] == list(plain[0])  # the other columns are unchanged
