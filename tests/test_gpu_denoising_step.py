"""Training with contrastive denoising queries on the GPU: the fused
evaluation of SetCriterion.dn_losses (rtdetr_set_criterion_loss with a
constant assignment) against its torch formulation, and TrainStep eager vs
the whole-step hipGraph for a -dn100 model (tests/test_gpu_step.py's setup:
R18, 4 experts top-2, batch 2, 256x320)."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPEC = "rtdetr-r18-moe4-top2-dn100"


def _setup(spec=SPEC, seed=6):  # seed 6: 6 + 0 boxes (real targets and an empty image)
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.data import SyntheticZOD
    from src.rtdetr_moe.model import RTDETRMoE

    torch.manual_seed(0)
    model = RTDETRMoE(spec).to(DEV).to(memory_format=torch.channels_last)
    images, targets, ctx = SyntheticZOD(batch=2, img_h=256, img_w=320, seed=seed).sample(DEV)
    images = images.contiguous(memory_format=torch.channels_last)
    targets = [{k: v.to(DEV) for k, v in t.items()} for t in targets]
    return model, SetCriterion(num_classes=1), images, targets, ctx


@pytest.mark.parametrize("C", [1, 3])
def test_dn_losses_fused_matches_torch(hip_lib, C):
    """fp32 on both sides: every component within 1e-4 relative, and the same
    gradients w.r.t. the denoising logits and boxes."""
    from src.rtdetr_moe.criterion import SetCriterion, pad_targets
    from src.rtdetr_moe.denoising import dn_shapes

    g = torch.Generator(device=DEV).manual_seed(21 + C)
    S, B, M = 3, 2, 16
    G, Qdn = dn_shapes(M, 100)
    outs = [{"pred_logits": torch.randn(B, Qdn, C, device=DEV, generator=g).requires_grad_(True),
             "pred_boxes": (torch.rand(B, Qdn, 4, device=DEV, generator=g) * 0.5 + 0.2).requires_grad_(True)}
            for _ in range(S)]
    leaves = [t for o in outs for t in (o["pred_logits"], o["pred_boxes"])]
    counts = [5, 16]
    targets = [{"boxes": torch.rand(n, 4, device=DEV, generator=g) * 0.4 + 0.3,
                "labels": torch.randint(0, C, (n,), device=DEV, generator=g)} for n in counts]
    tb, tl, nv = pad_targets(targets, M)
    nb = torch.tensor(float(sum(counts)), device=DEV)
    crit = SetCriterion(num_classes=C)
    assert crit.dn_fused_ok(outs, M)
    ref = crit.dn_losses(outs, tb, tl, nv, nb, G, fused=False)
    got = crit.dn_losses(outs, tb, tl, nv, nb, G, fused=True)
    assert set(ref) == set(got) and len(got) == 3 * S
    for k in ref:
        print(k, float(got[k].detach()), float(ref[k].detach()))
        torch.testing.assert_close(got[k], ref[k], rtol=1e-4, atol=0, msg=k)
    ref_grads = torch.autograd.grad(sum(ref.values()), leaves)
    got_grads = torch.autograd.grad(sum(got.values()), leaves)
    for i, (a, b) in enumerate(zip(got_grads, ref_grads)):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6, msg=f"grad of leaf {i}")


def test_denoising_train_step_graph_matches_eager(hip_lib):
    from src.rtdetr_moe.step import TrainStep

    runs, comps = {}, {}
    for graphs in (False, True):
        model, crit, images, targets, ctx = _setup()
        assert sum(len(t["boxes"]) for t in targets) > 0
        nb = max(1.0, float(sum(len(t["boxes"]) for t in targets)))
        step = TrainStep(model, crit, images, ctx, graphs=graphs, world=1, precision="bf16", lr=1e-3,
                         targets=targets if graphs else None, num_boxes=nb, seed=0)
        assert (step.stepper is not None) == graphs
        runs[graphs] = [float(step(images, ctx, targets, nb)) for _ in range(3)]
        comps[graphs] = set(step.last_losses)
        if graphs:
            assert step.stepper.captures == 1  # three steps, one capture: the graph is replayed
            assert int(step.stepper.status.item()) == 0
    torch.cuda.synchronize()
    eager, graph = runs[False], runs[True]
    print("eager", eager, "graph", graph)
    dn_names = {k + s for k in ("loss_vfl", "loss_bbox", "loss_giou") for s in ("_dn", "_dn_aux0", "_dn_aux1")}
    for losses, names in ((eager, comps[False]), (graph, comps[True])):
        assert all(torch.isfinite(torch.tensor(losses))), losses
        assert min(losses[1:]) < losses[0], losses  # same batch: the loss must go down
        assert dn_names <= names, names
    for a, b in zip(eager, graph):
        assert abs(a - b) <= 2e-2 * max(1.0, abs(a)), (eager, graph)


def test_no_dn_components_without_the_token(hip_lib):
    from src.rtdetr_moe.step import TrainStep

    model, crit, images, targets, ctx = _setup("rtdetr-r18-moe4-top2")
    assert not any("denoising" in k for k in model.state_dict())
    nb = max(1.0, float(sum(len(t["boxes"]) for t in targets)))
    step = TrainStep(model, crit, images, ctx, graphs=True, world=1, precision="bf16", lr=1e-3,
                     targets=targets, num_boxes=nb)
    step(images, ctx, targets, nb)
    torch.cuda.synchronize()
    assert step.stepper.dn_pack is None
    assert step.last_losses and not any("_dn" in k for k in step.last_losses)


def test_recapture_at_larger_capacity_resizes_the_groups(hip_lib):
    """A batch with more boxes than the captured padding re-captures at M = 32:
    G = 100 // 32 = 3 groups of 2 x 32 queries, new static buffers, a finite
    loss that still reports the denoising components."""
    from src.rtdetr_moe.step import TrainStep

    model, crit, images, targets, ctx = _setup()
    nb = max(1.0, float(sum(len(t["boxes"]) for t in targets)))
    step = TrainStep(model, crit, images, ctx, graphs=True, world=1, precision="bf16", lr=1e-3,
                     targets=targets, num_boxes=nb)
    step(images, ctx, targets, nb)
    assert step.stepper.M == 16 and step.stepper.dn_pack[2] == 6 and step.stepper.dn_pack[0].shape == (2, 192)
    g = torch.Generator(device=DEV).manual_seed(9)
    big = [{"boxes": torch.rand(n, 4, device=DEV, generator=g) * 0.2 + 0.3,
            "labels": torch.zeros(n, dtype=torch.int64, device=DEV)} for n in (20, 2)]
    loss = float(step(images, ctx, big, 22.0))
    torch.cuda.synchronize()
    assert step.stepper.captures == 2 and step.stepper.M == 32
    assert step.stepper.dn_pack[2] == 3 and step.stepper.dn_pack[0].shape == (2, 192)
    assert step.stepper.dn_pack[1].shape == (2, 192, 4)
    assert torch.isfinite(torch.tensor(loss))
    assert any(k.endswith("_dn") for k in step.last_losses)
    labels = step.stepper.dn_pack[0].view(2, 3, 2, 32)
    assert (labels[0, :, :, :20] == 0).all() and (labels[0, :, :, 20:] == 1).all() and (labels[1, :, :, 2:] == 1).all()
