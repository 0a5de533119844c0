"""Mosaic inside the whole-step hipGraph (tests/test_gpu_augment_step.py's
setup: R18, 4 experts top-2, batch 2, 250x320 in 256x320, three graphed steps):
the kernels write the graph's static inputs, the padding M covers every step's
bound, the denoising queries follow the mosaicked counts, runs are reproducible
per seed, and a mosaic probability of 0 from the start is the plain -aug step."""
from __future__ import annotations

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPEC = "rtdetr-r18-moe4-top2"
FLOOR = 2.0 ** -22
STEPS = 3
HW, PHW = (250, 320), (256, 320)


def _setup(spec):
    from src.rtdetr_moe.criterion import SetCriterion
    from src.rtdetr_moe.data import SyntheticZOD
    from src.rtdetr_moe.model import RTDETRMoE

    torch.manual_seed(0)
    model = RTDETRMoE(spec).to(DEV).to(memory_format=torch.channels_last)
    images, targets, ctx = SyntheticZOD(batch=2, img_h=250, img_w=320, seed=6).sample(DEV)   # 250 rows padded to 256
    targets = [{k: v.to(DEV) for k, v in t.items()} for t in targets]
    # a box 1 px wide in front of image 0's targets: s <= 1.5 keeps it under 2 px, always dropped
    tiny = torch.tensor([[0.5, 0.5, 1.0 / 320, 40.0 / 256]], device=DEV)
    targets[0] = {"boxes": torch.cat([tiny, targets[0]["boxes"]]),
                  "labels": torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), targets[0]["labels"]])}
    return model, SetCriterion(num_classes=1), images, targets, ctx


@functools.lru_cache(maxsize=None)
def _run(spec=SPEC, seed=0, mosaic=1.0, tag=0):
    """Three graphed steps with augment=True and the given mosaic probability
    (None: the argument is left out); the losses, every step's bound next to
    the graph's M, and a snapshot of the static inputs after the last step
    (``tag`` only separates repeated runs)."""
    from src.rtdetr_moe.criterion import pad_targets
    from src.rtdetr_moe.step import TrainStep

    model, crit, images, targets, ctx = _setup(spec)
    counts = [len(t["boxes"]) for t in targets]
    nb = max(1.0, float(sum(counts)))
    kw = {} if mosaic is None else {"mosaic": mosaic}
    step = TrainStep(model, crit, images, ctx, graphs=True, world=1, precision="bf16", lr=1e-3, targets=targets,
                     num_boxes=nb, seed=seed, content_hw=HW, augment=True, **kw)
    st = step.stepper
    losses, bounds = [], []
    for _ in range(STEPS):
        losses.append(step(images, ctx, targets, nb).clone())
        bounds.append((step.aug.need(counts), st.M))        # this step's table is the last one uploaded
    torch.cuda.synchronize()
    m_in = step._m_in if step.aug.mosaic_path else st.M
    return dict(losses=[float(v) for v in losses], captures=st.captures, status=int(st.status.item()), M=st.M,
                bounds=bounds, counts=counts, mosaic_path=step.aug.mosaic_path, images=images,
                raw=pad_targets(targets, m_in), static_images=st.static_images.clone(), tb=st.tb.clone(),
                tl=st.tl.clone(), nv=st.nv.clone(), nb=float(st.nb), table=step.aug.table_host.clone(),
                dn_pack=None if st.dn_pack is None else (st.dn_pack[0].clone(), st.dn_pack[2]))


def test_graphed_step_inputs_are_the_mosaicked_batch(hip_lib):
    from src.rtdetr_moe import augment as A

    r = _run()
    print("losses", r["losses"], "captures", r["captures"], "M", r["M"], "bounds", r["bounds"])
    assert all(torch.isfinite(torch.tensor(r["losses"])))
    assert r["captures"] <= 2 and r["status"] == 0 and r["mosaic_path"]
    assert all(M >= need for need, M in r["bounds"]) and r["M"] == r["bounds"][-1][1]
    assert r["M"] >= max(16, (4 * max(r["counts"]) + 15) // 16 * 16)         # the first capture's starting point
    table = r["table"]
    assert table.shape == (2, A.MOSAIC_COLS) and (table[:, 19:22] >= 0).all()
    images = r["images"].cpu()
    tb, tl, nv = (t.cpu() for t in r["raw"])
    img64, b64, l64, nv64, tot64 = A.mosaic_reference(images, tb, tl, nv, table, HW, r["M"], dtype=torch.float64)
    img32, b32, _, nv32, _ = A.mosaic_reference(images, tb, tl, nv, table, HW, r["M"], dtype=torch.float32)
    # the static images are bf16: the same call with an fp32 destination is within the kernel bound of the
    # float64 reference, and the static buffer is that result rounded once
    f32 = A.mosaic_images_hip(r["images"], table.to(DEV), torch.empty_like(r["static_images"], dtype=torch.float32),
                              HW)
    assert r["static_images"].dtype == torch.bfloat16
    assert torch.equal(r["static_images"].view(torch.int16), f32.to(torch.bfloat16).view(torch.int16))
    e32 = float((img32.double() - img64).abs().max())
    err = float((f32.cpu().double() - img64).abs().max())
    print(f"images: reference fp32 error {e32:.3e}, kernel error {err:.3e}")
    assert err <= max(4 * e32, FLOOR)
    assert (r["static_images"][:, :, 250:] == 0).all()
    assert torch.equal(nv32, nv64)                                       # the draw leaves no borderline box
    assert r["tb"].shape == (2, r["M"], 4)
    assert torch.equal(r["nv"].cpu(), nv64) and torch.equal(r["tl"].cpu(), l64)
    be32 = float((b32.double() - b64).abs().max())
    berr = float((r["tb"].cpu().double() - b64).abs().max())
    print(f"boxes: kept {nv64.tolist()} of {nv.tolist()}, reference fp32 error {be32:.3e}, kernel error {berr:.3e}")
    assert berr <= max(4 * be32, FLOOR)
    src = table[:, 18:22].long().tolist()
    for n in range(2):   # the 1 px box is gone wherever image 0 went
        assert int(nv64[n]) <= sum(r["counts"][s] for s in src[n]) - src[n].count(0)
    assert r["nb"] == max(1.0, float(tot64))


def test_denoising_queries_follow_the_mosaicked_counts(hip_lib):
    r = _run(spec=SPEC + "-mosaic-dn100", mosaic=None)
    assert all(torch.isfinite(torch.tensor(r["losses"]))) and r["captures"] <= 2 and r["mosaic_path"]
    nv = r["nv"].tolist()
    labels, G = r["dn_pack"]
    labels = labels.view(2, G, 2, r["M"])
    assert max(nv) > 0
    for b in range(2):
        # class 0 in the slots of the surviving boxes, the no-object class 1 behind them
        assert (labels[b, :, :, :nv[b]] == 0).all() and (labels[b, :, :, nv[b]:] == 1).all(), (b, nv)


def test_same_seed_same_losses(hip_lib):
    a, b, c = _run(), _run(tag=1), _run(seed=1)
    print(a["losses"], b["losses"], c["losses"])
    assert a["losses"] == b["losses"]
    assert torch.equal(a["table"], b["table"]) and torch.equal(a["static_images"], b["static_images"])
    assert not torch.equal(a["table"], c["table"])
    assert a["losses"] != c["losses"]


def test_mosaic_zero_is_the_plain_augmentation(hip_lib):
    off, plain = _run(mosaic=0.0), _run(mosaic=None)
    assert not off["mosaic_path"] and not plain["mosaic_path"] and off["M"] == plain["M"] == 16
    assert off["losses"] == plain["losses"]
    assert torch.equal(off["table"], plain["table"]) and off["table"].shape[1] == 16
    assert torch.equal(off["static_images"], plain["static_images"]) and torch.equal(off["tb"], plain["tb"])
    assert torch.equal(off["nv"], plain["nv"])


def test_eager_gpu_step(hip_lib):
    """graphs=False on the GPU: BatchAugment's own buffers, sized from the same bound."""
    from src.rtdetr_moe.step import TrainStep

    model, crit, images, targets, ctx = _setup(SPEC)
    step = TrainStep(model, crit, images, ctx, graphs=False, world=1, precision="bf16", lr=1e-3, mosaic=1.0,
                     content_hw=HW)
    losses = [float(step(images, ctx, targets, 7.0)) for _ in range(2)]
    torch.cuda.synchronize()
    assert step.aug is not None and step.aug.mosaic_path and step.stepper is None
    assert step.aug.need([len(t["boxes"]) for t in targets]) <= step.aug._out_targets[0].shape[1]
    assert all(torch.isfinite(torch.tensor(losses))), losses
