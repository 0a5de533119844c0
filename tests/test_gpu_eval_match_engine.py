"""The device matching path above the kernel: DeviceDetectionEvaluator against
DetectionEvaluator on the same tensors, engine._evaluate with MOE_EVAL_MATCH on
and off, and RTDETRMoE.postprocess_batched against postprocess.  Everything is
compared for equality: the device path may not move a metric by an ulp."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from eval_match_cases import random_image, to_targets

pytestmark = pytest.mark.gpu

W, H = 640, 480


def _same_lists(a, b):
    assert len(a.tp) == len(b.tp) > 0
    for name in ("tp", "conf", "pred_cls", "target_cls"):
        for i, (x, y) in enumerate(zip(getattr(a, name), getattr(b, name))):
            assert x.dtype == y.dtype and x.shape == y.shape, (name, i, x.dtype, y.dtype, x.shape, y.shape)
            np.testing.assert_array_equal(x, y, err_msg=f"{name}[{i}]")


def _same_metrics(a, b):
    for k in ("mp", "mr", "map50", "map"):
        assert getattr(a, k) == getattr(b, k), k
    assert len(a.curves_results) == len(b.curves_results)
    for ca, cb in zip(a.curves_results, b.curves_results):
        np.testing.assert_array_equal(ca[0], cb[0])
        np.testing.assert_array_equal(ca[1], cb[1])


def test_device_evaluator_equals_host_evaluator(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.metrics import DetectionEvaluator, DeviceDetectionEvaluator, gt_xyxy_pixels

    rng = np.random.default_rng(11)
    K = 100
    counts = [0, 3, 7, 1, 12, 0, 5, 2]
    imgs = [random_image(rng, K, counts[i % 8] + i // 8, size=float(H)) for i in range(44)]
    for im in imgs:
        im[1][rng.random(K) < 0.1] = 0.0005  # some rows under conf_thres
    dev, host = DeviceDetectionEvaluator(), DetectionEvaluator()
    L.launch_counts(reset=True)
    for s in range(0, 44, 8):  # 40 images in five batches of 8, then a partial batch of 4
        chunk = imgs[s:s + 8]
        tg = to_targets([(im[3], im[4]) for im in chunk], W, H)
        b, sc, lb = (torch.from_numpy(np.stack([im[i] for im in chunk])).cuda() for i in range(3))
        dev.update_batch(b, sc, lb, tg, size=(W, H))
        for im, t in zip(chunk, tg):
            host.update(im[0], im[1], im[2], gt_xyxy_pixels(t["boxes"].numpy().astype(np.float64), W, H),
                        t["labels"].numpy())
    assert L.launch_counts().get("eval_match") == 6  # one launch per batch
    _same_lists(dev, host)
    assert all(t.dtype == bool and t.shape[1] == 10 for t in dev.tp) and any(len(t) < K for t in dev.tp)
    bd, bh = dev.compute(), host.compute()
    assert bh.map50 > 0.0
    _same_metrics(bd, bh)
    assert dev.average_recall() == host.average_recall()


def test_evaluate_is_identical_with_the_switch_on_and_off(hip_lib, monkeypatch):
    from src.moe import _lib as L
    from src.rtdetr_moe import engine
    from src.rtdetr_moe.model import RTDETRMoE

    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    model = RTDETRMoE("rtdetr-r18-moe4-top1").to(dev).to(memory_format=torch.channels_last)
    runs = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("MOE_EVAL_MATCH", switch)
        evs, speed = [], {}
        L.launch_counts(reset=True)
        box = engine._evaluate(model, "synthetic:2", "val", (640, 640), 2, dev, 0, 0, speed, ev_out=evs)
        torch.cuda.synchronize()
        runs[switch] = (box, evs[0], L.launch_counts(reset=True), speed)
    assert runs["1"][2].get("eval_match") == 2, runs["1"][2]  # one launch per batch
    assert "eval_match" not in runs["0"][2], runs["0"][2]
    _same_lists(runs["1"][1], runs["0"][1])
    _same_metrics(runs["1"][0], runs["0"][0])
    assert runs["1"][1].average_recall() == runs["0"][1].average_recall()
    for sp in (runs["1"][3], runs["0"][3]):
        assert sp["postprocess"] > 0 and sp["inference"] > 0


def test_postprocess_batched_slices_to_postprocess(hip_lib):
    from src.rtdetr_moe.model import RTDETRMoE

    torch.manual_seed(0)
    model = RTDETRMoE("rtdetr-r18-moe4-top1")
    g = torch.Generator().manual_seed(1)
    out = {"pred_logits": torch.randn((3, 300, 1), generator=g).cuda(),
           "pred_boxes": torch.rand((3, 300, 4), generator=g).cuda()}
    sizes = [(640, 480)] * 3
    xyxy, sc, lb = model.postprocess_batched(out, sizes)
    assert tuple(xyxy.shape) == (3, 300, 4) and tuple(sc.shape) == (3, 300) == tuple(lb.shape) and xyxy.is_cuda
    dets = model.postprocess(out, sizes)
    assert len(dets) == 3
    for i, d in enumerate(dets):
        assert torch.equal(d["boxes"], xyxy[i]) and torch.equal(d["scores"], sc[i]) and torch.equal(d["labels"], lb[i])
