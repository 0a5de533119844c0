"""The host side of the device matching path (no GPU): the device evaluator on
CPU tensors is the host evaluator, the shared ground-truth helper reproduces
the expression engine._evaluate used inline, the binding refuses CPU tensors,
and a CPU evaluation never touches the library."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from eval_match_cases import random_image, to_targets

W, H = 640, 480


def test_device_evaluator_on_cpu_tensors_is_the_host_evaluator(monkeypatch):
    from src.moe import _lib as L
    from src.rtdetr_moe.metrics import DetectionEvaluator, DeviceDetectionEvaluator, gt_xyxy_pixels

    monkeypatch.setattr(L, "lib", lambda: pytest.fail("the CPU path loaded the HIP library"))
    rng = np.random.default_rng(5)
    K = 40
    imgs = [random_image(rng, K, n, size=float(H)) for n in (3, 0, 6, 1, 2)]
    imgs[0][1][::7] = 0.0005  # rows under conf_thres
    for switch in ("1", "0"):
        monkeypatch.setenv("MOE_EVAL_MATCH", switch)
        dev, host = DeviceDetectionEvaluator(), DetectionEvaluator()
        for s in (0, 3):  # a batch of 3 and a batch of 2
            chunk = imgs[s:s + 3]
            tg = to_targets([(im[3], im[4]) for im in chunk], W, H)
            b, sc, lb = (torch.from_numpy(np.stack([im[i] for im in chunk])) for i in range(3))
            dev.update_batch(b, sc, lb, tg, size=(W, H))
            for im, t in zip(chunk, tg):
                host.update(im[0], im[1], im[2], gt_xyxy_pixels(t["boxes"].numpy().astype(np.float64), W, H),
                            t["labels"].numpy())
        assert len(dev.tp) == 5
        for name in ("tp", "conf", "pred_cls", "target_cls"):
            for x, y in zip(getattr(dev, name), getattr(host, name)):
                assert x.dtype == y.dtype
                np.testing.assert_array_equal(x, y, err_msg=name)
        assert len(dev.tp[0]) < K and dev.tp[0].any()
        bd, bh = dev.compute(), host.compute()
        assert (bd.mp, bd.mr, bd.map50, bd.map) == (bh.mp, bh.mr, bh.map50, bh.map) and bh.map50 > 0
        assert dev.average_recall() == host.average_recall()


def test_gt_helper_reproduces_the_inline_expression():
    from src.rtdetr_moe.metrics import gt_xyxy_pixels

    rng = np.random.default_rng(0)
    for n, (w, h) in ((0, (640, 640)), (1, (1248, 704)), (17, (1280, 736))):
        gt = torch.from_numpy(rng.random((n, 4)).astype(np.float32)).numpy().astype(np.float64)
        want = np.stack([(gt[:, 0] - gt[:, 2] / 2) * w, (gt[:, 1] - gt[:, 3] / 2) * h,
                         (gt[:, 0] + gt[:, 2] / 2) * w, (gt[:, 1] + gt[:, 3] / 2) * h], 1) \
            if len(gt) else np.zeros((0, 4))
        got = gt_xyxy_pixels(gt, w, h)
        assert got.dtype == np.float64 and got.shape == (n, 4)
        assert got.tobytes() == want.tobytes()


def test_eval_match_refuses_cpu_tensors():
    from src.moe import _lib as L

    z = lambda shape, dt: torch.zeros(shape, dtype=dt)  # noqa: E731
    with pytest.raises(L.MoEKernelError, match="GPU tensor"):
        L.eval_match(z((1, 4, 4), torch.float32), z((1, 4), torch.float32), z((1, 4), torch.int32),
                     z((1, 2, 4), torch.float64), z((1, 2), torch.int32), z((1,), torch.int32),
                     z((10,), torch.float64))
    assert "rtdetr_eval_match" in L.SIGNATURES and L.PROF_KINDS[16] == "eval_match"


@pytest.mark.parametrize("switch", ["1", "0"])
def test_cpu_evaluate_never_touches_the_library(monkeypatch, switch):
    from src.moe import _lib as L
    from src.rtdetr_moe import engine
    from src.rtdetr_moe.metrics import DetectionEvaluator, DeviceDetectionEvaluator
    from src.rtdetr_moe.model import RTDETRMoE

    monkeypatch.setenv("MOE_EVAL_MATCH", switch)
    monkeypatch.setattr(L, "lib", lambda: pytest.fail("a CPU evaluation loaded the HIP library"))
    torch.manual_seed(0)
    model = RTDETRMoE("rtdetr-r18-moe4-top1")
    evs, speed = [], {}
    box = engine._evaluate(model, "synthetic:1", "val", (128, 128), 2, torch.device("cpu"), 0, 0, speed, ev_out=evs)
    assert type(evs[0]) is DetectionEvaluator and not isinstance(evs[0], DeviceDetectionEvaluator)
    assert len(evs[0].tp) == 2 and 0.0 <= box.map50 <= 1.0 and speed["postprocess"] > 0
