"""The size report's device path above the kernel:
DeviceDetectionEvaluator.update_batch(bands=...) against
DetectionEvaluator.update(bands=...) on the same tensors, and engine._evaluate
with MOE_EVAL_MATCH on and off.  Everything is compared for equality: the
device path may not move a code or a metric by an ulp."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from eval_match_cases import random_image, to_targets
from size_report_cases import BANDS3

pytestmark = pytest.mark.gpu

W, H = 640, 480
NAMES = ["far", "medium", "near"]


def _same_lists(a, b, names=("tp", "conf", "pred_cls", "target_cls", "codes")):
    assert len(a.tp) == len(b.tp) > 0
    for name in names:
        xs, ys = getattr(a, name), getattr(b, name)
        assert len(xs) == len(ys), name
        for i, (x, y) in enumerate(zip(xs, ys)):
            assert x.dtype == y.dtype and x.shape == y.shape, (name, i, x.dtype, y.dtype, x.shape, y.shape)
            np.testing.assert_array_equal(x, y, err_msg=f"{name}[{i}]")


def _same_band_targets(a, b):
    assert len(a.band_target_cls) == len(b.band_target_cls)
    for i, (xs, ys) in enumerate(zip(a.band_target_cls, b.band_target_cls)):
        assert len(xs) == len(ys)
        for x, y in zip(xs, ys):
            assert x.dtype == y.dtype
            np.testing.assert_array_equal(x, y, err_msg=f"band_target_cls[{i}]")


def _images():
    rng = np.random.default_rng(11)
    K = 100
    counts = [0, 3, 7, 1, 12, 0, 5, 2]
    imgs = [random_image(rng, K, counts[i % 8] + i // 8, size=float(H)) for i in range(44)]
    for im in imgs:
        im[1][rng.random(K) < 0.1] = 0.0005  # some rows under conf_thres
    scales = [(1.0, 3848 / 1248, 0.5, 2.0)[i % 4] for i in range(44)]
    return K, imgs, scales


def _run(dev, host, imgs, scales, bands):
    from src.rtdetr_moe.metrics import gt_xyxy_pixels

    for s in range(0, 44, 8):  # 40 images in five batches of 8, then a partial batch of 4
        chunk = imgs[s:s + 8]
        tg = to_targets([(im[3], im[4]) for im in chunk], W, H)
        b, sc, lb = (torch.from_numpy(np.stack([im[i] for im in chunk])).cuda() for i in range(3))
        kw = {} if bands is None else dict(bands=bands, scales=scales[s:s + 8])
        dev.update_batch(b, sc, lb, tg, size=(W, H), **kw)
        for i, (im, t) in enumerate(zip(chunk, tg)):
            kw = {} if bands is None else dict(bands=bands, scale=scales[s + i])
            host.update(im[0], im[1], im[2], gt_xyxy_pixels(t["boxes"].numpy().astype(np.float64), W, H),
                        t["labels"].numpy(), **kw)


def test_device_evaluator_equals_host_evaluator(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.metrics import DetectionEvaluator, DeviceDetectionEvaluator

    K, imgs, scales = _images()
    dev, host = DeviceDetectionEvaluator(), DetectionEvaluator()
    L.launch_counts(reset=True)
    _run(dev, host, imgs, scales, BANDS3)
    counts = L.launch_counts()
    assert counts.get("eval_match_bands") == 6 and counts.get("eval_match") == 6, counts  # one of each per batch
    _same_lists(dev, host)
    _same_band_targets(dev, host)
    assert all(c.dtype == np.uint8 and c.shape == (3, len(t), 10) for c, t in zip(dev.codes, dev.tp))
    assert any(len(t) < K for t in dev.tp)
    bd, bh = dev.compute_by_size(NAMES), host.compute_by_size(NAMES)
    assert bd == bh
    assert all(bh[n]["targets"] > 0 and bh[n]["AP50"] > 0 and bh[n]["LAMR"] < 1 for n in NAMES + ["all"]), bh
    assert bh["all"]["AP50"] == host.compute().map50 == dev.compute().map50


def test_without_bands_nothing_changes(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.metrics import DetectionEvaluator, DeviceDetectionEvaluator

    _, imgs, scales = _images()
    dev, host = DeviceDetectionEvaluator(), DetectionEvaluator()
    L.launch_counts(reset=True)
    _run(dev, host, imgs, scales, None)
    counts = L.launch_counts()
    assert counts.get("eval_match") == 6 and "eval_match_bands" not in counts, counts
    _same_lists(dev, host, ("tp", "conf", "pred_cls", "target_cls"))
    assert dev.codes == [] and dev.band_target_cls == [] and dev.bands is None
    # and the lists are those of a run with bands
    banded, host2 = DeviceDetectionEvaluator(), DetectionEvaluator()
    _run(banded, host2, imgs, scales, BANDS3)
    _same_lists(dev, banded, ("tp", "conf", "pred_cls", "target_cls"))


def test_evaluate_is_identical_with_the_switch_on_and_off(hip_lib, monkeypatch):
    from src.moe import _lib as L
    from src.rtdetr_moe import engine
    from src.rtdetr_moe.model import RTDETRMoE

    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    model = RTDETRMoE("rtdetr-r18-moe4-top1").to(dev).to(memory_format=torch.channels_last)
    bands = [("low", 0, 150), ("high", 150, None)]
    runs = {}
    for switch in ("1", "0", "off"):
        monkeypatch.setenv("MOE_EVAL_MATCH", "0" if switch == "0" else "1")
        evs, report = [], ({} if switch != "off" else None)
        L.launch_counts(reset=True)
        box = engine._evaluate(model, "synthetic:2", "val", (640, 640), 2, dev, 0, 0, None, ev_out=evs,
                               size_report=report, size_bands=bands)
        torch.cuda.synchronize()
        runs[switch] = (box, evs[0], L.launch_counts(reset=True), report)
    assert runs["1"][2].get("eval_match_bands") == 2 == runs["1"][2].get("eval_match"), runs["1"][2]
    assert "eval_match_bands" not in runs["0"][2] and "eval_match" not in runs["0"][2], runs["0"][2]
    assert "eval_match_bands" not in runs["off"][2] and runs["off"][2].get("eval_match") == 2, runs["off"][2]
    _same_lists(runs["1"][1], runs["0"][1])
    _same_band_targets(runs["1"][1], runs["0"][1])
    assert runs["1"][3] == runs["0"][3]
    rep = runs["1"][3]
    assert rep["unit"] == "source px" and rep["images"] == 4
    assert rep["bands"] == [{"name": "low", "lo": 0.0, "hi": 150.0}, {"name": "high", "lo": 150.0, "hi": None}]
    assert list(rep["detection"]) == ["low", "high", "all"]
    assert rep["detection"]["low"]["targets"] + rep["detection"]["high"]["targets"] == rep["detection"]["all"]["targets"] > 0
    # with the report off the pass appends what it did before the feature
    _same_lists(runs["off"][1], runs["1"][1], ("tp", "conf", "pred_cls", "target_cls"))
    assert runs["off"][1].codes == [] and runs["off"][3] is None
    for k in ("mp", "mr", "map50", "map"):
        assert getattr(runs["off"][0], k) == getattr(runs["1"][0], k) == getattr(runs["0"][0], k), k
