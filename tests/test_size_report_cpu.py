"""The size-stratified validation report on the CPU:
the banded reference matcher on constructed and seeded cases, the reduction
(AP per band with per-column ignore rows, log-average miss rate) against
answers worked out by hand, ``src_size`` from the loaders, and engine.validate
end to end on tests/golden/zod_mini.  Every comparison is ``==``."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
import torch

from eval_match_cases import random_image
from size_report_cases import BANDS3, INF, KM_CASES, constructed, seeded

FIX = Path(__file__).resolve().parent / "golden" / "zod_mini"
MODEL = "rtdetr-r18-moe4-top1"
IMGSZ = (320, 640)
ROW_KEYS = {"targets", "AP50", "AP50-95", "recall", "LAMR"}


def zod_mini_data(split="val"):
    return {split: {"img_folder": str(FIX / "frames"), "ann_file": str(FIX / "annotations" / "instances_train.json")}}


# ---------------------------------------------------------------------------
# the reference matcher
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", constructed(), ids=lambda c: c[0])
def test_constructed_cases(case):
    from src.rtdetr_moe.metrics import match_predictions_banded

    _, boxes, scores, gt, bands, scale, want = case
    K = len(boxes)
    code = match_predictions_banded(boxes, scores, np.zeros(K, np.int64), gt, np.zeros(len(gt), np.int64), bands, scale)
    assert code.dtype == np.uint8 and code.shape == (len(bands), K, 10)
    assert code[:, :, 0].tolist() == want


def test_preference_changes_the_taken_chain():
    """The preference case next to the plain matcher: there P takes the
    better-overlapping truth B and Q is left a false positive."""
    from src.rtdetr_moe.metrics import match_predictions

    _, boxes, scores, gt, _, _, _ = constructed()[0]
    tp = match_predictions(boxes, scores, np.zeros(2, np.int64), gt, np.zeros(2, np.int64))
    assert tp[:, 0].tolist() == [True, False]


def test_fp32_height_case_separates_the_dtypes():
    case = {c[0]: c for c in constructed()}["fp32 height"]
    y1, y2 = case[1][0, 1], case[1][0, 3]
    assert y1.dtype == np.float32 and float(y2 - y1) == 40.0 and float(y2) - float(y1) < 40.0


def test_band_arguments():
    from src.rtdetr_moe.metrics import check_bands, match_predictions_banded, named_bands

    for bad in ([], [(0, 1)] * 9, [(5, 5)], [(6, 5)], [(-1, 5)], [(0, float("nan"))], [(INF, INF)], [(0, 1, 2)], [3]):
        with pytest.raises(ValueError, match="bands"):
            check_bands(bad)
    assert check_bands([(0, INF)] * 8).shape == (8, 2)
    z = np.zeros((0, 4), np.float32)
    empty = match_predictions_banded(z, np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros((0, 4)),
                                     np.zeros(0, np.int64), BANDS3)
    assert empty.shape == (3, 0, 10) and empty.dtype == np.uint8
    names, bands = named_bands()
    assert names == ["far", "medium", "near"] and bands.tolist() == [[0, 40], [40, 100], [100, INF]]
    assert named_bands([("a", 0, 10), ("b", 10, None)])[1].tolist() == [[0, 10], [10, INF]]
    for bad in ([("a", 0, 10), ("a", 10, 20)], [("all", 0, 10)], [(0, 10)], ["far"], [("a", 10, 0)], []):
        with pytest.raises(ValueError, match="bands"):
            named_bands(bad)


@pytest.mark.parametrize("K,M", KM_CASES)
def test_one_open_band_equals_match_predictions(K, M):
    from src.rtdetr_moe.metrics import match_predictions

    (boxes, scores, labels, gts), code = seeded(K, M)
    for b, (g, gl) in enumerate(gts):
        want = match_predictions(boxes[b], scores[b], labels[b], g, gl)
        np.testing.assert_array_equal(code[b, 0], want.astype(np.uint8), err_msg=f"image {b}")


@pytest.mark.parametrize("K,M", KM_CASES)
def test_seeded_cases_are_not_vacuous(K, M):
    """Every code occurs in every band at IoU 0.5 (over the batch) whenever K >= 63."""
    _, code = seeded(K, M)
    counts = [[int((code[:, 1 + r, :, 0] == c).sum()) for c in (0, 1, 2)] for r in range(len(BANDS3))]
    print(f"K {K} M {M}: counts of codes 0/1/2 per band {counts}")
    assert set(np.unique(code).tolist()) <= {0, 1, 2}
    if K >= 63:
        assert min(min(row) for row in counts) > 0, counts


# ---------------------------------------------------------------------------
# the reduction
# ---------------------------------------------------------------------------
def test_ap_with_an_ignored_row_by_hand():
    """Two in-band truths; rows TP(.9), ignored(.8), FP(.7), TP(.6).  Without
    the ignored row: recall .5, .5, 1 and precision 1, 1/2, 2/3, envelope 1,
    2/3, 2/3 -> 51 recall points at 1 and 50 at 2/3."""
    from src.rtdetr_moe.metrics import size_band_metrics

    code = np.array([[1], [2], [0], [1]], np.uint8)
    conf = np.array([0.9, 0.8, 0.7, 0.6], np.float32)
    row = size_band_metrics(code, conf, np.zeros(4, np.int64), np.zeros(2, np.int64), images=1)
    want = float(np.array([1.0] * 51 + [2 / 3] * 50).mean())
    assert abs(want - (51 + 50 * 2 / 3) / 101) < 1e-15
    assert row["targets"] == 2 and row["AP50"] == want == row["AP50-95"] and row["recall"] == 1.0
    # the ignored row counted as a false positive would give precision 1, 1/2, 1/3, 1/2
    as_fp = size_band_metrics(np.array([[1], [0], [0], [1]], np.uint8), conf, np.zeros(4, np.int64),
                              np.zeros(2, np.int64), images=1)
    assert as_fp["AP50"] == float(np.array([1.0] * 51 + [0.5] * 50).mean())
    # input order does not matter: rows are sorted by score
    perm = [2, 0, 3, 1]
    assert size_band_metrics(code[perm], conf[perm], np.zeros(4, np.int64), np.zeros(2, np.int64), images=1) == row


def test_ignored_rows_are_dropped_per_column():
    """One truth, two columns: the row ignored in column 0 is a false positive in column 1."""
    from src.rtdetr_moe.metrics import size_band_metrics

    code = np.array([[2, 0], [1, 1]], np.uint8)
    row = size_band_metrics(code, np.array([0.9, 0.8], np.float32), np.zeros(2, np.int64), np.zeros(1, np.int64), 1)
    assert row["AP50"] == 1.0 and row["AP50-95"] == (1.0 + 0.5) / 2
    # two classes, one without in-band truths: the mean is over the class that has them
    row2 = size_band_metrics(code, np.array([0.9, 0.8], np.float32), np.array([1, 0]), np.zeros(1, np.int64), 1)
    assert row2["AP50"] == 1.0 == row2["AP50-95"]


def test_lamr_by_hand():
    from src.rtdetr_moe.metrics import log_average_miss_rate

    # 2 images, 4 targets; by score: TP FP TP ignored FP TP -> fppi 0 .5 .5 1 1, mr .75 .75 .5 .5 .25.
    # The references 0.01 .. 0.316 (seven) read row 0, 0.562 reads the last row at fppi .5, 1.0 the last row.
    code = np.array([1, 0, 1, 2, 0, 1], np.uint8)
    conf = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4], np.float32)
    want = float(np.exp(np.mean(np.log(np.array([0.75] * 7 + [0.5, 0.25])))))
    assert log_average_miss_rate(code, conf, 4, 2) == want
    perm = [5, 3, 1, 0, 2, 4]
    assert log_average_miss_rate(code[perm], conf[perm], 4, 2) == want
    # a false positive first, one image: no row at fppi < 1 -> 1.0 at eight references, mr 0 -> 1e-10 at the last
    got = log_average_miss_rate(np.array([0, 1], np.uint8), np.array([0.9, 0.8], np.float32), 1, 1)
    assert got == float(np.exp(np.mean(np.log(np.array([1.0] * 8 + [1e-10])))))
    assert log_average_miss_rate(np.zeros(0, np.uint8), np.zeros(0, np.float32), 3, 2) == 1.0  # no detections
    assert log_average_miss_rate(code, conf, 0, 2) is None


def _evaluator(bands, n_images=24, scale=1.0):
    from src.rtdetr_moe.metrics import DetectionEvaluator

    rng = np.random.default_rng(5)
    images = [random_image(rng, 40, 0 if i % 7 == 3 else int(rng.integers(1, 9))) for i in range(n_images)]
    ev = DetectionEvaluator()
    for im in images:
        im[1][rng.random(40) < 0.1] = 0.0005  # some rows under conf_thres
        ev.update(*im, bands=bands, scale=scale)
    return ev, images


def test_compute_by_size():
    from src.rtdetr_moe.metrics import DetectionEvaluator, _in_band, check_bands

    bands = [(0.0, 40.0), (40.0, 80.0), (80.0, INF), (500.0, 600.0)]
    ev, images = _evaluator(bands)
    assert all(c.shape == (4, len(t), 10) and c.dtype == np.uint8 for c, t in zip(ev.codes, ev.tp))
    assert any(len(t) < 40 for t in ev.tp)  # rows under conf_thres are dropped from the codes as from tp
    by = ev.compute_by_size(["far", "medium", "near", "none"])
    assert list(by) == ["far", "medium", "near", "none", "all"] and all(set(r) == ROW_KEYS for r in by.values())
    gh = np.concatenate([im[3][:, 3] - im[3][:, 1] for im in images])
    for r, name in enumerate(["far", "medium", "near", "none"]):
        assert by[name]["targets"] == int(_in_band(gh, check_bands(bands))[r].sum())
    assert sum(by[n]["targets"] for n in ("far", "medium", "near")) == by["all"]["targets"] == len(gh)
    # a band without in-band truths reports null metrics
    assert by["none"] == {"targets": 0, "AP50": None, "AP50-95": None, "recall": None, "LAMR": None}
    for name in ("far", "medium", "near"):
        row = by[name]
        assert row["targets"] > 0 and 0.0 < row["AP50-95"] < row["AP50"] <= 1.0
        assert 0.0 < row["recall"] <= 1.0 and 0.0 < row["LAMR"] <= 1.0
    # the "all" row is compute()'s
    box = ev.compute()
    assert by["all"]["AP50"] == box.map50 > 0 and by["all"]["AP50-95"] == box.map
    # compute() and the lists are untouched by the bands
    plain = DetectionEvaluator()
    for im in images:
        plain.update(*im)
    assert plain.codes == [] and plain.band_target_cls == [] and plain.bands is None
    for name in ("tp", "conf", "pred_cls", "target_cls"):
        for x, y in zip(getattr(ev, name), getattr(plain, name)):
            np.testing.assert_array_equal(x, y)
    assert plain.compute().map == box.map
    with pytest.raises(ValueError, match="bands"):
        plain.compute_by_size(["a"])
    with pytest.raises(ValueError, match="bands"):
        ev.update(*images[0], bands=[(0.0, 41.0)])  # another table than the earlier updates'
    ev.update(*images[0])  # an update without bands
    with pytest.raises(ValueError, match="bands"):
        ev.compute_by_size(["far", "medium", "near", "none"])


def test_one_open_band_reduces_to_the_all_row():
    """With the band (0, inf) and valid boxes nothing is ignored, so the band's
    row is the unstratified one: the same AP, recall and LAMR as "all"."""
    ev, _ = _evaluator([(0.0, INF)])
    by = ev.compute_by_size(["whole"])
    assert by["whole"] == by["all"] and by["all"]["LAMR"] is not None


# ---------------------------------------------------------------------------
# loaders and engine
# ---------------------------------------------------------------------------
def _write_frames(img_dir: Path, sizes):
    from PIL import Image

    img_dir.mkdir(parents=True)
    for i, (w, h) in enumerate(sizes):
        Image.new("RGB", (w, h), (40 * (i + 1),) * 3).save(img_dir / f"{i:06d}.png")


def test_loaders_add_src_size(tmp_path):
    from src.rtdetr_moe.data import CocoDataset, YoloDataset

    h, w = 48, 80  # evaluated size; padded to 64 x 96
    sizes = [(2 * w, 2 * h), (w, h)]  # the first frame is twice the evaluated size
    root = tmp_path / "yolo"
    _write_frames(root / "images" / "val", sizes)
    (root / "labels" / "val").mkdir(parents=True)
    (root / "labels" / "val" / "000000.txt").write_text("0 0.5 0.5 0.25 0.5\n")
    (root / "dataset.yaml").write_text(f"path: {root}\nval: images/val\nnc: 1\nnames:\n  0: pedestrian\n")
    ds = YoloDataset(root / "dataset.yaml", split="val", imgsz=(h, w))
    boxes = torch.tensor([[0.5 * w / 96, 0.5 * h / 64, 0.25 * w / 96, 0.5 * h / 64]], dtype=torch.float32)
    for i, size in enumerate(sizes):
        img, t, _ = ds[i]
        assert tuple(img.shape) == (3, 64, 96)
        assert set(t) == {"boxes", "labels", "orig_size", "src_size"}
        assert t["src_size"] == size and t["orig_size"] == (96, 64)
        assert torch.equal(t["boxes"], boxes if i == 0 else boxes[:0]) and t["labels"].tolist() == [0] * (1 - i)
        assert t["boxes"].dtype == torch.float32 and t["labels"].dtype == torch.int64

    _write_frames(tmp_path / "coco", sizes)
    ann = tmp_path / "ann.json"
    ann.write_text(json.dumps({
        "images": [{"id": i, "file_name": f"{i:06d}.png", "width": s[0], "height": s[1]} for i, s in enumerate(sizes)],
        "annotations": [{"id": 1, "image_id": 0, "category_id": 1, "bbox": [60, 24, 40, 48], "area": 1.0, "iscrowd": 0}],
        "categories": [{"id": 1, "name": "pedestrian"}]}))
    cd = CocoDataset(tmp_path / "coco", ann, imgsz=(h, w))
    for i, size in enumerate(sizes):
        _, t, _ = cd[i]
        assert set(t) == {"boxes", "labels", "orig_size", "src_size"}
        assert t["src_size"] == size and t["orig_size"] == (96, 64)
        assert torch.equal(t["boxes"], boxes if i == 0 else boxes[:0]) and t["labels"].tolist() == [0] * (1 - i)


def _check_schema(report, bands):
    assert list(report) == ["unit", "bands", "images", "detection"]
    assert report["unit"] == "source px" and report["bands"] == bands and report["images"] == 4
    names = [b["name"] for b in bands]
    assert list(report["detection"]) == names + ["all"]
    for row in report["detection"].values():
        assert set(row) == ROW_KEYS and isinstance(row["targets"], int)
        for k in ROW_KEYS - {"targets"}:
            assert (row[k] is None) if row["targets"] == 0 else (0.0 <= row[k] <= 1.0)
    assert sum(report["detection"][n]["targets"] for n in names) == report["detection"]["all"]["targets"] == 6


def test_validate_writes_the_size_report(tmp_path, monkeypatch):
    from src.rtdetr_moe import engine

    monkeypatch.delenv("MOE_SIZE_REPORT", raising=False)
    kw = dict(imgsz=IMGSZ, batch=3, device="cpu", workers=0)
    torch.manual_seed(0)
    off = engine.validate(MODEL, zod_mini_data(), project=str(tmp_path), name="off", **kw)
    assert off.size is None and not (tmp_path / "off" / "size_report.json").exists()
    torch.manual_seed(0)
    on = engine.validate(MODEL, zod_mini_data(), project=str(tmp_path), name="on", size_report=True, **kw)
    assert on.results_dict == off.results_dict
    default = [{"name": "far", "lo": 0.0, "hi": 40.0}, {"name": "medium", "lo": 40.0, "hi": 100.0},
               {"name": "near", "lo": 100.0, "hi": None}]
    _check_schema(on.size, default)
    assert on.size["detection"]["all"]["AP50"] == on.box.map50 and on.size["detection"]["all"]["AP50-95"] == on.box.map
    on_disk = json.loads((tmp_path / "on" / "size_report.json").read_text())
    assert on_disk == json.loads(json.dumps(on.size)) == on.size
    assert not (tmp_path / "on" / "context_report.json").exists()
    # the environment switch, configured bands, and both reports at once
    monkeypatch.setenv("MOE_SIZE_REPORT", "1")
    torch.manual_seed(0)
    both = engine.validate(MODEL, zod_mini_data(), context_report=True,
                           size_bands=[("small", 0, 1e9), ("huge", 1e9, None)], **kw)
    assert both.context is not None and both.results_dict == off.results_dict
    _check_schema(both.size, [{"name": "small", "lo": 0.0, "hi": 1e9}, {"name": "huge", "lo": 1e9, "hi": None}])
    # one band holding every box is the unstratified row; the other has no truth
    assert both.size["detection"]["small"] == both.size["detection"]["all"] == on.size["detection"]["all"]
    assert both.size["detection"]["huge"]["targets"] == 0 and both.size["detection"]["huge"]["LAMR"] is None


def test_validate_scales_heights_to_the_source_frame(monkeypatch):
    """zod_mini's frames are larger than the evaluated 320 x 640, so a truth's
    band follows its height in the frame, not in the tensor."""
    from src.rtdetr_moe import engine

    monkeypatch.delenv("MOE_SIZE_REPORT", raising=False)
    d = json.loads((FIX / "annotations" / "instances_train.json").read_text())
    heights = [a["bbox"][3] for a in d["annotations"]]
    src_h = {im["height"] for im in d["images"]}
    assert len(heights) == 6 and all(h > IMGSZ[0] for h in src_h)
    edge = float(np.median(heights))
    torch.manual_seed(0)
    m = engine.validate(MODEL, zod_mini_data(), imgsz=IMGSZ, batch=3, device="cpu", workers=0, size_report=True,
                        size_bands=[("lo", 0, edge), ("hi", edge, None)])
    assert m.size["detection"]["lo"]["targets"] == sum(h < edge for h in heights) > 0
    assert m.size["detection"]["hi"]["targets"] == sum(h >= edge for h in heights) > 0


def test_size_bands_are_validated():
    from src.rtdetr_moe import engine

    for bad in ([("a", 10, 5)], [("a", 0, 10)] * 9, [("a", 0, 10), ("a", 10, 20)], [("all", 0, 10)], [(0, 10)], []):
        with pytest.raises(ValueError, match="bands"):
            engine.validate(MODEL, zod_mini_data(), imgsz=IMGSZ, batch=3, device="cpu", workers=0, size_report=True,
                            size_bands=bad)
