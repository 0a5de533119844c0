"""rtdetr_eval_match (csrc/evalmatch.hip) against metrics.match_predictions,
per image, on float32 predictions and float64 truth: the tp arrays are equal
bit for bit (assert_array_equal), ties, thresholds hit exactly, degenerate
boxes and numpy's float32 prediction area included."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from eval_match_cases import box_iou_f64_area, random_image, to_targets

pytestmark = pytest.mark.gpu


def _oracle(boxes, scores, labels, gts):
    from src.rtdetr_moe.metrics import match_predictions

    return [match_predictions(boxes[b], scores[b], labels[b], np.asarray(g, np.float64).reshape(-1, 4),
                              np.asarray(gl, np.int64)) for b, (g, gl) in enumerate(gts)]


def _device(boxes, scores, labels, gts, M=None):
    """tp bool [B, K, T] of the kernel; the padding slots hold NaN / 1e30 boxes
    and a label every prediction class matches somewhere (never to be read)."""
    from src.moe import _lib as L
    from src.rtdetr_moe.metrics import IOU_THRESHOLDS

    B = len(gts)
    M = M or max(1, max(len(gl) for _, gl in gts))
    gb = np.full((B, M, 4), np.nan)
    gb[:, 1::2] = 1e30
    glab = np.zeros((B, M), np.int32)
    nv = np.zeros(B, np.int32)
    for b, (g, gl) in enumerate(gts):
        n = len(gl)
        gb[b, :n] = np.asarray(g, np.float64).reshape(-1, 4)
        glab[b, :n] = gl
        glab[b, n:] = labels[b][0]
        nv[b] = n
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tp = L.eval_match(cu(boxes), cu(scores), cu(labels.astype(np.int32)), cu(gb), cu(glab), cu(nv),
                      cu(np.asarray(IOU_THRESHOLDS, np.float64)))
    assert tp.dtype == torch.uint8 and tuple(tp.shape) == (B, boxes.shape[1], len(IOU_THRESHOLDS))
    return tp.cpu().numpy().astype(bool)


def _check(boxes, scores, labels, gts, M=None):
    want = _oracle(boxes, scores, labels, gts)
    got = _device(boxes, scores, labels, gts, M)
    for b, w in enumerate(want):
        np.testing.assert_array_equal(got[b], w, err_msg=f"image {b}")
    return np.stack(want)


@pytest.mark.parametrize("K,M", [(300, 1), (300, 20), (300, 65), (300, 130), (1, 20), (63, 20), (65, 20)])
def test_random_batches(hip_lib, K, M):
    rng = np.random.default_rng(1000 * K + M)
    ns = [0, 1, M, M // 2, min(5, M), M]
    imgs = [random_image(rng, K, n) for n in ns]
    boxes, scores, labels = (np.stack([im[i] for im in imgs]) for i in range(3))
    want = _check(boxes, scores, labels, [(im[3], im[4]) for im in imgs], M)
    if K >= 63:  # the case is not vacuous: true positives at the loosest and misses at the tightest threshold
        assert want[..., 0].any() and want[..., 0].sum() > want[..., -1].sum()


def test_score_ties_and_unsorted_input(hip_lib):
    rng = np.random.default_rng(7)
    K, n = 48, 6
    imgs = [random_image(rng, K, n, classes=1) for _ in range(4)]
    boxes, _, labels = (np.stack([im[i] for im in imgs]) for i in range(3))
    scores = (rng.integers(1, 5, (4, K)) / 4).astype(np.float32)  # 4 distinct values, in no order
    want = _check(boxes, scores, labels, [(im[3], im[4]) for im in imgs])
    # the ties matter: visiting in plain index order, or by an unstable order, changes the result
    from src.rtdetr_moe.metrics import match_predictions

    rev = [match_predictions(boxes[b][::-1], scores[b][::-1], labels[b][::-1], imgs[b][3], imgs[b][4])[::-1]
           for b in range(4)]
    assert any((r != w).any() for r, w in zip(rev, want))


def test_iou_exactly_on_thresholds(hip_lib):
    """Truth [0,0,20,20]; predictions [0,0,20,h], h = 10..19 (IoU = h/20) and
    their mirror images, the lower IoU scored higher, so at each threshold the
    first prediction that passes is the one sitting exactly on it."""
    hs = np.arange(10, 20)
    a = np.stack([np.zeros(10), np.zeros(10), np.full(10, 20.0), hs], 1)
    m = np.stack([np.zeros(10), 20.0 - hs, np.full(10, 20.0), np.full(10, 20.0)], 1)
    gt = np.array([[0.0, 0.0, 20.0, 20.0]])
    gl = np.zeros(1, np.int64)
    desc = np.linspace(0.9, 0.1, 10).astype(np.float32)
    boxes = np.stack([a, m, a, m]).astype(np.float32)
    scores = np.stack([desc, desc, desc[::-1], desc[::-1]])
    labels = np.zeros((4, 10), np.int64)
    want = _check(boxes, scores, labels, [(gt, gl)] * 4)
    assert want[0].sum() == 10  # one prediction per threshold takes the truth
    # each prediction alone against the truth: K = 1, one image per prediction
    _check(np.concatenate([a, m])[:, None].astype(np.float32), np.ones((20, 1), np.float32),
           np.zeros((20, 1), np.int64), [(gt, gl)] * 20)


def test_equal_ious_take_the_lowest_truth(hip_lib):
    box, other = [10.0, 10.0, 50.0, 60.0], [100.5, 100.25, 150.75, 170.5]
    gt = np.array([box, other, box, other, box])
    gl = np.zeros(5, np.int64)
    boxes = np.array([[box, [10.5, 10, 50, 60], [10, 10, 49, 60], [10, 11, 50, 60], other, other, other]],
                     np.float32)
    scores = np.array([[0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3]], np.float32)
    want = _check(boxes, scores, np.zeros((1, 7), np.int64), [(gt, gl)])
    # three copies of `box`: the first three predictions match, the fourth finds none left
    np.testing.assert_array_equal(want[0][:, 0], [1, 1, 1, 0, 1, 1, 0])
    # which of two equal IoUs is taken shows in the next prediction: A overlaps truth 0 and
    # truth 1 equally and takes truth 0, which leaves truth 1 -- its own box -- to B
    gt = np.array([[8.0, 10.0, 48.0, 60.0], [12.0, 10.0, 52.0, 60.0]])
    boxes = np.array([[[10, 10, 50, 60], [12, 10, 52, 60]]], np.float32)
    want = _check(boxes, np.array([[0.9, 0.8]], np.float32), np.zeros((1, 2), np.int64), [(gt, np.zeros(2, np.int64))])
    assert want[0][1].all() and want[0][0, 0]


def test_degenerate_boxes(hip_lib):
    gt = np.array([[5.0, 5.0, 5.0, 9.0],      # zero width
                   [30.0, 30.0, 20.0, 40.0],  # inverted x
                   [7.0, 7.0, 7.0, 7.0],      # a point
                   [0.0, 0.0, 10.0, 10.0]])
    gl = np.zeros(4, np.int64)
    boxes = np.array([[[5, 5, 5, 9],        # identical to the zero-area truth: 0 / max(0, 1e-9)
                       [7, 7, 7, 7],
                       [30, 30, 20, 40],    # inverted, identical to an inverted truth
                       [10, 0, 0, 10],      # inverted over a real truth
                       [0, 0, 10, 10],
                       [0, 0, 10, 0],       # zero height inside a real truth
                       [2, 2, 8, 8]]], np.float32)
    scores = np.linspace(0.9, 0.3, 7).astype(np.float32)[None]
    _check(boxes, scores, np.zeros((1, 7), np.int64), [(gt, gl)])
    _check(boxes, scores[:, ::-1].copy(), np.zeros((1, 7), np.int64), [(gt, gl)])


# (prediction float32 xyxy, truth, index of the IoU threshold whose tp bit depends on the
# prediction area being float32): found by a CPU search over predictions whose IoU sits
# within an ulp of a threshold
F32_AREA_CASES = [
    ([1.673078804742545e-04, 0.0, 106.0, 79.9001235961914], [0.0, 0.0, 106.0, 94.0], 7),
    ([float.fromhex("0x1.aeb56ep-18"), 0.0, 129.0, float.fromhex("0x1.34cccep+7")], [0.0, 0.0, 129.0, 193.0], 6),
    ([float.fromhex("0x1.849324p-15"), 0.0, 258.0, float.fromhex("0x1.81b336p+7")], [0.0, 0.0, 258.0, 203.0], 9),
    ([float.fromhex("0x1.9f1a12p-16"), 0.0, 199.0, float.fromhex("0x1.588002p+7")], [0.0, 0.0, 199.0, 265.0], 3),
    ([float.fromhex("0x1.c5af2cp-16"), 0.0, 374.0, float.fromhex("0x1.e1199cp+7")], [0.0, 0.0, 374.0, 283.0], 7),
]


def test_float32_prediction_area(hip_lib):
    from src.rtdetr_moe.metrics import IOU_THRESHOLDS, box_iou_np

    n = len(F32_AREA_CASES)
    boxes = np.array([[c[0]] for c in F32_AREA_CASES], np.float32)
    gts = [(np.array([c[1]], np.float64), np.zeros(1, np.int64)) for c in F32_AREA_CASES]
    # on the CPU: a float64 prediction area really flips the bit, in both directions over the cases
    flips = set()
    for b, (_, _, ti) in enumerate(F32_AREA_CASES):
        ref = box_iou_np(boxes[b], gts[b][0])[0, 0] >= IOU_THRESHOLDS[ti]
        alt = box_iou_f64_area(boxes[b], gts[b][0])[0, 0] >= IOU_THRESHOLDS[ti]
        assert ref != alt, f"case {b} no longer separates float32 from float64 area"
        flips.add(bool(ref))
    assert flips == {True, False}
    want = _check(boxes, np.ones((n, 1), np.float32), np.zeros((n, 1), np.int64), gts)
    for b, (_, _, ti) in enumerate(F32_AREA_CASES):
        assert want[b, 0, ti] == (box_iou_np(boxes[b], gts[b][0])[0, 0] >= IOU_THRESHOLDS[ti])


def test_limits(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.metrics import DetectionEvaluator, DeviceDetectionEvaluator

    rng = np.random.default_rng(3)
    K = L.EVAL_MATCH_MAX_K + 1
    boxes, scores, labels, gt, gl = random_image(rng, K, 4)
    with pytest.raises(L.MoEKernelError, match="rtdetr_eval_match"):
        _device(boxes[None], scores[None], labels[None], [(gt, gl)])
    # the evaluator runs the host path instead, with the host path's result
    dev, host = DeviceDetectionEvaluator(), DetectionEvaluator()
    L.launch_counts(reset=True)
    W = H = 640
    tg = to_targets([(gt, gl)], W, H)
    cu = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    dev.update_batch(cu(boxes[None]), cu(scores[None]), cu(labels[None]), tg, size=(W, H))
    assert "eval_match" not in L.launch_counts()
    from src.rtdetr_moe.metrics import gt_xyxy_pixels

    host.update(boxes, scores, labels, gt_xyxy_pixels(tg[0]["boxes"].numpy().astype(np.float64), W, H),
                tg[0]["labels"].numpy())
    for name in ("tp", "conf", "pred_cls", "target_cls"):
        np.testing.assert_array_equal(getattr(dev, name)[0], getattr(host, name)[0], err_msg=name)
    assert dev.tp[0].any()
