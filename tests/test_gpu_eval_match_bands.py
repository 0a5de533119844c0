"""rtdetr_eval_match_bands (csrc/evalmatch.hip) against
metrics.match_predictions_banded, per image: the codes are equal bit for bit
(assert_array_equal) over the shapes at which the kernel changes path, 1 / 3 /
8 bands, per-image scales, the constructed ignore-region cases, score ties,
poisoned padding, and the argument limits."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from eval_match_cases import random_image
from size_report_cases import BANDS3, BANDS8, INF, KM_CASES, SCALES, batch, constructed, reference, seeded

pytestmark = pytest.mark.gpu


def _device(boxes, scores, labels, gts, bands, scales=None, M=None, iouv=None):
    """code uint8 [B, R, K, T] of the kernel; the padding slots hold NaN / 1e30
    boxes and a label every prediction class matches somewhere (never to be read)."""
    from src.moe import _lib as L
    from src.rtdetr_moe.metrics import IOU_THRESHOLDS

    iouv = IOU_THRESHOLDS if iouv is None else iouv
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
    sc = np.ones(B) if scales is None else np.asarray(scales, np.float64)
    code = L.eval_match_bands(cu(boxes), cu(scores), cu(labels.astype(np.int32)), cu(gb), cu(glab), cu(nv),
                              cu(np.asarray(iouv, np.float64)), cu(sc), cu(np.asarray(bands, np.float64)))
    assert code.dtype == torch.uint8 and tuple(code.shape) == (B, len(bands), boxes.shape[1], len(iouv))
    return code.cpu().numpy()


def _check(boxes, scores, labels, gts, bands, scales=None, M=None, iouv=None, want=None):
    if want is None:
        want = reference(boxes, scores, labels, gts, bands, scales, iouv)
    got = _device(boxes, scores, labels, gts, bands, scales, M, iouv)
    for b in range(len(gts)):
        for r in range(len(bands)):
            np.testing.assert_array_equal(got[b, r], want[b, r], err_msg=f"image {b} band {r} {bands[r]}")
    return want


@pytest.mark.parametrize("K,M", KM_CASES)
def test_random_batches(hip_lib, K, M):
    """Truth counts [0, 1, M, M // 2, min(5, M), M]: the n <= 64 register path,
    the strided path and the unroll tail (K = 1, 63, 65)."""
    (boxes, scores, labels, gts), want = seeded(K, M)  # bands (0, inf) + BANDS3 at scale 1, shared with the CPU tests
    _check(boxes, scores, labels, gts, [(0.0, INF)] + BANDS3, M=M, want=want)
    # per-image scales move the truths between the bands
    scaled = _check(boxes, scores, labels, gts, BANDS3, SCALES, M)
    if K >= 63:
        assert (scaled != want[:, 1:]).any() and {0, 1, 2} == set(np.unique(scaled[..., 0]).tolist())


@pytest.mark.parametrize("K,M", [(65, 20), (300, 65)])
def test_one_and_eight_bands(hip_lib, K, M):
    boxes, scores, labels, gts = batch(K, M)
    _check(boxes, scores, labels, gts, [(40.0, 80.0)], SCALES, M)
    want = _check(boxes, scores, labels, gts, BANDS8, SCALES, M)
    seen = [set(np.unique(want[:, r, :, 0]).tolist()) for r in range(8)]
    # the whole axis ignores nothing; the narrow band (59.5, 60.25) may hold no truth of a small batch
    assert seen[3] == {0, 1} and seen[6] >= {0, 2} and all(seen[r] == {0, 1, 2} for r in (0, 1, 2, 4, 5, 7)), seen


@pytest.mark.parametrize("T", [1, 16])
def test_one_and_sixteen_thresholds(hip_lib, T):
    boxes, scores, labels, gts = batch(65, 20)
    iouv = np.linspace(0.5, 0.95, T) if T > 1 else np.array([0.5])
    want = _check(boxes, scores, labels, gts, BANDS3, SCALES, 20, iouv)
    assert (want == 1).any()


def test_constructed_cases(hip_lib):
    for name, boxes, scores, gt, bands, scale, want0 in constructed():
        K = len(boxes)
        want = _check(boxes[None], scores[None], np.zeros((1, K), np.int64), [(gt, np.zeros(len(gt), np.int64))],
                      bands, [scale])
        assert want[0, :, :, 0].tolist() == want0, name


def test_score_ties_and_unsorted_input(hip_lib):
    rng = np.random.default_rng(7)
    K, n = 48, 6
    imgs = [random_image(rng, K, n, classes=1) for _ in range(4)]
    boxes, _, labels = (np.stack([im[i] for im in imgs]) for i in range(3))
    scores = (rng.integers(1, 5, (4, K)) / 4).astype(np.float32)  # 4 distinct values, in no order
    gts = [(im[3], im[4]) for im in imgs]
    want = _check(boxes, scores, labels, gts, BANDS3)
    # the ties matter: the reversed input visits equal scores in the other order and gives other codes
    rev = reference(boxes[:, ::-1], scores[:, ::-1], labels[:, ::-1], gts, BANDS3)[:, :, ::-1]
    assert (rev != want).any()


def test_more_truths_than_one_per_lane_with_ignore_regions(hip_lib):
    """The strided path (n > 64) with out-of-band truths that overlap in-band
    ones: the preference and the consumed ignore regions decide codes there."""
    rng = np.random.default_rng(21)
    boxes, scores, labels, gt, gl = random_image(rng, 200, 70, classes=1)
    # a second, taller truth around each of the first 30: it overlaps the same predictions
    tall = gt[:30].copy()
    tall[:, 3] += 0.35 * (tall[:, 3] - tall[:, 1])
    gt2, gl2 = np.concatenate([gt, tall]), np.concatenate([gl, gl[:30]])
    want = _check(boxes[None], scores[None], labels[None], [(gt2, gl2)], BANDS3, [1.0])
    plain = reference(boxes[None], scores[None], labels[None], [(gt2, gl2)], [(0.0, INF)])
    assert (want[0, :, :, 0] == 2).any() and ((want[0] == 1) != (plain[0] == 1)).any()


def test_limits_launch_nothing(hip_lib):
    from src.moe import _lib as L

    rng = np.random.default_rng(3)
    boxes, scores, labels, gt, gl = random_image(rng, 8, 4)
    args = (boxes[None], scores[None], labels[None], [(gt, gl)])
    L.launch_counts(reset=True)
    with pytest.raises(L.MoEKernelError, match="rtdetr_eval_match_bands"):
        _device(*args, [(float(i), float(i + 1)) for i in range(L.EVAL_MATCH_MAX_R + 1)])  # R = 9
    K = L.EVAL_MATCH_MAX_K + 1
    big = random_image(rng, K, 4)
    with pytest.raises(L.MoEKernelError, match="rtdetr_eval_match_bands"):
        _device(big[0][None], big[1][None], big[2][None], [(big[3], big[4])], BANDS3)
    # a NULL pointer, through the C entry point
    d = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = d.data_ptr()
    for null_at in (7, 8, 14):  # scale, bands, code
        a = [p] * 9 + [1, 8, 4, 10, 3, p, None]
        a[null_at] = None
        assert hip_lib.rtdetr_eval_match_bands(*a) != 0
        assert b"NULL pointer" in hip_lib.moe_last_error()
    torch.cuda.synchronize()
    assert int(d.abs().sum()) == 0
    counts = L.launch_counts()
    assert "eval_match_bands" not in counts and "eval_match" not in counts, counts
