"""Detection metrics computed in-house (pycocotools / faster_coco_eval are
absent here).  Produces what the reference's serializer
reads from an Ultralytics metrics object (src/models/vision/yolo.py:204-300):
``results_dict`` keys ``metrics/{precision,recall,mAP50,mAP50-95}(B)``,
``box.{map50,map,mp,mr,curves,curves_results}`` and ``speed``.

AP per class: predictions matched greedily by descending score to unmatched
ground truth of the same class at IoU thresholds 0.50:0.05:0.95; AP is the
area under the monotone precision envelope sampled at 101 recall points
(COCO interpolation, pycocotools' accumulate).  P and R are reported at the confidence that maximises
the class-mean F1 (Ultralytics convention).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10)


def box_iou_np(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)))
    lt = np.maximum(a[:, None, :2], b[None, :, :2])
    rb = np.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = np.clip(rb - lt, 0, None)
    inter = wh[..., 0] * wh[..., 1]
    area_a = np.prod(np.clip(a[:, 2:] - a[:, :2], 0, None), 1)
    area_b = np.prod(np.clip(b[:, 2:] - b[:, :2], 0, None), 1)
    return inter / np.maximum(area_a[:, None] + area_b[None] - inter, 1e-9)


def match_predictions(pred_boxes, pred_scores, pred_labels, gt_boxes, gt_labels, iouv=IOU_THRESHOLDS):
    """tp [n_pred, n_thr] (bool) for one image."""
    n = len(pred_boxes)
    tp = np.zeros((n, len(iouv)), dtype=bool)
    if n == 0 or len(gt_boxes) == 0:
        return tp
    iou = box_iou_np(pred_boxes, gt_boxes)
    same = pred_labels[:, None] == gt_labels[None, :]
    order = np.argsort(-pred_scores, kind="stable")
    for ti, thr in enumerate(iouv):
        taken = np.zeros(len(gt_boxes), dtype=bool)
        for i in order:
            cand = np.where(same[i] & ~taken & (iou[i] >= thr))[0]
            if len(cand):
                j = cand[np.argmax(iou[i, cand])]
                taken[j] = True
                tp[i, ti] = True
    return tp


MAX_BANDS = 8
# pedestrian height bands in source-frame pixels, [lo, hi): Caltech / CityPersons style far / medium / near
DEFAULT_SIZE_BANDS = (("far", 0.0, 40.0), ("medium", 40.0, 100.0), ("near", 100.0, float("inf")))


def check_bands(bands) -> np.ndarray:
    """bands: R pairs (lo, hi) of box heights, lo inclusive, hi exclusive (inf
    allowed) -> float64 [R, 2].  Requires 1 <= R <= MAX_BANDS, 0 <= lo < hi."""
    try:
        b = np.asarray(bands, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"bands: expected pairs (lo, hi), got {bands!r}") from e
    if b.ndim != 2 or b.shape[1] != 2 or not 1 <= len(b) <= MAX_BANDS:
        raise ValueError(f"bands: expected 1..{MAX_BANDS} pairs (lo, hi), got shape {b.shape}")
    if not (np.isfinite(b[:, 0]) & (b[:, 0] >= 0) & (b[:, 0] < b[:, 1])).all():  # a NaN edge fails a comparison
        raise ValueError(f"bands: every pair needs 0 <= lo < hi (hi may be inf), got {b.tolist()}")
    return np.ascontiguousarray(b)


def named_bands(size_bands=None):
    """size_bands: None (DEFAULT_SIZE_BANDS) or a sequence of (name, lo, hi),
    hi None or inf for an open band -> (names, float64 [R, 2])."""
    rows = DEFAULT_SIZE_BANDS if size_bands is None else list(size_bands)
    names, pairs = [], []
    for row in rows:
        if isinstance(row, (str, bytes)) or not hasattr(row, "__len__") or len(row) != 3:
            raise ValueError(f"size_bands: expected (name, lo, hi) triples, got {row!r}")
        name, lo, hi = row
        names.append(str(name))
        pairs.append((lo, float("inf") if hi is None else hi))
    if len(set(names)) != len(names) or "all" in names:
        raise ValueError(f"size_bands: names must be unique and not 'all', got {names}")
    return names, check_bands(pairs)


def _in_band(heights: np.ndarray, bands: np.ndarray) -> np.ndarray:
    """bool [R, n]: lo <= height < hi (a NaN or negative height is in no band)."""
    return (heights[None, :] >= bands[:, :1]) & (heights[None, :] < bands[:, 1:])


def band_heights(pred_boxes, gt_boxes, scale=1.0):
    """(prediction heights, truth heights) float64 in source pixels: the truth
    height in float64, the prediction height in the dtype of its array (float32
    from the postprocessor), then widened, each times ``scale``."""
    scale = np.float64(scale)
    pb = np.asarray(pred_boxes).reshape(-1, 4)
    gb = np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4)
    return (pb[:, 3] - pb[:, 1]).astype(np.float64) * scale, (gb[:, 3] - gb[:, 1]) * scale


def match_predictions_banded(pred_boxes, pred_scores, pred_labels, gt_boxes, gt_labels, bands, scale=1.0,
                             iouv=IOU_THRESHOLDS):
    """code uint8 [R, n_pred, n_thr] for one image: 0 false positive, 1 true
    positive, 2 ignored.  Per band (``check_bands``; heights in source pixels,
    ``scale`` source pixels per evaluated pixel) the truths outside the band
    are ignore regions: visiting predictions as match_predictions does, with a
    fresh taken set per band and threshold, a prediction takes among the
    untaken same-label truths with iou >= thr the best in-band one (code 1),
    else the best out-of-band one (code 2); with no candidate it is a false
    positive if its own height is in the band and ignored otherwise."""
    bands = check_bands(bands)
    n = len(pred_boxes)
    code = np.zeros((len(bands), n, len(iouv)), dtype=np.uint8)
    if n == 0:
        return code
    ph, gh = band_heights(pred_boxes, gt_boxes, scale)
    code[:] = np.where(_in_band(ph, bands), 0, 2).astype(np.uint8)[:, :, None]
    if len(gt_boxes) == 0:
        return code
    g_in = _in_band(gh, bands)
    iou = box_iou_np(pred_boxes, gt_boxes)
    same = pred_labels[:, None] == gt_labels[None, :]
    order = np.argsort(-pred_scores, kind="stable")
    for r in range(len(bands)):
        for ti, thr in enumerate(iouv):
            taken = np.zeros(len(gt_boxes), dtype=bool)
            for i in order:
                ok = same[i] & ~taken & (iou[i] >= thr)
                for c, cand in ((1, np.where(ok & g_in[r])[0]), (2, np.where(ok & ~g_in[r])[0])):
                    if len(cand):
                        taken[cand[np.argmax(iou[i, cand])]] = True
                        code[r, i, ti] = c
                        break
    return code


def log_average_miss_rate(code, conf, targets: int, images: int):
    """MR^-2 of one threshold column: code [N] (0 FP, 1 TP, 2 ignored) and conf
    [N] over the whole split.  The kept rows by descending score give fppi =
    cumFP / images and mr = 1 - cumTP / targets; mr is sampled at the nine
    np.logspace(-2, 0, 9) fppi references (the last row with fppi <= ref, 1.0
    when there is none) and averaged in the log domain.  None without targets."""
    if targets <= 0 or images <= 0:
        return None
    code, conf = np.asarray(code), np.asarray(conf)
    keep = code != 2
    code = code[keep][np.argsort(-conf[keep], kind="stable")]
    fppi = np.cumsum(code == 0) / images
    mr = 1.0 - np.cumsum(code == 1) / targets
    idx = np.searchsorted(fppi, np.logspace(-2, 0, 9), side="right") - 1
    sampled = np.where(idx >= 0, mr[np.maximum(idx, 0)], 1.0) if len(mr) else np.ones(9)
    return float(np.exp(np.mean(np.log(np.maximum(sampled, 1e-10)))))


def size_band_metrics(code, conf, pred_cls, target_cls, images: int, eps=1e-16) -> dict:
    """One row of the size report: code [N, n_thr] (0 / 1 / 2), conf and
    pred_cls [N] over the split, target_cls the in-band truth labels.  Column j
    drops its own ignored rows, then AP is ap_per_class's: the 101-point _ap per
    class with the in-band truth count as the denominator, averaged over the
    classes that have in-band truths.  recall: the class mean of the highest
    recall reached at column 0."""
    n_t = int(len(target_cls))
    if n_t == 0:
        return {"targets": 0, "AP50": None, "AP50-95": None, "recall": None, "LAMR": None}
    order = np.argsort(-conf, kind="stable")
    code, conf, pred_cls = code[order], conf[order], pred_cls[order]
    classes = np.unique(target_cls)
    ap = np.zeros((len(classes), code.shape[1]))
    rec = np.zeros(len(classes))
    for ci, c in enumerate(classes):
        n_l = int((target_cls == c).sum())
        for j in range(code.shape[1]):
            col = code[(pred_cls == c) & (code[:, j] != 2), j]
            if len(col) == 0:
                continue
            tpc = (col == 1).cumsum()
            fpc = (col == 0).cumsum()
            recall = tpc / (n_l + eps)
            ap[ci, j] = _ap(recall, tpc / (tpc + fpc))
            if j == 0:
                rec[ci] = recall[-1]
    return {"targets": n_t, "AP50": float(ap[:, 0].mean()), "AP50-95": float(ap.mean()), "recall": float(rec.mean()),
            "LAMR": log_average_miss_rate(code[:, 0], conf, n_t, images)}


def gt_xyxy_pixels(gt_cxcywh: np.ndarray, W, H) -> np.ndarray:
    """Ground truth for the matcher: normalised cxcywh float64 [n, 4] -> xyxy
    pixels float64 [n, 4] of a W x H image.  The one expression both evaluators
    use, so the host and the device path see the same doubles."""
    gt = gt_cxcywh
    if not len(gt):
        return np.zeros((0, 4))
    return np.stack([(gt[:, 0] - gt[:, 2] / 2) * W, (gt[:, 1] - gt[:, 3] / 2) * H,
                     (gt[:, 0] + gt[:, 2] / 2) * W, (gt[:, 1] + gt[:, 3] / 2) * H], 1)


def _ap(recall, precision):
    """COCO 101-point AP: mean over recall thresholds r of the best precision
    at any recall >= r (0 where r is never reached)."""
    if len(recall) == 0:
        return 0.0
    env = np.flip(np.maximum.accumulate(np.flip(precision)))
    rs = np.linspace(0, 1, 101)
    inds = np.searchsorted(recall, rs, side="left")
    q = np.where(inds < len(env), env[np.minimum(inds, len(env) - 1)], 0.0)
    return float(q.mean())


def ap_per_class(tp, conf, pred_cls, target_cls, eps=1e-16):
    """Returns dict(p, r, f1, ap [nc, n_thr], classes, px, curves) over the dataset."""
    order = np.argsort(-conf, kind="stable")
    tp, conf, pred_cls = tp[order], conf[order], pred_cls[order]
    classes = np.unique(target_cls) if len(target_cls) else np.unique(pred_cls)
    nc = len(classes)
    px = np.linspace(0, 1, 1000)
    ap = np.zeros((nc, tp.shape[1]))
    p_curve = np.zeros((nc, 1000))
    r_curve = np.zeros((nc, 1000))
    pr_curve = np.zeros((nc, 1000))
    for ci, c in enumerate(classes):
        sel = pred_cls == c
        n_l = int((target_cls == c).sum())
        n_p = int(sel.sum())
        if n_p == 0 or n_l == 0:
            continue
        fpc = (1 - tp[sel]).cumsum(0)
        tpc = tp[sel].cumsum(0)
        recall = tpc / (n_l + eps)
        precision = tpc / (tpc + fpc)
        r_curve[ci] = np.interp(-px, -conf[sel], recall[:, 0], left=0)
        p_curve[ci] = np.interp(-px, -conf[sel], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            ap[ci, j] = _ap(recall[:, j], precision[:, j])
        # PR curve at IoU 0.5 on the recall grid
        mrec = np.concatenate([[0.0], recall[:, 0], [1.0]])
        mpre = np.flip(np.maximum.accumulate(np.flip(np.concatenate([[1.0], precision[:, 0], [0.0]]))))
        pr_curve[ci] = np.interp(px, mrec, mpre)
    f1 = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    i = int(np.argmax(f1.mean(0))) if nc else 0
    return dict(p=p_curve[:, i], r=r_curve[:, i], f1=f1[:, i], ap=ap, classes=classes, px=px,
                p_curve=p_curve, r_curve=r_curve, f1_curve=f1, pr_curve=pr_curve)


@dataclass
class BoxMetrics:
    """Mirror of the attributes the reference reads from ``metrics.box``."""
    mp: float = 0.0
    mr: float = 0.0
    map50: float = 0.0
    map: float = 0.0
    curves: list = field(default_factory=lambda: ["Precision-Recall(B)", "F1-Confidence(B)",
                                                  "Precision-Confidence(B)", "Recall-Confidence(B)"])
    curves_results: list = field(default_factory=list)


class DetectionEvaluator:
    """Accumulates per-image matches, then reduces to dataset metrics."""

    def __init__(self):
        self.tp, self.conf, self.pred_cls, self.target_cls = [], [], [], []
        self.image_ctx = []  # per image: its context id, or None when the update gave none
        # the size report (updates that carried bands): per image the codes uint8 [R, n_kept, n_thr]
        # and, per band, the labels of the in-band truths; the band table of those updates
        self.codes, self.band_target_cls, self.bands = [], [], None

    def update(self, pred_boxes, pred_scores, pred_labels, gt_boxes, gt_labels, conf_thres=0.001, *, ctx=None,
               bands=None, scale=1.0):
        """ctx: the image's context id (moe.context), for compute_by_context().
        bands, scale: the height bands (``check_bands``) and this image's source
        pixels per evaluated pixel, for compute_by_size(); None appends nothing
        for the size report."""
        if bands is not None:
            bands = self._use_bands(bands)
        keep = pred_scores >= conf_thres
        pb, ps, pl = pred_boxes[keep], pred_scores[keep], pred_labels[keep]
        self.tp.append(match_predictions(pb, ps, pl, gt_boxes, gt_labels))
        self.conf.append(ps)
        self.pred_cls.append(pl)
        self.target_cls.append(gt_labels)
        self.image_ctx.append(None if ctx is None else int(ctx))
        if bands is not None:
            self._append_size(match_predictions_banded(pb, ps, pl, gt_boxes, gt_labels, bands, scale), gt_boxes,
                              gt_labels, bands, scale)

    def _use_bands(self, bands) -> np.ndarray:
        bands = check_bands(bands)
        if self.bands is None:
            self.bands = bands
        elif not np.array_equal(self.bands, bands):
            raise ValueError("update: the bands differ from those of an earlier update")
        return bands

    def _append_size(self, code, gt_boxes, gt_labels, bands, scale):
        gt_labels = np.asarray(gt_labels)
        g_in = _in_band(band_heights(np.zeros((0, 4)), gt_boxes, scale)[1], bands)
        self.codes.append(code)
        self.band_target_cls.append([gt_labels[g_in[r]] for r in range(len(bands))])

    def compute_by_size(self, names) -> dict:
        """{band name: {"targets", "AP50", "AP50-95", "recall", "LAMR"}} per band
        of the updates' band table (``size_band_metrics``; None metrics for a
        band without in-band truths), plus "all": the unstratified row from
        ``tp`` -- AP from compute(), recall the class mean of the highest
        recall at IoU 0.5 (compute()'s recall-confidence curve at confidence
        0), LAMR from the same function fed tp.  Needs every update to have
        carried ``bands``."""
        if self.bands is None or len(self.codes) != len(self.tp):
            raise ValueError("compute_by_size: an update carried no bands (bands=...)")
        names = [str(n) for n in names]
        if len(names) != len(self.bands) or len(set(names)) != len(names) or "all" in names:
            raise ValueError(f"compute_by_size: need {len(self.bands)} unique band names other than 'all'")
        images, T = len(self.tp), len(IOU_THRESHOLDS)
        cat = lambda xs, d: np.concatenate(xs, 0) if xs else np.zeros((0,) + d)  # noqa: E731
        conf, pred_cls = cat(self.conf, ()), cat(self.pred_cls, ())
        out = {}
        for r, name in enumerate(names):
            out[name] = size_band_metrics(cat([c[r] for c in self.codes], (T,)), conf, pred_cls,
                                          cat([t[r] for t in self.band_target_cls], ()), images)
        n_t = int(sum(len(t) for t in self.target_cls))
        row = {"targets": n_t, "AP50": None, "AP50-95": None, "recall": None, "LAMR": None}
        if n_t:
            box = self.compute()
            tp0 = cat(self.tp, (T,))[:, 0].astype(np.uint8)
            row.update({"AP50": box.map50, "AP50-95": box.map,
                        "recall": float(box.curves_results[3][1][:, 0].mean()),
                        "LAMR": log_average_miss_rate(tp0, conf, n_t, images)})
        out["all"] = row
        return out

    def average_recall(self, max_det: int = 100) -> float:
        """COCO AR@max_det (all classes, area "all"): per image the max_det
        highest-scoring detections, recall at each IoU threshold of
        IOU_THRESHOLDS, averaged over thresholds (and classes present)."""
        n_gt = {}
        for tc in self.target_cls:
            for c in np.asarray(tc).reshape(-1).tolist():
                n_gt[int(c)] = n_gt.get(int(c), 0) + 1
        if not n_gt:
            return -1.0
        hits = {c: np.zeros(len(IOU_THRESHOLDS)) for c in n_gt}
        for tp, conf, pc in zip(self.tp, self.conf, self.pred_cls):
            order = np.argsort(-np.asarray(conf), kind="stable")[:max_det]
            for j in order:
                c = int(pc[j])
                if c in hits:
                    hits[c] += np.asarray(tp[j], dtype=np.float64)
        return float(np.mean([(hits[c] / n_gt[c]).mean() for c in n_gt]))

    def compute(self) -> BoxMetrics:
        return self._reduce(self.tp, self.conf, self.pred_cls, self.target_cls)

    def compute_by_context(self, labels=None) -> dict:
        """{context label: {"images", "targets", "box": BoxMetrics}} for every
        context with at least one image: compute()'s reduction over that
        context's images only, so each entry equals what a fresh evaluator fed
        just those images returns.  labels: names by context id (default
        moe.context.CONTEXT_LABELS; an id past them is named by its number).
        Needs every update to have carried ``ctx``."""
        if labels is None:
            from ..moe.context import CONTEXT_LABELS as labels
        if len(self.image_ctx) != len(self.tp) or any(c is None for c in self.image_ctx):
            raise ValueError("compute_by_context: an update carried no context id (ctx=...)")
        out = {}
        for c in sorted(set(self.image_ctx)):
            rows = [i for i, ci in enumerate(self.image_ctx) if ci == c]
            pick = lambda xs: [xs[i] for i in rows]  # noqa: E731
            tc = pick(self.target_cls)
            out[labels[c] if 0 <= c < len(labels) else str(c)] = {
                "images": len(rows), "targets": int(sum(len(t) for t in tc)),
                "box": self._reduce(pick(self.tp), pick(self.conf), pick(self.pred_cls), tc)}
        return out

    @staticmethod
    def _reduce(tps, confs, pred_clss, target_clss) -> BoxMetrics:
        cat = lambda xs, d: np.concatenate(xs, 0) if xs else np.zeros((0,) + d)  # noqa: E731
        tp = cat(tps, (len(IOU_THRESHOLDS),))
        conf = cat(confs, ())
        pred_cls = cat(pred_clss, ())
        target_cls = cat(target_clss, ())
        box = BoxMetrics()
        if len(target_cls) == 0:
            return box
        if len(conf) == 0:
            px = np.linspace(0, 1, 1000)
            zero = np.zeros((1, 1000))
            box.curves_results = [[px, zero, "Recall", "Precision"], [px, zero, "Confidence", "F1"],
                                  [px, zero, "Confidence", "Precision"], [px, zero, "Confidence", "Recall"]]
            return box
        r = ap_per_class(tp.astype(np.float64), conf, pred_cls, target_cls)
        box.mp = float(r["p"].mean())
        box.mr = float(r["r"].mean())
        box.map50 = float(r["ap"][:, 0].mean())
        box.map = float(r["ap"].mean())
        box.curves_results = [[r["px"], r["pr_curve"], "Recall", "Precision"],
                              [r["px"], r["f1_curve"], "Confidence", "F1"],
                              [r["px"], r["p_curve"], "Confidence", "Precision"],
                              [r["px"], r["r_curve"], "Confidence", "Recall"]]
        return box


class DeviceDetectionEvaluator(DetectionEvaluator):
    """DetectionEvaluator whose per-image matching runs on the GPU, a batch per
    launch (``rtdetr_eval_match``: match_predictions and box_iou_np restated bit
    for bit, numpy's dtypes included).  ``update_batch`` appends to ``tp / conf /
    pred_cls / target_cls`` exactly what ``update`` would have appended for each
    image, so ``compute()`` and ``average_recall()`` -- inherited -- return the
    same floats.

    The kernel matches all K predictions and the rows below ``conf_thres`` are
    dropped afterwards.  That equals dropping them first, as ``update`` does:
    they sort strictly after every kept row, so no kept row ever sees a truth
    they took.  The same holds per band for the codes of the size report
    (``update_batch(bands=...)``, ``rtdetr_eval_match_bands``:
    match_predictions_banded restated bit for bit).

    The host path (``update`` per image, no error) runs instead when the inputs
    are on the CPU, when ``MOE_EVAL_MATCH=0`` (read per call), or when K, the
    batch's largest truth count or the number of thresholds exceeds the
    kernel's limits.  NaN scores and non-finite boxes are outside the contract;
    labels must fit int32.
    """

    def __init__(self):
        super().__init__()
        self._thr = {}  # device -> IOU_THRESHOLDS uploaded once

    def _device_path(self, boxes, K, max_gt) -> bool:
        import os

        if not boxes.is_cuda or os.environ.get("MOE_EVAL_MATCH", "1") == "0":
            return False
        from ..moe import _lib as L

        return (1 <= K <= L.EVAL_MATCH_MAX_K and max_gt <= L.EVAL_MATCH_MAX_M
                and 1 <= len(IOU_THRESHOLDS) <= L.EVAL_MATCH_MAX_T)

    def update_batch(self, boxes, scores, labels, targets, conf_thres=0.001, *, size, ctx=None, bands=None,
                     scales=None):
        """boxes [B, K, 4] xyxy pixels, scores [B, K], labels [B, K]: the stacked
        tensors of the postprocessor (``RTDETRMoE.postprocess_batched``).
        targets: per image a dict with ``boxes`` (normalised cxcywh [n, 4]) and
        ``labels`` [n] on the CPU, as the loader yields them.  size: (W, H), the
        pixel size the predictions are scaled to.  ctx: the batch's context ids
        (a host sequence of B ints), for compute_by_context().  bands: the
        height bands of the size report (``check_bands``), with scales: per
        image its source pixels per evaluated pixel (default 1.0), for
        compute_by_size().

        Device path: one host-to-device copy (the padded truth), one launch and
        one device-to-host copy (tp, scores and labels packed) per batch.  With
        bands the scale and band tables ride in the same upload, the codes come
        from one more launch (``rtdetr_eval_match_bands``) and join the same
        copy back."""
        import torch

        W, H = size
        if bands is not None:
            bands = self._use_bands(bands)
            scales = np.ones(len(targets)) if scales is None else np.asarray(scales, dtype=np.float64).reshape(-1)
            if len(scales) != len(targets):
                raise ValueError(f"update_batch: {len(targets)} targets, {len(scales)} scales")
        B, K = int(scores.shape[0]), int(scores.shape[1])
        gts = [(gt_xyxy_pixels(np.asarray(t["boxes"]).astype(np.float64), W, H), np.asarray(t["labels"]))
               for t in targets]
        if len(gts) != B:
            raise ValueError(f"update_batch: {B} images of predictions, {len(gts)} targets")
        ctx = [None] * B if ctx is None else [int(c) for c in ctx]
        if len(ctx) != B:
            raise ValueError(f"update_batch: {B} images of predictions, {len(ctx)} context ids")
        max_gt = max((len(g) for g, _ in gts), default=0)
        boxes, scores = boxes.float(), scores.float()
        if B == 0 or not self._device_path(boxes, K, max_gt):
            for b, (g, gl) in enumerate(gts):
                self.update(boxes[b].cpu().numpy(), scores[b].cpu().numpy(), labels[b].cpu().numpy(), g, gl,
                            conf_thres, ctx=ctx[b], bands=bands, scale=1.0 if bands is None else scales[b])
            return
        from ..moe import _lib as L

        dev = boxes.device
        thr = self._thr.get(dev)
        if thr is None:
            thr = self._thr[dev] = torch.from_numpy(np.ascontiguousarray(IOU_THRESHOLDS, dtype=np.float64)).to(dev)
        # the padded truth in one host buffer: fp64 boxes | int32 labels | int32 counts
        # (with bands: fp64 boxes | fp64 scales [B] | fp64 bands [R, 2] | int32 labels | int32 counts)
        M = max(max_gt, 1)
        R = 0 if bands is None else len(bands)
        nb, nl = B * M * 32, B * M * 4
        ns = 0 if bands is None else (B + 2 * R) * 8
        host = np.zeros(nb + ns + nl + B * 4, dtype=np.uint8)
        gb = host[:nb].view(np.float64).reshape(B, M, 4)
        gl32 = host[nb + ns:nb + ns + nl].view(np.int32).reshape(B, M)
        nv = host[nb + ns + nl:].view(np.int32)
        for b, (g, gl) in enumerate(gts):
            gb[b, :len(g)] = g
            gl32[b, :len(g)] = gl
            nv[b] = len(g)
        if bands is not None:
            host[nb:nb + B * 8].view(np.float64)[:] = scales
            host[nb + B * 8:nb + ns].view(np.float64)[:] = bands.reshape(-1)
        d = torch.from_numpy(host).to(dev)
        lab32 = labels.to(torch.int32).contiguous()
        scores = scores.contiguous()
        boxes = boxes.contiguous()
        d_gb = d[:nb].view(torch.float64).view(B, M, 4)
        d_gl = d[nb + ns:nb + ns + nl].view(torch.int32).view(B, M)
        d_nv = d[nb + ns + nl:].view(torch.int32)
        tp = L.eval_match(boxes, scores, lab32, d_gb, d_gl, d_nv, thr)
        T = int(tp.shape[2])
        parts = [scores.view(torch.uint8).view(B, K * 4), lab32.view(torch.uint8).view(B, K * 4), tp.view(B, K * T)]
        if bands is not None:
            code = L.eval_match_bands(boxes, scores, lab32, d_gb, d_gl, d_nv, thr,
                                      d[nb:nb + B * 8].view(torch.float64),
                                      d[nb + B * 8:nb + ns].view(torch.float64).view(R, 2))
            parts.append(code.view(B, R * K * T))
        packed = torch.cat(parts, 1).cpu().numpy()
        sc = np.ascontiguousarray(packed[:, :4 * K]).view(np.float32)
        label_dtype = torch.empty(0, dtype=labels.dtype).numpy().dtype  # pred_cls keeps the dtype update() appends
        lb = np.ascontiguousarray(packed[:, 4 * K:8 * K]).view(np.int32).astype(label_dtype)
        tpn = packed[:, 8 * K:8 * K + K * T].reshape(B, K, T).astype(bool)
        for b, (g, gl) in enumerate(gts):
            keep = sc[b] >= conf_thres
            self.tp.append(tpn[b][keep])
            self.conf.append(sc[b][keep])
            self.pred_cls.append(lb[b][keep])
            self.target_cls.append(gl)
            self.image_ctx.append(ctx[b])
            if bands is not None:
                cb = packed[b, 8 * K + K * T:].reshape(R, K, T)
                self._append_size(np.ascontiguousarray(cb[:, keep]), g, gl, bands, scales[b])
