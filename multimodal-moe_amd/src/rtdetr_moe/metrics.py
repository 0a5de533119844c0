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

    def update(self, pred_boxes, pred_scores, pred_labels, gt_boxes, gt_labels, conf_thres=0.001, *, ctx=None):
        """ctx: the image's context id (moe.context), for compute_by_context()."""
        keep = pred_scores >= conf_thres
        pb, ps, pl = pred_boxes[keep], pred_scores[keep], pred_labels[keep]
        self.tp.append(match_predictions(pb, ps, pl, gt_boxes, gt_labels))
        self.conf.append(ps)
        self.pred_cls.append(pl)
        self.target_cls.append(gt_labels)
        self.image_ctx.append(None if ctx is None else int(ctx))

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
    they took.

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

    def update_batch(self, boxes, scores, labels, targets, conf_thres=0.001, *, size, ctx=None):
        """boxes [B, K, 4] xyxy pixels, scores [B, K], labels [B, K]: the stacked
        tensors of the postprocessor (``RTDETRMoE.postprocess_batched``).
        targets: per image a dict with ``boxes`` (normalised cxcywh [n, 4]) and
        ``labels`` [n] on the CPU, as the loader yields them.  size: (W, H), the
        pixel size the predictions are scaled to.  ctx: the batch's context ids
        (a host sequence of B ints), for compute_by_context().

        Device path: one host-to-device copy (the padded truth), one launch and
        one device-to-host copy (tp, scores and labels packed) per batch."""
        import torch

        W, H = size
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
                            conf_thres, ctx=ctx[b])
            return
        from ..moe import _lib as L

        dev = boxes.device
        thr = self._thr.get(dev)
        if thr is None:
            thr = self._thr[dev] = torch.from_numpy(np.ascontiguousarray(IOU_THRESHOLDS, dtype=np.float64)).to(dev)
        # the padded truth in one host buffer: fp64 boxes | int32 labels | int32 counts
        M = max(max_gt, 1)
        nb, nl = B * M * 32, B * M * 4
        host = np.zeros(nb + nl + B * 4, dtype=np.uint8)
        gb = host[:nb].view(np.float64).reshape(B, M, 4)
        gl32 = host[nb:nb + nl].view(np.int32).reshape(B, M)
        nv = host[nb + nl:].view(np.int32)
        for b, (g, gl) in enumerate(gts):
            gb[b, :len(g)] = g
            gl32[b, :len(g)] = gl
            nv[b] = len(g)
        d = torch.from_numpy(host).to(dev)
        lab32 = labels.to(torch.int32).contiguous()
        scores = scores.contiguous()
        tp = L.eval_match(boxes.contiguous(), scores, lab32, d[:nb].view(torch.float64).view(B, M, 4),
                          d[nb:nb + nl].view(torch.int32).view(B, M), d[nb + nl:].view(torch.int32), thr)
        T = int(tp.shape[2])
        packed = torch.cat([scores.view(torch.uint8).view(B, K * 4), lab32.view(torch.uint8).view(B, K * 4),
                            tp.view(B, K * T)], 1).cpu().numpy()
        sc = np.ascontiguousarray(packed[:, :4 * K]).view(np.float32)
        label_dtype = torch.empty(0, dtype=labels.dtype).numpy().dtype  # pred_cls keeps the dtype update() appends
        lb = np.ascontiguousarray(packed[:, 4 * K:8 * K]).view(np.int32).astype(label_dtype)
        tpn = packed[:, 8 * K:].reshape(B, K, T).astype(bool)
        for b, (_, gl) in enumerate(gts):
            keep = sc[b] >= conf_thres
            self.tp.append(tpn[b][keep])
            self.conf.append(sc[b][keep])
            self.pred_cls.append(lb[b][keep])
            self.target_cls.append(gl)
            self.image_ctx.append(ctx[b])
