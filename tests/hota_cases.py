"""Shared support of the HOTA tests (hota.py's reference on the CPU, the
rtdetr_hota_* kernels on the GPU): a plain fp64 transcription of the published
HOTA algorithm (Luiten et al., IJCV 2021, as TrackEval's HOTA.eval_sequence
states it: a running float sum for the potential matches, an fp64 score, the
assignment on the [truths, rows] matrix), comparison helpers, and cached
reference results.  Not a test."""
from __future__ import annotations

import functools

import numpy as np

import mot_eval_cases as mc

EPS = np.finfo("float").eps
ALPHAS = np.arange(0.05, 0.99, 0.05)

# (F, NG, NT, shown truths, shown rows, ignore share, tie share): the shapes the rule is compared at, seeds 0..39
TRANSCRIPTION_SHAPES = ((30, 12, 16, (4, 12), (4, 16), 0.1, 0.0),
                        (12, 40, 70, (20, 40), (30, 65), 0.05, 0.0),
                        (20, 6, 9, (0, 6), (0, 9), 0.2, 0.3))


def transcription(frames, NG, NT, thr=0.5):
    """TrackEval's HOTA.eval_sequence on the frames after moteval's steps 1-2 (hota.frame_rows).  -> {"TP", "FN",
    "FP" int [19], "mc" [19, NG, NT], "HOTA", "DetA", "AssA", "LocA" (means over the thresholds)}."""
    from scipy.optimize import linear_sum_assignment

    from src.rtdetr_moe.hota import frame_rows

    rows = []
    for gb, gi, gf, tb, ti in frames:
        g, t, iou, _ = frame_rows((gb, gi, gf), (tb, ti), NG, NT, thr)
        rows.append((g, t, np.ascontiguousarray(iou.T).astype(np.float64)))  # similarity [truths, rows]
    potential = np.zeros((NG, NT))
    gt_id_count, tracker_id_count = np.zeros((NG, 1)), np.zeros((1, NT))
    for g, t, sim in rows:
        denom = sim.sum(0)[np.newaxis, :] + sim.sum(1)[:, np.newaxis] - sim
        sim_iou = np.zeros_like(sim)
        mask = denom > 0 + EPS
        sim_iou[mask] = sim[mask] / denom[mask]
        potential[g[:, np.newaxis], t[np.newaxis, :]] += sim_iou
        gt_id_count[g] += 1
        tracker_id_count[0, t] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        gas = potential / (gt_id_count + tracker_id_count - potential)
    n = len(ALPHAS)
    tp, fn, fp, loc = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    counts = [np.zeros((NG, NT)) for _ in ALPHAS]
    for g, t, sim in rows:
        if len(g) == 0:
            fp += len(t)
            continue
        if len(t) == 0:
            fn += len(g)
            continue
        score = gas[g[:, np.newaxis], t[np.newaxis, :]] * sim
        match_rows, match_cols = linear_sum_assignment(-score)
        for a, alpha in enumerate(ALPHAS):
            ok = sim[match_rows, match_cols] >= alpha - EPS
            r, c = match_rows[ok], match_cols[ok]
            tp[a] += len(r)
            fn[a] += len(g) - len(r)
            fp[a] += len(t) - len(r)
            if len(r) > 0:
                loc[a] += sum(sim[r, c])
                counts[a][g[r], t[c]] += 1
    ass_a = np.zeros(n)
    for a in range(n):
        m = counts[a]
        ass_a[a] = np.sum(m * (m / np.maximum(1, gt_id_count + tracker_id_count - m))) / np.maximum(1, tp[a])
    det_a = tp / np.maximum(1, tp + fn + fp)
    loc_a = np.maximum(1e-10, loc) / np.maximum(1e-10, tp)
    return {"TP": tp.astype(np.int64), "FN": fn.astype(np.int64), "FP": fp.astype(np.int64),
            "mc": np.stack(counts).astype(np.int64), "HOTA": float(np.mean(np.sqrt(det_a * ass_a))),
            "DetA": float(np.mean(det_a)), "AssA": float(np.mean(ass_a)), "LocA": float(np.mean(loc_a))}


def assert_same(got, ref, keys=None):
    """Every array of a HOTA state equal, no tolerance: floating point compared as integer views."""
    from src.rtdetr_moe.hota import HOTA_ARRAYS

    for key in keys or (*HOTA_ARRAYS, "gas", "loc_part"):
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(ref[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (key, a.dtype, b.dtype, a.shape, b.shape)
        if a.dtype == np.float64:
            a, b = a.view(np.int64), b.view(np.int64)
        elif a.dtype == np.float32:
            a, b = a.view(np.int32), b.view(np.int32)
        assert np.array_equal(a, b), (key, np.argwhere(a != b)[:8].tolist())


@functools.lru_cache(maxsize=None)
def drawn(seed, F, NG, NT, m, k, ignore=0.0, tie=0.0):
    """(frames, hota_reference's state) of mot_eval_cases.draw_frames, computed once per shape."""
    from src.rtdetr_moe.hota import hota_reference

    frames = mc.draw_frames(seed, F, NG, NT, m, k, ignore=ignore, tie=tie)
    return frames, hota_reference(frames, NG, NT)


def mot_files(frames, gid=lambda g: 10 + 3 * int(g), tid=lambda t: 5 + 2 * int(t)):
    """draw_frames' frames as MOTChallenge (ground-truth text with class 8 for the ignore regions, result text)."""
    rows_g, rows_t = [], []
    for f, (gb, gi, gf, tb, ti) in enumerate(frames, 1):
        rows_g += [(f, gid(g), *np.round(b, 2).tolist(), 1, 1 if fl else 8, 1) for b, g, fl in zip(gb, gi, gf)]
        rows_t += [(f, tid(t), *np.round(b, 2).tolist(), 0.9, -1, -1, -1) for b, t in zip(tb, ti)]
    return mc.mot_text(rows_g), mc.mot_text(rows_t)
