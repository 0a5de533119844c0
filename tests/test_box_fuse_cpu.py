"""Box fusion on the host: merge.fuse_reference against hand-worked answers,
against merge_reference's kept set, against a float64 restatement of its
averages and on the synthetic localisation study; engine.predict(device="cpu",
tiles=..., merge="fuse") against the same pipeline built by hand."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest
import torch

from box_fuse_cases import FRAME_H, FRAME_W, cut_sides, draw, draw_batch, hand_cases, reference_batch, run_hand_case

ROOT = Path(__file__).resolve().parents[1]
FRAMES = ROOT / "tests" / "golden" / "zod_mini" / "frames"
SPEC = "rtdetr-r18-moe4-top1"
IMGSZ = (320, 640)


def _host(boxes, scores, labels, windows, conf, thr, metric, max_det, agnostic, fuse_thr):
    from src.rtdetr_moe.merge import fuse_reference

    kept, fused, members = fuse_reference(boxes[0], scores[0], labels[0], None, conf, thr, metric, max_det, agnostic,
                                          fuse_thr, None if windows is None else windows[0])
    assert kept.dtype == np.int64 and fused.dtype == np.float32 and members.dtype == np.int32
    assert fused.shape == (len(kept), 4) and members.shape == (len(kept),)
    return kept.tolist(), torch.from_numpy(fused).reshape(-1, 4), members.tolist()


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c["name"].replace(" ", "_"))
def test_hand_worked_answers(case):
    run_hand_case(case, _host)


def test_kept_indices_are_merge_references():
    from src.rtdetr_moe.merge import fuse_reference, merge_reference

    for P, k, max_det, metric, agnostic, conf in ((5, 26, 300, "ios", False, 0.0), (5, 52, 100, "iou", True, 0.25),
                                                  (3, 43, 7, "ios", False, 0.0), (5, 300, 300, "ios", False, 0.25)):
        boxes, scores, labels, windows = draw_batch(2, P, k, seed=P * k + max_det)
        for b, nv in enumerate((None, P * k // 2)):
            want = merge_reference(boxes[b], scores[b], labels[b], nv, conf, 0.5, metric, max_det, agnostic)
            kept, fused, members = fuse_reference(boxes[b], scores[b], labels[b], nv, conf, 0.5, metric, max_det,
                                                  agnostic, 0.55, windows[b])
            assert kept.tolist() == want.tolist() and len(kept) >= 2
            assert bool((members >= 1).all()) and (max_det == 7 or int(members.max()) >= 2)
            # inside the frame and ordered
            assert bool((fused[:, [0, 1]] >= 0).all() and (fused[:, 2] <= FRAME_W).all())
            assert bool((fused[:, 3] <= FRAME_H).all())
            assert bool((fused[:, 0] <= fused[:, 2]).all() and (fused[:, 1] <= fused[:, 3]).all())
    # no windows: N need not be a multiple of anything
    boxes, scores, labels, _ = draw_batch(1, 5, 13, seed=3)
    kept, _, members = fuse_reference(boxes[0, :61], scores[0, :61], labels[0, :61], None, 0.0, 0.5)
    assert kept.tolist() == merge_reference(boxes[0, :61], scores[0, :61], labels[0, :61], None, 0.0, 0.5).tolist()
    with pytest.raises(ValueError):  # 61 % 5
        fuse_reference(boxes[0, :61], scores[0, :61], labels[0, :61], None, 0.0, 0.5, windows=np.zeros((5, 4)))
    with pytest.raises(ValueError):
        fuse_reference(boxes[0], scores[0], labels[0], None, 0.0, 0.5, metric="giou")


def test_averages_against_float64():
    """Step 4 restated in float64 on fuse_reference's own clusters.  The bound
    is derived, not picked: a side averages n members with weights s_i > 0 and
    coordinates c_i >= 0.  In fp32 (u = 2^-24) num carries one rounding per
    product and n - 1 per running sum, den n - 1, the division one more, so
    fused = exact * (1 + theta) with |theta| <= gamma(2 n) = 2 n u / (1 - 2 n u)
    (Higham, Accuracy and Stability, lemma 3.1 and 3.3).  The clamp to the frame
    only moves both values closer."""
    u = 2.0 ** -24
    checked = worst = 0
    for seed in range(4):
        boxes, scores, labels, windows = draw_batch(1, 5, 120, seed=40 + seed)
        (r,) = reference_batch(boxes, scores, labels, windows, None, 0.0, 0.5, "ios", 300, False, 0.55)
        b64, s64, W = boxes[0].numpy().astype(np.float64), scores[0].numpy().astype(np.float64), windows[0].numpy()
        cut = cut_sides(boxes[0].numpy(), W)
        lo, hi = W[0][[0, 1, 0, 1]].astype(np.float64), W[0][[2, 3, 2, 3]].astype(np.float64)
        for q, lead in enumerate(r["kept"]):
            mem = np.nonzero(r["rank"] == q)[0]
            assert len(mem) == int(r["members"][q])
            exact, bound = b64[lead].copy(), np.zeros(4)
            for side in range(4):
                use = mem[(~cut[mem, side]) & (s64[mem] > 0)]
                if len(use):
                    exact[side] = (s64[use] * b64[use, side]).sum() / s64[use].sum()
                    g = 2 * len(use) * u
                    bound[side] = g / (1 - g) * abs(exact[side])
            exact = np.minimum(np.maximum(exact, lo), hi)
            got = r["fused"][q].numpy().astype(np.float64)
            for a, c in ((0, 2), (1, 3)):
                if exact[a] > exact[c] - (bound[a] + bound[c]):  # unordered, or too close to call in fp32
                    continue
                for side in (a, c):
                    assert abs(got[side] - exact[side]) <= bound[side], (seed, q, side, got[side], exact[side])
                    if len(mem) >= 2 and bound[side] > 0:
                        checked += 1
                        worst = max(worst, abs(got[side] - exact[side]) / bound[side])
    print(f"{checked} fused sides of clusters of >= 2 checked, worst error / bound {worst:.3f}")
    assert checked >= 200


def test_fusion_localises_better_than_suppression_on_the_synthetic_study():
    """The study of the rule's draft: 40 pedestrian-shaped objects per frame,
    full-frame copies jittered by 6 % of the height, tile copies by 2 %.  The
    mean worst-side error of the kept boxes against the truth, over the rows
    whose leader copies an object: fused below unfused.  The reference against
    itself on fixed seeds: no margin."""
    from src.rtdetr_moe.merge import fuse_reference

    err_lead, err_fused, rows = [], [], 0
    for seed in range(20):
        boxes, scores, labels, windows, truth, obj = draw(5, 60, 500 + seed, objects=40)
        kept, fused, members = fuse_reference(boxes, scores, labels, None, 0.25, 0.5, "ios", 300, False, 0.55, windows)
        m = obj[kept]
        sel = (m >= 0).numpy()
        t = truth[m[sel]].numpy()
        err_lead.append(np.abs(boxes[kept][sel].numpy() - t).max(1))
        err_fused.append(np.abs(fused[sel] - t).max(1))
        rows += int(sel.sum())
    lead, fus = float(np.concatenate(err_lead).mean()), float(np.concatenate(err_fused).mean())
    print(f"{rows} kept rows: mean worst-side error {lead:.2f} px kept as they stand, {fus:.2f} px fused")
    assert rows >= 20 * 30 and fus < lead


def _hand_candidates(path, model, tiles):
    from PIL import Image

    from src.rtdetr_moe.merge import tile_windows
    from src.rtdetr_moe.preprocess import FrameSource, host_resize, mapped_sizes, padded_hw

    frame = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
    H, W = frame.shape[:2]
    out_hw, pad_hw = padded_hw(IMGSZ)
    ctx = torch.tensor([FrameSource([path]).context_id(path)], dtype=torch.int32)
    cand, wins = [], [(0, 0, W, H)] + tile_windows(W, H, tiles=tiles, overlap=0.2)
    for x0, y0, tw, th in wins:
        x = host_resize(np.ascontiguousarray(frame[y0:y0 + th, x0:x0 + tw]), out_hw, pad_hw)[None]
        with torch.no_grad():
            out = model(x, ctx)
        b, sc, lb = model.postprocess_batched(out, mapped_sizes([(tw, th)], out_hw, pad_hw), num_top=300)
        lo = torch.tensor([x0, y0, x0, y0], dtype=b.dtype)
        hi = torch.tensor([x0 + tw, y0 + th, x0 + tw, y0 + th], dtype=b.dtype)
        cand.append((torch.minimum(torch.maximum(b[0] + lo, lo), hi), sc[0], lb[0]))
    windows = torch.tensor([[x0, y0, x0 + tw, y0 + th] for x0, y0, tw, th in wins], dtype=torch.float32)
    return tuple(torch.cat([c[j] for c in cand]) for j in range(3)) + (windows,)


def test_predict_cpu_fuse_equals_the_pipeline_built_by_hand():
    from src.rtdetr_moe import engine
    from src.rtdetr_moe.merge import fuse_reference

    path = sorted(FRAMES.glob("*.jpg"))[0]
    torch.manual_seed(0)
    res = engine.predict(SPEC, [path], imgsz=IMGSZ, batch=1, device="cpu", conf=0.0, workers=0, tiles=(2, 1),
                         merge="fuse")
    assert res.speed["passes"] == 3
    (p,) = res.predictions
    model = res.model.model
    model.eval()
    cb, cs, cl, windows = _hand_candidates(path, model, (2, 1))
    assert windows.tolist() == [[0, 0, 1248, 704], [0, 0, 1248, 392], [0, 312, 1248, 704]]
    keep, fused, members = fuse_reference(cb, cs, cl, None, 0.0, 0.5, "ios", 300, False, 0.55, windows)
    keep = torch.from_numpy(keep)
    assert 2 <= len(keep) < 900 and int(members.max()) >= 2  # something was fused
    assert torch.equal(p.boxes, torch.from_numpy(fused)) and not torch.equal(p.boxes, cb[keep])
    assert torch.equal(p.scores, cs[keep]) and torch.equal(p.labels, cl[keep]) and torch.equal(p.source, keep // 300)
    assert p.members.dtype == torch.int64 and torch.equal(p.members, torch.from_numpy(members).to(torch.int64))
    assert p.boxes.dtype == torch.float32 and bool((p.scores[:-1] >= p.scores[1:]).all())
    assert bool((p.boxes >= 0).all() and (p.boxes[:, [0, 2]] <= 1248).all() and (p.boxes[:, [1, 3]] <= 704).all())
    # merge="nms" is the call without the argument, and has no members
    torch.manual_seed(0)
    a = engine.predict(SPEC, [path], imgsz=IMGSZ, batch=1, device="cpu", conf=0.0, workers=0, tiles=(2, 1),
                       merge="nms").predictions[0]
    torch.manual_seed(0)
    b = engine.predict(SPEC, [path], imgsz=IMGSZ, batch=1, device="cpu", conf=0.0, workers=0,
                       tiles=(2, 1)).predictions[0]
    assert a.members is None and b.members is None
    assert torch.equal(a.boxes, b.boxes) and torch.equal(a.scores, b.scores) and torch.equal(a.labels, b.labels)
    assert torch.equal(a.source, b.source) and torch.equal(a.boxes, cb[keep]) and torch.equal(a.scores, p.scores)
    # predictions.json keeps its format
    rows = engine.coco_results([p])
    assert len(rows) == len(keep) and set(rows[0]) == {"image_id", "file_name", "category_id", "bbox", "score"}


def test_predict_refuses_bad_fuse_options(monkeypatch):
    from src.rtdetr_moe import engine, preprocess

    path = sorted(FRAMES.glob("*.jpg"))[0]
    kw = dict(imgsz=(128, 256), batch=1, device="cpu", conf=0.0, workers=0)
    made = []
    monkeypatch.setattr(preprocess, "FrameSource", lambda *a, **k: made.append(1))  # predict imports it per call
    monkeypatch.setattr(engine, "EvalForward", lambda *a, **k: made.append(1))
    with pytest.raises(ValueError, match="merge"):
        engine.predict(SPEC, [path], tiles=(2, 2), merge="wbf", **kw)
    with pytest.raises(ValueError, match="tiles"):
        engine.predict(SPEC, [path], merge="fuse", **kw)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="fuse_iou"):
            engine.predict(SPEC, [path], tiles=(2, 2), merge="fuse", fuse_iou=bad, **kw)
    # 73 passes of 50 candidates fit the merge (3650 <= 4096) but not the fusion's 64 windows
    with pytest.raises(ValueError, match="passes"):
        engine.predict(SPEC, [path], tiles=(8, 9), merge="fuse", max_det=50, **kw)
    assert not made  # refused before any frame is read


def test_boundary_and_script_pass_the_fuse_options():
    from scripts import predict_detector
    from src.models.vision import rtdetr as B

    torch.manual_seed(0)
    res = B.predict_rtdetr_detector(SPEC, str(FRAMES / "000101.jpg"), imgsz=(128, 256), batch=2, device="cpu",
                                    conf=0.0, tiles=(1, 2), merge="fuse", fuse_iou=0.3)
    (p,) = res.predictions
    assert p.members is not None and len(p.members) == len(p.scores) and bool((p.members >= 1).all())
    torch.manual_seed(0)
    (q,) = B.predict_rtdetr_detector(SPEC, str(FRAMES / "000101.jpg"), imgsz=(128, 256), batch=2, device="cpu",
                                     conf=0.0, tiles=(1, 2), merge="fuse", fuse_iou=1.0).predictions
    assert bool((q.members == 1).all()) and int(p.members.max()) >= 2  # fuse_iou reached the rule
    with pytest.raises(ValueError):
        B.predict_rtdetr_detector(SPEC, str(FRAMES / "000101.jpg"), imgsz=(128, 256), device="cpu", merge="fuse")
    a = predict_detector.parse_args(["--weights", SPEC, "--source", "x", "--tiles", "2x2", "--merge", "fuse",
                                     "--fuse-iou", "0.4"])
    assert a.merge == "fuse" and a.fuse_iou == 0.4
    d = predict_detector.parse_args(["--weights", SPEC, "--source", "x"])
    assert d.merge == "nms" and d.fuse_iou == 0.55
