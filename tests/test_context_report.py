"""The per-context validation report on the CPU: the
routing-table reference against a table written out by hand, the mutual
information, per-context detection metrics against fresh evaluators, and
engine.validate end to end on tests/golden/zod_mini.  Every comparison is an
integer or ``==``."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
import torch

from eval_match_cases import random_image

FIX = Path(__file__).resolve().parent / "golden" / "zod_mini"
F = 1 << 32  # one, in the tables' fixed point
MODEL = "rtdetr-r18-moe4-top1"
IMGSZ = (320, 640)


def zod_mini_data(split="val"):
    return {split: {"img_folder": str(FIX / "frames"), "ann_file": str(FIX / "annotations" / "instances_train.json")}}


def _hand_case():
    # T 6 = two images of 3 tokens, E 3, k 2; image 0 is context 1, image 1 context 0
    idx = torch.tensor([[0, 1], [1, 2], [0, 2], [2, 0], [1, 0], [2, 1]], dtype=torch.int32)
    w = torch.tensor([[0.75, 0.25], [0.5, 0.5], [0.75, 0.25], [0.625, 0.375], [0.75, 0.25], [0.5, 0.5]])
    pos = torch.tensor([[0, 3], [4, 6], [1, -1], [7, 2], [5, 8], [9, 10]], dtype=torch.int32)  # one dropped slot
    probs = torch.tensor([[0.5, 0.25, 0.25], [0.125, 0.5, 0.375], [0.5, 0.125, 0.375],
                          [0.25, 0.125, 0.625], [0.25, 0.5, 0.25], [0.125, 0.375, 0.5]])
    ctx = torch.tensor([1, 0], dtype=torch.int32)
    q = F // 8  # every weight and probability above is a multiple of 1/8
    want = torch.tensor([
        # context 0 = image 1 (tokens 3..5): assignments, top-1, dropped, gate mass, prob mass per expert
        [[2, 0, 0, 5 * q, 5 * q], [2, 1, 0, 10 * q, 8 * q], [2, 2, 0, 9 * q, 11 * q]],
        # context 1 = image 0 (tokens 0..2); the dropped slot is token 2's second choice, expert 2
        [[2, 2, 0, 12 * q, 9 * q], [2, 1, 0, 6 * q, 7 * q], [2, 0, 1, 6 * q, 8 * q]],
    ], dtype=torch.int64)
    return idx, w, pos, probs, ctx, want


def test_reference_equals_a_table_written_by_hand():
    from src.moe.stats import route_stats_reference

    idx, w, pos, probs, ctx, want = _hand_case()
    got = route_stats_reference(idx, w, pos, probs, ctx, 3, 2)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, 3, 5)
    assert torch.equal(got, want)
    # without pos nothing is dropped; without ctx_img every token is context 0
    no_pos = want.clone()
    no_pos[:, :, 2] = 0
    assert torch.equal(route_stats_reference(idx, w, None, probs, ctx, 3, 2), no_pos)
    assert torch.equal(route_stats_reference(idx, w, pos, probs, None, 3, 1), want.sum(0, keepdim=True))
    # fix() rounds half to even: 2^-33 -> 0.5 -> 0, 3 * 2^-33 -> 1.5 -> 2
    tiny = torch.tensor([[2.0 ** -33], [3 * 2.0 ** -33]])
    got = route_stats_reference(torch.zeros((2, 1), dtype=torch.int32), tiny, None, tiny, None, 1, 1)
    assert got[0, 0].tolist() == [2, 2, 0, 2, 2]


def test_reference_ignores_out_of_range_contexts_and_experts():
    from src.moe.stats import route_stats_reference

    idx, w, pos, probs, ctx, want = _hand_case()
    for bad in (-1, 2, 7):
        got = route_stats_reference(idx, w, pos, probs, torch.tensor([1, bad], dtype=torch.int32), 3, 2)
        assert torch.equal(got[1], want[1])  # image 0's contribution is unchanged
        assert int(got[0].abs().sum()) == 0  # image 1 is nowhere
    # an expert index outside [0, E) drops that slot only (token 0's second choice, expert 1 of context 1)
    idx2 = idx.clone()
    for bad in (-1, 3):
        idx2[0, 1] = bad
        w2 = want.clone()
        w2[1, 1] -= torch.tensor([1, 0, 0, F // 4, 0])
        assert torch.equal(route_stats_reference(idx2, w, pos, probs, ctx, 3, 2), w2)


def test_mi_bits():
    from src.moe.stats import mi_bits, routing_summary

    assert mi_bits([[5, 0], [0, 5]]) == 1.0     # the context decides the expert: one bit
    assert mi_bits([[3, 3], [3, 3]]) == 0.0     # it decides nothing
    assert mi_bits(np.zeros((6, 4), np.int64)) == 0.0
    assert 0.0 < mi_bits([[4, 1], [1, 4]]) < 1.0
    _, _, _, _, _, want = _hand_case()
    s = routing_summary(want.numpy(), 2, ("a", "b"))
    assert s["assignments"] == [[2, 2, 2], [2, 2, 2]] and s["tokens"] == [3, 3] and s["mi_bits"] == 0.0
    assert s["dropped"] == [[0, 0, 0], [0, 0, 1]] and s["gate_mass_float"][1] == [1.5, 0.75, 0.75]
    assert s["expert_share"][0] == [2 / 6, 2 / 6, 2 / 6] and s["prob_mass"][0][2] == 11 * (F // 8)
    json.dumps(s)


def test_compute_by_context_equals_fresh_evaluators():
    from src.moe.context import CONTEXT_LABELS
    from src.rtdetr_moe.metrics import DetectionEvaluator

    rng = np.random.default_rng(5)
    ids = [0, 2, 3, 5]
    images = [random_image(rng, 40, 0 if i % 7 == 3 else int(rng.integers(1, 9))) for i in range(24)]
    ctx = [ids[i % 4] for i in range(24)]
    ev = DetectionEvaluator()
    for im, c in zip(images, ctx):
        ev.update(*im, ctx=c)
    assert ev.image_ctx == ctx
    by = ev.compute_by_context()
    assert list(by) == [CONTEXT_LABELS[c] for c in ids]  # absent contexts are absent
    for c in ids:
        fresh = DetectionEvaluator()
        sub = [im for im, ci in zip(images, ctx) if ci == c]
        for im in sub:
            fresh.update(*im)
        want, got = fresh.compute(), by[CONTEXT_LABELS[c]]
        assert got["images"] == 6 and got["targets"] == sum(len(im[3]) for im in sub)
        assert (got["box"].mp, got["box"].mr, got["box"].map50, got["box"].map) == \
            (want.mp, want.mr, want.map50, want.map)
        assert want.map50 > 0 and len(got["box"].curves_results) == len(want.curves_results) == 4
        for a, b in zip(got["box"].curves_results, want.curves_results):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    whole = DetectionEvaluator()
    for im in images:
        whole.update(*im)
    a, b = ev.compute(), whole.compute()  # compute() is untouched by the context ids
    assert (a.mp, a.mr, a.map50, a.map) == (b.mp, b.mr, b.map50, b.map)
    ev.update(*images[0])  # an update without a context id
    with pytest.raises(ValueError, match="context"):
        ev.compute_by_context()


def check_report_tokens(report, model):
    """The zod_mini report's routing tables: one image in each of night,
    mid_sun, high_sun and missing, so every MoE layer saw its tokens per image
    in those bins and none elsewhere."""
    from src.moe.context import CONTEXT_LABELS

    present = [0, 3, 4, 5]
    assert report["bins"] == list(CONTEXT_LABELS)
    assert list(report["detection"]) == [CONTEXT_LABELS[c] for c in present]
    assert all(d["images"] == 1 for d in report["detection"].values())
    assert sum(d["targets"] for d in report["detection"].values()) == 6
    layers = model.moe_layers()
    assert len(report["routing"]) == len(layers) > 0
    for r, layer in zip(report["routing"], layers):
        # the AIFI encoder layer routes the stride-32 map, a decoder layer its 300 queries
        per_image = (IMGSZ[0] // 32) * (IMGSZ[1] // 32) if r["layer"].startswith("encoder.") else 300
        k = layer.cfg.top_k
        assert r["experts"] == layer.cfg.num_experts and r["top_k"] == k
        tokens = [per_image if c in present else 0 for c in range(len(CONTEXT_LABELS))]
        assert r["tokens"] == tokens
        assert [sum(row) for row in r["top1"]] == tokens
        assert [sum(row) for row in r["assignments"]] == [k * t for t in tokens]
        assert 0.0 <= r["mi_bits"] <= 2.0


def test_validate_writes_the_context_report(tmp_path, monkeypatch):
    from src.rtdetr_moe import engine

    monkeypatch.delenv("MOE_CONTEXT_REPORT", raising=False)
    torch.manual_seed(0)
    m = engine.validate(MODEL, zod_mini_data(), imgsz=IMGSZ, batch=3, device="cpu", workers=0,
                        project=str(tmp_path), name="on", context_report=True)
    assert m.context is not None
    check_report_tokens(m.context, m.model.model)
    on_disk = json.loads((tmp_path / "on" / "context_report.json").read_text())
    assert on_disk == json.loads(json.dumps(m.context))
    assert all(layer.route_stats is None for layer in m.model.model.moe_layers())  # the sinks are cleared
    # the environment switch, as the unchanged reference scripts would set it
    monkeypatch.setenv("MOE_CONTEXT_REPORT", "1")
    torch.manual_seed(0)
    m2 = engine.validate(MODEL, zod_mini_data(), imgsz=IMGSZ, batch=3, device="cpu", workers=0)
    assert m2.context == m.context and m2.results_dict == m.results_dict


def test_validate_without_the_switch_is_unchanged(tmp_path, monkeypatch):
    from src.rtdetr_moe import engine

    monkeypatch.delenv("MOE_CONTEXT_REPORT", raising=False)
    m = engine.validate(MODEL, zod_mini_data(), imgsz=IMGSZ, batch=3, device="cpu", workers=0,
                        project=str(tmp_path), name="off")
    assert m.context is None
    assert not (tmp_path / "off" / "context_report.json").exists()
    assert set(m.results_dict) == {"metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)",
                                   "metrics/mAP50-95(B)", "fitness"}


def test_training_adds_the_context_columns(tmp_path, monkeypatch):
    import csv

    from src.moe.context import CONTEXT_LABELS
    from src.rtdetr_moe import engine

    monkeypatch.delenv("MOE_CONTEXT_REPORT", raising=False)
    data = {**zod_mini_data("train"), **zod_mini_data("val")}
    res = engine.train(engine.TrainArgs(model=MODEL, data=data, imgsz=(96, 160), epochs=1, batch=4, device="cpu",
                                        project=str(tmp_path), name="on", workers=0, context_report=True))
    with open(res.save_dir / "results.csv") as f:
        (row,) = list(csv.DictReader(f))
    for c, label in enumerate(CONTEXT_LABELS):  # an empty cell for a bin without targets
        cell = row.pop(f"metrics/mAP50-95(B)/{label}")
        assert (cell == "") == (c in (1, 2)) and (cell == "" or 0.0 <= float(cell) <= 1.0)
    layers = len(res.model.model.moe_layers())
    for i in range(layers):
        assert 0.0 <= float(row.pop(f"moe/l{i}_ctx_mi")) <= 2.0
    # what is left are the columns of a run without the switch
    assert list(row) == ["epoch", "train/loss", "time_s", *res.results_dict] + \
        [f"moe/l{i}_{name}" for i in range(layers) for name in ("load_cv", "lb", "z")]
