"""engine.predict(flip=True) and engine.validate(flip=True) on the GPU: the
mirrored passes as further chunks of slots over the same descriptor rows
(rtdetr_resize_pad_u8_flip), the same captured graph, the passes merged in one
rtdetr_nms_merge / rtdetr_box_fuse launch per batch (rtdetr-r18-moe4-top1,
random weights, conf 0; the model and the size of tests/test_gpu_predict.py,
frames of 160 x 96)."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FRAMES = ROOT / "tests" / "golden" / "zod_mini" / "frames"
SPEC = "rtdetr-r18-moe4-top1"
IMGSZ = (320, 640)


def _frames(d, n=3):
    """n zod_mini frames at 160 x 96 (PNG: decoded bytes are the written ones); the first is its own mirror."""
    from PIL import Image

    d.mkdir(parents=True, exist_ok=True)
    out = []
    for i, p in enumerate(sorted(FRAMES.glob("*.jpg"))[:n]):
        a = np.asarray(Image.open(p).convert("RGB").resize((160, 96), Image.BILINEAR), dtype=np.uint8).copy()
        if i == 0:
            a[:, 80:] = a[:, :80][:, ::-1]
            assert np.array_equal(a, a[:, ::-1])
        q = d / f"{i:02d}_{p.stem}.png"
        Image.fromarray(a).save(q)
        out.append(q)
    return out


def _predict(source, batch=2, **kw):
    from src.rtdetr_moe import engine

    torch.manual_seed(0)  # the spec's random weights: the same model in every run
    return engine.predict(SPEC, source, imgsz=IMGSZ, batch=batch, device="0", conf=0.0, workers=0, **kw)


def _same_rows(a, b):
    return (torch.equal(a.boxes, b.boxes) and torch.equal(a.scores, b.scores) and torch.equal(a.labels, b.labels)
            and (a.source is None) == (b.source is None) and (a.source is None or torch.equal(a.source, b.source))
            and (a.members is None) == (b.members is None) and (a.members is None or torch.equal(a.members, b.members)))


@pytest.fixture(scope="module")
def flip_runs(hip_lib, tmp_path_factory):
    """predict(flip=True) without tiles on three frames at batch 2, merged on the device and on the host: the
    results, the launch counts, and every input the device run's forward was called with."""
    from src.moe import _lib as L
    from src.rtdetr_moe import engine

    d = tmp_path_factory.mktemp("flip_frames")
    paths = _frames(d)
    inputs = []

    class Recording(engine.EvalForward):
        def __call__(self, images, ctx):
            if not getattr(self, "preparing", False):
                inputs.append(images.clone())
            return super().__call__(images, ctx)

        def prepare(self, images, ctx):
            self.preparing = True
            super().prepare(images, ctx)
            self.preparing = False

    runs, counts = {}, {}
    with pytest.MonkeyPatch.context() as mp:
        for switch, fwd in (("1", Recording), ("0", engine.EvalForward)):
            mp.setenv("MOE_PREDICT_MERGE", switch)
            mp.setattr(engine, "EvalForward", fwd)
            L.launch_counts(reset=True)
            runs[switch] = _predict(d, flip=True)
            counts[switch] = L.launch_counts(reset=True)
    return dict(dir=d, paths=paths, runs=runs, counts=counts, inputs=inputs)


def test_flip_without_tiles_is_two_passes_and_one_merge_per_batch(flip_runs):
    from src.rtdetr_moe.merge import merge_reference

    runs, counts = flip_runs["runs"], flip_runs["counts"]
    # batches of 2 and 1 frames: per batch one resize launch per pass and one merge
    assert counts["1"].get("resize") == 4 and counts["1"].get("merge") == 2, counts["1"]
    assert counts["0"].get("resize") == 4 and "merge" not in counts["0"], counts["0"]
    assert len(flip_runs["inputs"]) == 4  # two replays per batch
    for res in runs.values():
        assert [p.path for p in res.predictions] == [str(q) for q in flip_runs["paths"]]
        assert set(res.speed) == {"preprocess", "inference", "postprocess", "passes"} and res.speed["passes"] == 2
        assert all(res.speed[key] > 0 for key in ("preprocess", "inference", "postprocess"))
    for a, b in zip(runs["1"].predictions, runs["0"].predictions):
        assert _same_rows(a, b)  # merged on the device as on the host, row for row
        n = len(a.scores)
        assert a.size == (160, 96) and 2 <= n <= 300 and a.members is None
        assert set(a.source.tolist()) <= {0, 1} and a.source.dtype == torch.int64
        assert bool((a.boxes >= 0).all() and (a.boxes[:, [0, 2]] <= 160).all() and (a.boxes[:, [1, 3]] <= 96).all())
        assert bool((a.scores[:-1] >= a.scores[1:]).all())
        assert merge_reference(a.boxes, a.scores, a.labels, None, 0.0, 0.5, "ios", 300).tolist() == list(range(n))
    # both passes reach the result somewhere in the run
    assert {int(s) for p in runs["1"].predictions for s in p.source.tolist()} == {0, 1}


def test_self_mirror_frame_gives_the_mirrored_pass_the_same_input(flip_runs):
    first, mirrored = flip_runs["inputs"][:2]  # the first batch: frame 0 is its own mirror, frame 1 is not
    assert tuple(first.shape) == (2, 3, *IMGSZ)
    assert torch.equal(first[0], mirrored[0])
    assert not torch.equal(first[1], mirrored[1])
    # the second batch's fill slot is empty in both passes
    last, last_mirrored = flip_runs["inputs"][2:]
    assert bool((last[1] == 0).all() and (last_mirrored[1] == 0).all()) and not torch.equal(last[0], last_mirrored[0])


def test_tiles_flip_and_fuse(hip_lib, flip_runs, monkeypatch):
    from src.moe import _lib as L

    runs, counts = {}, {}
    for switch in ("1", "0"):
        monkeypatch.setenv("MOE_PREDICT_MERGE", switch)
        L.launch_counts(reset=True)
        runs[switch] = _predict(flip_runs["dir"], tiles=(1, 2), flip=True, merge="fuse")
        counts[switch] = L.launch_counts(reset=True)
    # batches of 2 and 1 frames, 6 passes: 2 + 4 tile slots per half in chunks of 2 -> (1 + 2) x 2 + (1 + 1) x 2
    assert counts["1"].get("resize") == 10 and counts["1"].get("box_fuse") == 2, counts["1"]
    assert "merge" not in counts["1"]
    assert counts["0"].get("resize") == 10 and "box_fuse" not in counts["0"], counts["0"]
    fused = 0
    for a, b in zip(runs["1"].predictions, runs["0"].predictions):
        assert _same_rows(a, b)
        assert bool((a.source >= 0).all() and (a.source < 6).all())
        assert a.members.dtype == torch.int64 and bool((a.members >= 1).all())
        assert bool((a.boxes >= 0).all() and (a.boxes[:, [0, 2]] <= 160).all() and (a.boxes[:, [1, 3]] <= 96).all())
        fused += int((a.members > 1).sum())
    assert fused > 0
    assert runs["1"].speed["passes"] == 6 == runs["0"].speed["passes"]
    assert {int(s) for p in runs["1"].predictions for s in p.source.tolist()} - {0, 1, 2}  # a mirrored pass kept rows


def test_track_with_flip_reports_a_subset_of_the_untracked_rows(hip_lib, flip_runs):
    from src.moe import _lib as L

    # the random weights score every query alike, on a coarse grid of values: bands at the quartiles of the
    # distinct scores of the untracked run, and a track reported from its first hit
    u = torch.unique(torch.cat([p.scores for p in flip_runs["runs"]["1"].predictions]))
    lo, hi, new = (float(u[min(len(u) * q // 4, len(u) - 1)]) for q in (1, 2, 3))
    L.launch_counts(reset=True)
    res = _predict(flip_runs["dir"], flip=True, sequence_of=lambda p: "s",
                   track=dict(track_low=lo, track_high=hi, new_thr=new, min_hits=1))
    counts = L.launch_counts(reset=True)
    assert counts.get("track") == 2 and counts.get("merge") == 2 and counts.get("resize") == 4, counts
    total = 0
    for t, u in zip(res.predictions, flip_runs["runs"]["1"].predictions):
        assert t.track_ids is not None and len(t.track_ids) == len(t.scores) and t.sequence == "s"
        rows = torch.cat([u.boxes, u.scores[:, None], u.labels[:, None].float()], 1)
        mine = torch.cat([t.boxes, t.scores[:, None], t.labels[:, None].float()], 1)
        for r, s in zip(mine, t.source):
            hit = (rows == r).all(1)
            assert bool(hit.any()) and int(s) in u.source[hit].tolist()  # the same bits, the same pass
        total += len(mine)
    assert total > 0


def test_flip_false_is_the_call_without_the_argument(hip_lib, flip_runs):
    from src.moe import _lib as L

    runs, counts = [], []
    for kw in ({}, {"flip": False}):
        L.launch_counts(reset=True)
        runs.append(_predict(flip_runs["dir"], **kw))
        counts.append(L.launch_counts(reset=True))
    assert counts[0] == counts[1] and counts[0].get("resize") == 2 and "merge" not in counts[0], counts
    assert set(runs[1].speed) == {"preprocess", "inference", "postprocess"}
    for a, b in zip(runs[0].predictions, runs[1].predictions):
        assert _same_rows(a, b) and b.source is None and b.members is None and tuple(b.boxes.shape) == (300, 4)
    # the unmirrored pass of the flip run is this run: the rows it kept from pass 0 are rows of it
    for a, f in zip(runs[0].predictions, flip_runs["runs"]["1"].predictions):
        kept = f.boxes[f.source == 0]
        assert all(bool((a.boxes == r).all(1).any()) for r in kept)


def test_validate_with_flip(hip_lib, monkeypatch):
    from src.moe import _lib as L
    from src.rtdetr_moe import engine

    calls = []

    class Counting(engine.EvalForward):
        def __call__(self, images, ctx):
            if not getattr(self, "preparing", False):
                calls.append(1)
            return super().__call__(images, ctx)

        def prepare(self, images, ctx):
            self.preparing = True
            super().prepare(images, ctx)
            self.preparing = False

    monkeypatch.setattr(engine, "EvalForward", Counting)
    kw = dict(imgsz=(128, 128), batch=2, device="0", workers=0)
    out, counts, n_calls = [], [], []
    for more in ({}, {"flip": False}, {"flip": True}, {"flip": True, "merge": "fuse"}):
        torch.manual_seed(0)
        del calls[:]
        L.launch_counts(reset=True)
        out.append(engine.validate(SPEC, "synthetic:2", **more, **kw))
        c = L.launch_counts(reset=True)
        counts.append({k: c.get(k, 0) for k in ("merge", "box_fuse", "eval_match")})
        n_calls.append(len(calls))
    assert n_calls == [2, 2, 4, 4]  # twice the forward replays
    assert counts[0] == counts[1] == {"merge": 0, "box_fuse": 0, "eval_match": 2}
    assert counts[2] == {"merge": 2, "box_fuse": 0, "eval_match": 2}
    assert counts[3] == {"merge": 0, "box_fuse": 2, "eval_match": 2}
    assert out[0].results_dict == out[1].results_dict and set(out[0].speed) == set(out[2].speed)
    for m in out[2:]:
        assert all(0.0 <= v <= 1.0 for v in m.results_dict.values()) and m.speed["inference"] > 0


@pytest.mark.parametrize("mode", ["nms", "fuse"])
def test_validate_flip_scores_on_the_gpu_the_rows_of_the_cpu_path(hip_lib, monkeypatch, mode):
    """What the matcher is handed on the GPU, against the CPU path on the same two passes (which
    tests/test_flip_cpu.py holds against the rule written out): the second forward's input is the batch with its
    content region mirrored, and the one merge (fusion) launch gives merge_reference's (fuse_reference's) rows, the
    tail past them zero.  Content 100 columns in a tensor of 128: the un-mirroring width is the content's."""
    from src.rtdetr_moe import engine, metrics

    inputs, passes, handed = [], [], []

    class Recording(engine.EvalForward):
        def __call__(self, images, ctx):
            if not getattr(self, "preparing", False):
                inputs.append(images.clone())
            return super().__call__(images, ctx)

        def prepare(self, images, ctx):
            self.preparing = True
            super().prepare(images, ctx)
            self.preparing = False

    flip_rows = engine._flip_rows

    def spy_rows(first, second, content_w, content_h, rule, on_gpu):
        got = flip_rows(first, second, content_w, content_h, rule, on_gpu)
        passes.append(([t.clone() for t in first], [t.clone() for t in second], content_w, content_h, rule, on_gpu,
                       [t.clone() for t in got]))
        return got

    update_batch = metrics.DeviceDetectionEvaluator.update_batch

    def spy_update(self, boxes, scores, labels, *a, **kw):
        handed.append((boxes.clone(), scores.clone(), labels.clone()))
        return update_batch(self, boxes, scores, labels, *a, **kw)

    monkeypatch.setattr(engine, "EvalForward", Recording)
    monkeypatch.setattr(engine, "_flip_rows", spy_rows)
    monkeypatch.setattr(metrics.DeviceDetectionEvaluator, "update_batch", spy_update)
    torch.manual_seed(0)
    engine.validate(SPEC, "synthetic:2", imgsz=(128, 100), batch=2, device="0", workers=0, flip=True, merge=mode,
                    merge_iou=0.4, merge_metric="iou", fuse_iou=0.3)
    assert len(inputs) == 4 and len(passes) == 2 == len(handed)
    kept = 0
    for b, (first, second, cw, ch, rule, on_gpu, got) in enumerate(passes):
        images, mirrored = inputs[2 * b], inputs[2 * b + 1]
        assert tuple(images.shape) == (2, 3, 128, 128) and (cw, ch, on_gpu) == (100, 128, True)
        assert rule == (mode == "fuse", 0.4, "iou", 0.3)
        want = images.clone()
        want[..., :100] = torch.flip(images[..., :100], dims=(-1,))
        assert torch.equal(mirrored, want) and not torch.equal(mirrored, images)
        assert bool((images[..., 100:] == 0).all()) and mirrored.is_contiguous(memory_format=torch.channels_last)
        assert not torch.equal(first[1], second[1])  # the two passes differ
        K = first[1].shape[1]
        assert all(torch.equal(h, g) for h, g in zip(handed[b], got)) and tuple(got[0].shape) == (2, K, 4)
        cpu = flip_rows([t.cpu() for t in first], [t.cpu() for t in second], cw, ch, rule, False)
        for i in range(2):
            n = len(cpu[1][i])
            assert 1 <= n <= K
            assert torch.equal(got[0][i, :n].cpu(), cpu[0][i]) and torch.equal(got[1][i, :n].cpu(), cpu[1][i])
            assert torch.equal(got[2][i, :n].cpu(), cpu[2][i])
            assert bool((got[1][i, n:] == 0).all() and (got[0][i, n:] == 0).all())
            kept += n
    assert kept > 4
