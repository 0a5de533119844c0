"""track.track_reference(shift=...) on the CPU: with each frame's camera shift
the tracks survive a pan that breaks them without it; without a shift nothing
changes; and the arguments and bindings that go with it."""
from __future__ import annotations

import numpy as np
import pytest

from motion_cases import PAN, pan_sequence, run_reference_shift
from track_cases import draw_sequence, identities, run_reference


def test_the_pan_keeps_one_id_per_object_with_the_shift():
    from src.rtdetr_moe.track import TrackArgs

    seq, shifts = pan_sequence()
    assert shifts[:, 0].tolist() == [float(v) for v in PAN] and not shifts[:, 1].any()
    res = run_reference_shift(seq, TrackArgs(), 64, shifts)
    ids, switches = identities(seq, res["out_id"])
    # the reference as built (the shift after the velocity): 8 objects x 19 frames, reported from their second frame
    assert all(len(v) == 1 for v in ids.values()) and switches == 0, (ids, switches)
    assert sorted(v[0] for v in ids.values()) == list(range(1, 9)), ids  # one id per object, ids 1..8
    assert int(res["count"].sum()) == 152 and res["count"].tolist() == [0] + [8] * 19
    assert int(res["state"]["next_id"]) == 9
    # the same input without the shift: the tree before this feature
    bare = run_reference_shift(seq, TrackArgs(), 64, None)
    ids0, switches0 = identities(seq, bare["out_id"])
    assert max(len(v) for v in ids0.values()) > 1 and switches0 > 0, (ids0, switches0)
    assert int(bare["count"].sum()) < 152


def test_no_shift_is_todays_tracker_bit_for_bit():
    from src.rtdetr_moe.track import TrackArgs, states_equal

    seq = draw_sequence(20, 24, 65, seed=2, jitter=2.0, miss=0.12, low_share=0.2, fp=3, leave={0: 12})
    args = TrackArgs(max_age=3)
    today = run_reference(seq, args, 64)  # never passes ``shift``
    none = run_reference_shift(seq, args, 64, None)
    zero = run_reference_shift(seq, args, 64, np.zeros((24, 2), np.float32))
    assert today["events"]["refound"] >= 1 and today["events"]["reported"] >= 100
    for res in (none, zero):  # no coordinate of this input is -0.0, so adding zero changes no bit either
        assert np.array_equal(res["out_id"], today["out_id"]) and np.array_equal(res["count"], today["count"])
        assert np.array_equal(res["out_box"].view(np.int32), today["out_box"].view(np.int32))
        assert states_equal(res["state"], today["state"])


def test_a_zero_shift_is_not_none_where_a_coordinate_is_minus_zero():
    from src.rtdetr_moe.track import new_state, track_reference

    outs = []
    for shift in (None, (0.0, 0.0)):
        state = new_state(2)  # a confirmed track at rest on the frame's corner: -0.0 + -0.0 stays -0.0
        state["box"][0], state["vel"][0] = (-0.0, -0.0, 40.0, 100.0), (-0.0, -0.0, 0.0, 0.0)
        state["score"][0], state["id"][0], state["hits"][0], state["next_id"] = 0.9, 1, 3, 2
        # a frame without rows: the track coasts on its prediction, box + vel (+ shift)
        track_reference(state, np.zeros((0, 4), np.float32), [], [], None, dict(min_hits=1), shift=shift)
        outs.append(state["box"][0].view(np.int32).tolist())
    assert outs[0][:2] == [np.int32(-2 ** 31)] * 2 and outs[1][:2] == [0, 0] and outs[0][2:] == outs[1][2:]


def test_the_shift_moves_coasting_tracks_and_leaves_the_velocity():
    from src.rtdetr_moe.track import new_state, track_reference

    state = new_state(2)
    a = dict(min_hits=1)
    track_reference(state, np.array([[100, 50, 140, 150]], np.float32), [0.9], [0], None, a)
    track_reference(state, np.array([[102, 50, 142, 150]], np.float32), [0.9], [0], None, a)
    vel = state["vel"][0].copy()
    before = state["box"][0].copy()
    track_reference(state, np.zeros((0, 4), np.float32), [], [], None, a, shift=(30.0, -7.5))
    f32 = np.float32
    want = (before + vel) + np.array([30.0, -7.5, 30.0, -7.5], f32)
    assert np.array_equal(state["box"][0], want) and np.array_equal(state["vel"][0], vel) and state["age"][0] == 1


def test_trackargs_cmc_fields():
    from src.rtdetr_moe.track import TrackArgs

    d = TrackArgs()
    assert (d.cmc, d.cmc_radius, d.cmc_gate, d.cmc_rows) == (False, 48, 0.1, (0.0, 1.0))
    assert TrackArgs.parse(True) == TrackArgs()
    a = TrackArgs.parse({"cmc": True, "cmc_radius": 16, "cmc_gate": 0, "cmc_rows": [0.0, 0.75]})
    assert (a.cmc, a.cmc_radius, a.cmc_gate, a.cmc_rows) == (True, 16, 0.0, (0.0, 0.75))
    assert a.as_dict()["cmc_rows"] == (0.0, 0.75)
    for bad in (dict(cmc=1), dict(cmc="yes"), dict(cmc_radius=0), dict(cmc_radius=50), dict(cmc_radius=68),
                dict(cmc_radius=12.5), dict(cmc_gate=1.0), dict(cmc_gate=-0.01), dict(cmc_gate=float("nan")),
                dict(cmc_rows=(0.5, 0.5)), dict(cmc_rows=(-0.1, 1.0)), dict(cmc_rows=(0.0, 1.1)), dict(cmc_rows=0.5),
                dict(cmc_rows=(0.0, 0.5, 1.0))):
        with pytest.raises(ValueError, match="cmc"):
            TrackArgs(**bad)


def test_bindings():
    from src.moe import _lib as L

    assert "rtdetr_frame_shift" in L.SIGNATURES and "rtdetr_track_update_shift" in L.SIGNATURES
    assert L.PROF_KINDS[21] == "motion" and L.PROF_KINDS[20] == "track"
    assert len(L.SIGNATURES["rtdetr_track_update_shift"][1]) == len(L.SIGNATURES["rtdetr_track_update"][1]) + 1


def test_engine_track_with_cmc_on_the_cpu(tmp_path):
    import json

    import torch

    from motion_cases import draw_frames
    from src.rtdetr_moe import engine

    layout = (("seqA", [(0, 0), (7, -3), (-12, 5)]), ("seqB", [(0, 0), (-5, 9)]))
    src = tmp_path / "frames"
    src.mkdir()
    draw_frames(src, layout, (128, 256))
    kw = dict(imgsz=(128, 256), batch=2, device="cpu", conf=0.0, workers=0)
    torch.manual_seed(0)
    plain = engine.predict("rtdetr-r18-moe4-top1", src, **kw)
    # the random weights score every query alike: bands at the quartiles of the distinct scores
    u = torch.unique(torch.cat([p.scores for p in plain.predictions]))
    lo, hi, new = (float(u[min(len(u) * q // 4, len(u) - 1)]) for q in (1, 2, 3))
    bands = dict(track_low=lo, track_high=hi, new_thr=new, min_hits=1)
    torch.manual_seed(0)
    off = engine.track("rtdetr-r18-moe4-top1", src, tracker=bands, **kw)
    torch.manual_seed(0)
    on = engine.track("rtdetr-r18-moe4-top1", src, tracker=dict(bands, cmc=True, cmc_radius=16), project=str(tmp_path),
                      name="run", **kw)
    assert all(p.camera_shift is None and p.camera_status is None for p in off.predictions)
    steps = [s for _, seq in layout for s in seq]
    for p, (dx, dy) in zip(on.predictions, steps):  # 512 x 256 frames: two source pixels per input pixel
        assert p.camera_shift == (2.0 * dx, 2.0 * dy) and p.camera_status == int(p.frame > 1), (p.path, p.camera_shift)
    assert sum(len(p.track_ids) for p in on.predictions) >= 5
    # the detections are the same rows; the shift changes what the tracks match
    assert any(not torch.equal(a.track_boxes, b.track_boxes) for a, b in zip(on.predictions, off.predictions))
    got = json.loads((tmp_path / "run" / "camera_motion.json").read_text())
    assert got == {"seqA": [[1, 0.0, 0.0, 0], [2, 14.0, -6.0, 1], [3, -24.0, 10.0, 1]],
                   "seqB": [[1, 0.0, 0.0, 0], [2, -10.0, 18.0, 1]]}
    assert (tmp_path / "run" / "tracks.json").exists()


def test_scripts_take_the_cmc_options():
    from scripts import predict_detector as P

    base = ["--weights", "rtdetr-r18-moe4-top1", "--source", "x"]
    a = P.parse_args(base + ["--track", "--cmc", "--cmc-radius", "32", "--cmc-gate", "0.2", "--cmc-rows", "0,0.8"])
    assert P.tracker_args(a) == {"cmc": True, "cmc_radius": 32, "cmc_gate": 0.2, "cmc_rows": (0.0, 0.8)}
    a = P.parse_args(base + ["--track", "--tracker", '{"max_age": 3}', "--cmc"])
    assert P.tracker_args(a) == {"max_age": 3, "cmc": True}
    assert P.tracker_args(P.parse_args(base + ["--track"])) is True and P.tracker_args(P.parse_args(base)) is None
    assert P.tracker_args(P.parse_args(base + ["--track", "--tracker", '{"cmc": true}'])) == {"cmc": True}
    for bad in (["--cmc"], ["--track", "--cmc-radius", "32"], ["--cmc-rows", "0,1"]):
        with pytest.raises(SystemExit):
            P.parse_args(base + bad)
