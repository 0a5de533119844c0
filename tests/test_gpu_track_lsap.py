"""rtdetr_track_update_assoc / rtdetr_track_sweep_assoc (TrackArgs.assoc = "lsap"
through _lib.track_update / _lib.track_sweep) against track.track_reference:
out_id, out_boxes (as bits), count and the whole state after the launch, exactly,
into garbage-filled outputs -- the kernel prunes and solves the reference's
problems with the reference's solver, tie for tie.  Every drawn case asserts on
the reference, before the GPU is touched, that problems are solved and that the
answer differs from the greedy rule's (track_lsap_cases.check_preconditions)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import track_lsap_cases as C
from track_cases import check_hand_case
from tune_cases import KEY, case, reports_equal

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _garbage(F, K):
    return (torch.full((F, K), 12345, dtype=torch.int32, device=DEV),
            torch.full((F, K, 4), float("nan"), device=DEV), torch.full((F,), 999, dtype=torch.int32, device=DEV))


def _launch(L, state, seqs, order, slots, resets, nvs, args, shift=None):
    """One launch over the frames ``order`` = [(sequence number, frame)], -> numpy (out_id, out_box, count)."""
    t = lambda key, dt: torch.from_numpy(np.stack([seqs[q][key][f] for q, f in order])).to(dt).to(DEV)  # noqa: E731
    boxes, scores, labels = t("boxes", torch.float32), t("scores", torch.float32), t("labels", torch.int32)
    nv = None
    if nvs is not None:
        nv = torch.tensor([int(nvs[q][f]) for q, f in order], dtype=torch.int32, device=DEV)
    F, K = scores.shape
    sh = None if shift is None else torch.from_numpy(np.stack([shift[q][f] for q, f in order])).float().to(DEV)
    out = L.track_update(state, boxes, scores, labels, nv, torch.tensor(slots, dtype=torch.int32, device=DEV),
                         torch.tensor(resets, dtype=torch.int32, device=DEV), args, out=_garbage(F, K), shift=sh)
    return tuple(o.cpu().numpy() for o in out)


def _same(got, ref, frames=None):
    oid, obox, cnt = got
    sel = slice(None) if frames is None else frames
    assert np.array_equal(cnt, ref["count"][sel]), (cnt.tolist(), ref["count"][sel].tolist())
    assert np.array_equal(oid, ref["out_id"][sel]), np.argwhere(oid != ref["out_id"][sel])[:8].tolist()
    a, b = obox.view(np.int32), np.ascontiguousarray(ref["out_box"][sel]).view(np.int32)
    assert np.array_equal(a, b), np.argwhere(a != b)[:8].tolist()


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_drawn_sequences(hip_lib, shape):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackState, states_equal

    K, T, F = shape[:3]
    C.check_preconditions(shape)
    if shape == C.SHAPES[-1]:
        C.check_coverage()
    c = C.drawn(shape)
    state = TrackState(1, T, DEV)
    L.launch_counts(reset=True)
    got = _launch(L, state, [c["seq"]], [(0, f) for f in range(F)], [0] * F, [0] * F,
                  None if c["nv"] is None else [c["nv"]], c["args"])
    assert L.launch_counts(reset=True) == {"track": 1}
    _same(got, c["ref"])
    assert states_equal(state.export(0), c["ref"]["state"])


@pytest.mark.parametrize("case_", C.lsap_hand_cases(), ids=lambda c: c["name"])
def test_hand_cases(hip_lib, case_):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackArgs, TrackState, states_equal

    c = case_
    for assoc, want in (("lsap", c["ids"]), ("greedy", c["greedy"])):
        args = TrackArgs(max_tracks=c["T"], assoc=assoc, **c["args"])
        ref = C.run(c["seq"], args, c["T"], state=C.state_of(c["T"], c["tracks"]))
        state = TrackState(1, c["T"], DEV)
        state.load(0, C.state_of(c["T"], c["tracks"]))
        got = _launch(L, state, [c["seq"]], [(0, 0)], [0], [0], [c["seq"]["n_valid"]], args)
        n = int(c["seq"]["n_valid"][0])
        assert got[0][0][:n].tolist() == want, (c["name"], assoc)
        _same(got, ref)
        assert states_equal(state.export(0), ref["state"])


@pytest.mark.parametrize("case_", C.tie_cases(), ids=lambda c: c["name"])
def test_tie_cases_under_lsap(hip_lib, case_):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackArgs, TrackState, states_equal

    c = case_
    args = TrackArgs(max_tracks=c["T"], max_age=3, assoc="lsap", **c["args"])
    ref = C.run(c["seq"], args, c["T"])
    F = c["seq"]["scores"].shape[0]
    state = TrackState(1, c["T"], DEV)
    got = _launch(L, state, [c["seq"]], [(0, f) for f in range(F)], [0] * F, [0] * F, [c["seq"]["n_valid"]], args)
    check_hand_case(c, dict(out_id=got[0]))
    _same(got, ref)
    assert states_equal(state.export(0), ref["state"])


def test_two_launches_carry_the_state(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackState, states_equal

    shape = (300, 64, 16, 50, "given", 6, 8, True)
    K, T, F = shape[:3]
    c = C.drawn(shape)
    state = TrackState(1, T, DEV)
    parts = [_launch(L, state, [c["seq"]], [(0, f) for f in fr], [0] * len(fr), [0] * len(fr), [c["nv"]], c["args"])
             for fr in (range(7), range(7, 16))]
    _same(tuple(np.concatenate([p[j] for p in parts]) for j in range(3)), c["ref"])
    assert states_equal(state.export(0), c["ref"]["state"])


def test_two_sequences_interleaved(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackState, states_equal

    K, T = 65, 65
    args = C.shape_args(T)
    seqs = [C.draw_crowd(30, F, K, seed=40 + q, dup=4) for q, F in enumerate((6, 4))]
    refs = [C.run(s, args, T) for s in seqs]
    assert all(r["events"]["solves"] >= 3 and r["events"]["solve_n_max"] >= 8 for r in refs)
    order = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (0, 3), (1, 2), (0, 4), (1, 3), (0, 5)]
    slot_of = {0: 2, 1: 0}  # slot 1 has no frames
    state = TrackState(3, T, DEV)
    got = _launch(L, state, seqs, order, [slot_of[q] for q, _ in order], [0] * len(order),
                  [s["n_valid"] for s in seqs], args)
    for q, ref in enumerate(refs):
        rows = [i for i, (qq, _) in enumerate(order) if qq == q]
        _same(tuple(g[rows] for g in got), ref)
        assert states_equal(state.export(slot_of[q]), ref["state"])


def test_with_a_shift_table(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackState, states_equal

    K, T, F = 65, 64, 16
    args = C.shape_args(T)
    seq = C.draw_crowd(30, F, K, seed=50)
    shift = np.random.default_rng(1).uniform(-6, 6, (F, 2)).astype(np.float32)
    seq["boxes"] += np.cumsum(np.concatenate([shift, shift], 1), 0)[:, None, :]  # the camera moves every box
    ref = C.run(seq, args, T, shift=shift)
    plain = C.run(seq, args, T)
    assert ref["events"]["solves"] >= F - 1 and not np.array_equal(ref["out_id"], plain["out_id"])
    state = TrackState(1, T, DEV)
    got = _launch(L, state, [seq], [(0, f) for f in range(F)], [0] * F, [0] * F, [seq["n_valid"]], args, shift=[shift])
    _same(got, ref)
    assert states_equal(state.export(0), ref["state"])
    state = TrackState(1, T, DEV)  # and with NULL
    got = _launch(L, state, [seq], [(0, f) for f in range(F)], [0] * F, [0] * F, [seq["n_valid"]], args)
    _same(got, plain)
    assert states_equal(state.export(0), plain["state"])


def _raw_update(lib, entry, state, t, F, K, T, a, out, shift=None, assoc=None):
    common = (t["boxes"].data_ptr(), t["scores"].data_ptr(), t["labels"].data_ptr(), t["nv"].data_ptr(),
              t["slot"].data_ptr(), t["reset"].data_ptr(), F, K, 1, T, a.track_high, a.track_low, a.new_thr,
              a.match_iou, a.second_iou, a.max_age, a.min_hits, a.alpha, a.beta, 0,
              *(x.data_ptr() for x in state.tensors()), *(o.data_ptr() for o in out))
    sh = None if shift is None else shift.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    if entry == "rtdetr_track_update_assoc":
        return lib.rtdetr_track_update_assoc(*common, sh, assoc, st)
    return lib.rtdetr_track_update_shift(*common, sh, st)


def test_greedy_through_the_new_entry_is_the_old_one_bit_for_bit(hip_lib):
    from src.rtdetr_moe.track import TrackState

    shape = (300, 256, 16, 120, "given", 3, 0, True)
    K, T, F = shape[:3]
    c = C.drawn(shape)
    a = C.shape_args(T, assoc="greedy")
    seq = c["seq"]
    shift = torch.from_numpy(np.random.default_rng(2).uniform(-2, 2, (F, 2)).astype(np.float32)).to(DEV)
    t = dict(boxes=torch.from_numpy(seq["boxes"]).to(DEV), scores=torch.from_numpy(seq["scores"]).to(DEV),
             labels=torch.from_numpy(seq["labels"]).to(DEV), nv=torch.from_numpy(c["nv"]).to(DEV),
             slot=torch.zeros(F, dtype=torch.int32, device=DEV), reset=torch.zeros(F, dtype=torch.int32, device=DEV))
    for sh in (None, shift):
        res = {}
        for entry in ("rtdetr_track_update_shift", "rtdetr_track_update_assoc"):
            state, out = TrackState(1, T, DEV), _garbage(F, K)
            assert _raw_update(hip_lib, entry, state, t, F, K, T, a, out, sh, 0) == 0, hip_lib.moe_last_error()
            torch.cuda.synchronize()
            res[entry] = [x.clone() for x in (*out, *state.tensors())]
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(*res.values()))
        assert int(res["rtdetr_track_update_assoc"][2].sum()) >= 1000  # rows were reported


GRID6 = {"assoc": ["greedy", "lsap"], "match_iou": [0.2, 0.4, 0.6]}


def _sweep_inputs(seqs):
    """Two sequences' frames interleaved, as one launch's inputs."""
    F = min(len(s["n_valid"]) for s in seqs)
    order = [(q, f) for f in range(F) for q in range(len(seqs))]
    cat = lambda key, dt: torch.from_numpy(np.stack([seqs[q][key][f] for q, f in order])).to(dt).to(DEV)  # noqa: E731
    slot = torch.tensor([q for q, _ in order], dtype=torch.int32, device=DEV)
    return order, (cat("boxes", torch.float32), cat("scores", torch.float32), cat("labels", torch.int32),
                   cat("n_valid", torch.int32), slot, torch.zeros_like(slot))


def test_sweep_of_six_configurations_mixing_both_modes(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe import tune
    from src.rtdetr_moe.track import SweepState, states_equal

    K, T, F, S = 65, 65, 12, 2
    configs = tune.expand_grid(GRID6, C.shape_args(T, assoc="greedy"))
    assert [c.assoc for c in configs] == ["greedy"] * 3 + ["lsap"] * 3
    seqs = [C.draw_crowd(30, F, K, seed=60 + q, dup=4) for q in range(S)]
    refs = [[C.run(sq, cfg, T) for sq in seqs] for cfg in configs]
    assert all(r["events"]["solves"] >= F - 1 for g in range(3, 6) for r in refs[g])
    assert any(not np.array_equal(refs[g][q]["out_id"], refs[g + 3][q]["out_id"]) for g in range(3) for q in range(S))
    order, inputs = _sweep_inputs(seqs)
    state = SweepState(len(configs), S, T, DEV)
    G, n = len(configs), len(order)
    out = (torch.full((G, n, T), 777, dtype=torch.int32, device=DEV), torch.full((G, n, T, 4), float("nan"), device=DEV),
           torch.full((G, n, T), 777, dtype=torch.int32, device=DEV), torch.full((G, n), 777, dtype=torch.int32,
                                                                                  device=DEV))
    L.launch_counts(reset=True)
    oid, obox, orow, cnt = (x.cpu().numpy() for x in L.track_sweep(state, *inputs, configs, out=out))
    assert L.launch_counts(reset=True) == {"track_sweep": 1}
    for g in range(G):
        for q in range(S):
            ref = refs[g][q]
            for i, (qq, f) in enumerate(order):
                if qq != q:
                    continue
                rows = np.nonzero(ref["out_id"][f] >= 0)[0]
                k = len(rows)
                assert cnt[g, i] == k == ref["count"][f], (g, q, f)
                assert np.array_equal(oid[g, i, :k], ref["out_id"][f][rows]) and (oid[g, i, k:] == -1).all()
                assert np.array_equal(orow[g, i, :k], rows) and (orow[g, i, k:] == -1).all()
                assert np.array_equal(obox[g, i, :k].view(np.int32), ref["out_box"][f][rows].view(np.int32))
                assert not obox[g, i, k:].view(np.int32).any()
            assert states_equal(state.export(g, q), ref["state"]), (g, q)


def test_all_greedy_tables_equal_the_old_sweep(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe import tune
    from src.rtdetr_moe.track import SweepState

    K, T, F, S = 65, 65, 12, 2
    configs = tune.expand_grid({"match_iou": [0.2, 0.4, 0.6]}, C.shape_args(T, assoc="greedy"))
    seqs = [C.draw_crowd(30, F, K, seed=60 + q, dup=4) for q in range(S)]
    order, inputs = _sweep_inputs(seqs)
    G, n = len(configs), len(order)
    pf = torch.tensor([[float(getattr(c, k)) for k in L.SWEEP_F] for c in configs], dtype=torch.float32, device=DEV)
    pi = torch.tensor([[int(getattr(c, k)) for k in L.SWEEP_I] for c in configs], dtype=torch.int32, device=DEV)
    pa = torch.zeros(G, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    res = {}
    for entry in ("rtdetr_track_sweep", "rtdetr_track_sweep_assoc"):
        state = SweepState(G, S, T, DEV)
        out = (torch.full((G, n, T), 777, dtype=torch.int32, device=DEV),
               torch.full((G, n, T, 4), float("nan"), device=DEV),
               torch.full((G, n, T), 777, dtype=torch.int32, device=DEV),
               torch.full((G, n), 777, dtype=torch.int32, device=DEV))
        head = (*(x.data_ptr() for x in inputs), n, K, S, T, G, pf.data_ptr(), pi.data_ptr(),
                *(x.data_ptr() for x in state.tensors()), *(x.data_ptr() for x in out), None)
        tail = (pa.data_ptr(), st) if entry.endswith("assoc") else (st,)
        assert getattr(hip_lib, entry)(*head, *tail) == 0, hip_lib.moe_last_error()
        torch.cuda.synchronize()
        res[entry] = [x.clone() for x in (*out, *state.tensors())]
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(*res.values()))
    assert int(res["rtdetr_track_sweep"][3].sum()) >= 300  # rows were reported


def test_tune_sweep_with_an_assoc_grid_equals_the_cpu(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe import tune

    c = case(65, 2)
    base = {"max_tracks": 64, "max_age": 3}
    grid = {"assoc": ["greedy", "lsap"], "match_iou": [0.2, 0.5]}
    want = tune.sweep(c["dets"], c["gt"], grid, base=base, hota=True, device="cpu")
    L.launch_counts(reset=True)
    timing = {}
    got = tune.sweep(c["dets"], c["gt"], grid, base=base, hota=True, device=DEV, timing=timing)
    assert timing["launches"] == 1 and L.launch_counts(reset=True).get("track_sweep") == 1
    assert got == want
    assert [cfg["assoc"] for cfg in got["configs"]] == ["greedy", "greedy", "lsap", "lsap"]
    # the tracks themselves, bit for bit, per configuration
    configs = tune.expand_grid(grid, base)
    dev = tune.sweep_tracks(c["dets"], configs, 64, DEV)
    ref = tune.track_sweep_reference(c["dets"], configs, 64)
    assert all(reports_equal(dev[g][KEY], ref[g][KEY]) for g in range(4))


def test_bad_arguments_return_an_error_without_a_launch(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import SweepState, TrackState

    F, K, T, G = 2, 8, 4, 2
    state = TrackState(1, T, DEV)
    a = C.shape_args(T)
    t = dict(boxes=torch.zeros((F, K, 4), device=DEV), scores=torch.zeros((F, K), device=DEV),
             labels=torch.zeros((F, K), dtype=torch.int32, device=DEV), nv=torch.zeros(F, dtype=torch.int32, device=DEV),
             slot=torch.zeros(F, dtype=torch.int32, device=DEV), reset=torch.zeros(F, dtype=torch.int32, device=DEV))
    out = _garbage(F, K)
    before = [x.clone() for x in (*out, *state.tensors())]
    L.launch_counts(reset=True)
    for kw in (dict(assoc=2), dict(assoc=-1), dict(assoc=1 << 20), dict(K=1025), dict(T=257), dict(T=0), dict(F=1025)):
        q = {"F": F, "K": K, "T": T, "assoc": 1, **kw}
        assert _raw_update(hip_lib, "rtdetr_track_update_assoc", state, t, q["F"], q["K"], q["T"], a, out, None,
                           q["assoc"]) != 0, kw
        assert hip_lib.moe_last_error().decode().startswith("rtdetr_track_update_assoc"), kw
    # the sweep: NULL params_assoc, and the limits
    sw = SweepState(G, 1, T, DEV)
    pf, pi = torch.zeros((G, 7), device=DEV), torch.ones((G, 3), dtype=torch.int32, device=DEV)
    pa = torch.zeros(G, dtype=torch.int32, device=DEV)
    so = (torch.zeros((G, F, T), dtype=torch.int32, device=DEV), torch.zeros((G, F, T, 4), device=DEV),
          torch.zeros((G, F, T), dtype=torch.int32, device=DEV), torch.zeros((G, F), dtype=torch.int32, device=DEV))
    st = torch.cuda.current_stream().cuda_stream

    def sweep(K=K, T=T, G=G, pa=pa.data_ptr()):
        return hip_lib.rtdetr_track_sweep_assoc(t["boxes"].data_ptr(), t["scores"].data_ptr(), t["labels"].data_ptr(),
                                                None, t["slot"].data_ptr(), t["reset"].data_ptr(), F, K, 1, T, G,
                                                pf.data_ptr(), pi.data_ptr(), *(x.data_ptr() for x in sw.tensors()),
                                                *(x.data_ptr() for x in so), None, pa, st)

    for kw in (dict(pa=None), dict(K=1025), dict(T=257), dict(G=0), dict(G=1025)):
        assert sweep(**kw) != 0, kw
        assert hip_lib.moe_last_error().decode().startswith("rtdetr_track_sweep_assoc"), kw
    torch.cuda.synchronize()
    assert not L.launch_counts()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip((*out, *state.tensors()), before))
    assert sweep() == 0 and _raw_update(hip_lib, "rtdetr_track_update_assoc", state, t, F, K, T, a, out, None, 1) == 0
    torch.cuda.synchronize()
    assert L.launch_counts(reset=True) == {"track": 1, "track_sweep": 1}
    assert {"rtdetr_track_update_assoc", "rtdetr_track_sweep_assoc"} <= set(L.SIGNATURES)
