"""rtdetr_track_sweep (_lib.track_sweep) against tune.track_sweep_reference:
count, the compact ids / boxes (as bits) / rows and every configuration's whole
state, exactly; with one configuration it is the compaction of
rtdetr_track_update's outputs; and tune.sweep end to end on the GPU against the
CPU.  The outputs are pre-filled with poison: every element must be written."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from tune_cases import GRID16, KEY, SHAPES, case, check_distinct, reference

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F = 24


def _poison(G, n, T):
    return (torch.full((G, n, T), 12345, dtype=torch.int32, device=DEV),
            torch.full((G, n, T, 4), float("nan"), device=DEV),
            torch.full((G, n, T), 777, dtype=torch.int32, device=DEV),
            torch.full((G, n), 999, dtype=torch.int32, device=DEV))


def _launch(L, state, seq, part, configs, slots, shift=None, n_valid=False):
    """One launch over seq's frames ``part`` -> numpy (ids, boxes, rows, count), each with a leading G."""
    up = lambda key, dt: torch.from_numpy(np.ascontiguousarray(seq[key][part])).to(dt).to(DEV)  # noqa: E731
    n = len(seq["scores"][part])
    sh = None if shift is None else torch.from_numpy(np.ascontiguousarray(shift[part], np.float32)).to(DEV)
    got = L.track_sweep(state, up("boxes", torch.float32), up("scores", torch.float32), up("labels", torch.int32),
                        up("n_valid", torch.int32) if n_valid else None,
                        torch.tensor(slots, dtype=torch.int32, device=DEV),
                        torch.zeros(n, dtype=torch.int32, device=DEV), configs, out=_poison(state.G, n, state.T),
                        shift=sh)
    return tuple(o.cpu().numpy() for o in got)


def _same(got, ref, part, g):
    ids, boxes, rows, count = (x[g] for x in got)
    assert np.array_equal(count, ref["count"][part]), (g, count.tolist(), ref["count"][part].tolist())
    assert np.array_equal(ids, ref["ids"][part]), (g, np.argwhere(ids != ref["ids"][part])[:8].tolist())
    assert np.array_equal(rows, ref["rows"][part]), (g, np.argwhere(rows != ref["rows"][part])[:8].tolist())
    a, b = boxes.view(np.int32), np.ascontiguousarray(ref["boxes"][part]).view(np.int32)
    assert np.array_equal(a, b), (g, np.argwhere(a != b)[:8].tolist())


def test_one_configuration_is_the_compaction_of_track_update(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import SweepState, TrackArgs, TrackState

    K, T = 65, 64
    seq = case(K, 2)["seq"]
    args = TrackArgs(max_age=3, max_tracks=T)
    up = lambda key, dt: torch.from_numpy(seq[key]).to(dt).to(DEV)  # noqa: E731
    tab = torch.zeros(F, dtype=torch.int32, device=DEV)
    plain = TrackState(1, T, DEV)
    oid, obox, cnt = (o.cpu().numpy() for o in L.track_update(
        plain, up("boxes", torch.float32), up("scores", torch.float32), up("labels", torch.int32),
        up("n_valid", torch.int32), tab, tab, args))
    state = SweepState(1, 1, T, DEV)
    ids, boxes, rows, count = _launch(L, state, seq, slice(0, F), [args], [0] * F, n_valid=True)
    assert int(cnt.sum()) >= 200 and np.array_equal(count[0], cnt)
    for f in range(F):
        d = np.nonzero(oid[f] >= 0)[0]
        n = len(d)
        assert np.array_equal(rows[0, f, :n], d) and (rows[0, f, n:] == -1).all()
        assert np.array_equal(ids[0, f, :n], oid[f][d]) and (ids[0, f, n:] == -1).all()
        assert boxes[0, f, :n].tobytes() == obox[f][d].tobytes() and not boxes[0, f, n:].view(np.int32).any()
    for a, b in zip(state.tensors(), plain.tensors()):
        assert torch.equal(a[0].view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("K,T,seed", SHAPES)
def test_grid16_equals_the_reference(hip_lib, K, T, seed):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import SweepState, states_equal

    seq = case(K, seed)["seq"]
    configs, ref = reference(K, T, seed)
    check_distinct(K, T, seed, ref)
    if (K, T, seed) == (40, 8, 3):
        assert max(r["state"]["dropped"] for r in ref) == 254  # the full-slot path
    G = len(configs)
    state = SweepState(G, 2, T, DEV)
    for g in (0, G - 1):
        state.load(g, 0, ref[3]["state"])  # somebody's tracks in slot 0, which must stay as they are
    idle = [t[:, 0].clone() for t in state.tensors()]
    L.launch_counts(reset=True)
    for part in (slice(0, 9), slice(9, F)):
        n = len(range(*part.indices(F)))
        got = _launch(L, state, seq, part, configs, [1] * n)
        for g in range(G):
            _same(got, ref[g], part, g)
    assert L.launch_counts(reset=True) == {"track_sweep": 2}
    exported = state.export_all()
    for g in range(G):
        assert states_equal(state.export(g, 1), ref[g]["state"]), g
        assert states_equal(exported[g][1], ref[g]["state"]), g
    for t, before in zip(state.tensors(), idle):
        assert torch.equal(t[:, 0].view(torch.int32), before.view(torch.int32))
    assert states_equal(state.export(G - 1, 0), ref[3]["state"])


def test_shifts_equal_the_reference_and_null_adds_nothing(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import SweepState, states_equal

    K, T, seed = 65, 64, 2
    seq = case(K, seed)["seq"]
    rng = np.random.default_rng(seed)
    shifts = (rng.normal(0, 6.0, (F, 2)) * (rng.random((F, 1)) < 0.7)).astype(np.float32)  # test_gpu_track_shift's
    configs, ref = reference(K, T, seed, shifts=shifts, tag="shift")
    _, bare = reference(K, T, seed)
    assert (shifts == 0).all(1).any() and (shifts != 0).all(1).any()
    assert not any(states_equal(a["state"], b["state"]) for a, b in zip(ref, bare))  # the shifts mattered
    for table, want in ((shifts, ref), (None, bare)):
        state = SweepState(len(configs), 1, T, DEV)
        got = _launch(L, state, seq, slice(0, F), configs, [0] * F, shift=table)
        for g in range(len(configs)):
            _same(got, want[g], slice(0, F), g)
            assert states_equal(state.export(g, 0), want[g]["state"]), g


def test_a_frame_of_nobodys_slot_is_empty_for_every_configuration(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe import tune
    from src.rtdetr_moe.track import SweepState, TrackArgs, states_equal

    K, T = 65, 64
    c = case(K, 2)
    configs = tune.expand_grid(GRID16, TrackArgs(max_tracks=T))
    keep = [0, 2, 3]
    dets = {KEY: {i + 1: c["dets"][KEY][f + 1] for i, f in enumerate(keep)}}
    ref = [r[KEY] for r in tune.track_sweep_reference(dets, configs, T)]
    state = SweepState(len(configs), 2, T, DEV)
    before = [t[:, 1].clone() for t in state.tensors()]
    got = _launch(L, state, c["seq"], slice(0, 6), configs, [0, -1, 0, 0, 2, 1 << 20])
    for g in range(len(configs)):
        _same(tuple(x[:, keep] for x in got), ref[g], slice(0, 3), g)
        assert states_equal(state.export(g, 0), ref[g]["state"])
        for f in (1, 4, 5):
            assert got[3][g, f] == 0 and (got[0][g, f] == -1).all() and (got[2][g, f] == -1).all()
            assert not got[1][g, f].view(np.int32).any()
    for t, b in zip(state.tensors(), before):
        assert torch.equal(t[:, 1].view(torch.int32), b.view(torch.int32))


def test_refusals_name_the_entry_and_launch_nothing(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import SweepState, TrackArgs

    n, K, T, G = 2, 8, 4, 3
    state = SweepState(G, 1, T, DEV)
    boxes, scores = torch.zeros((n, K, 4), device=DEV), torch.zeros((n, K), device=DEV)
    labels = torch.zeros((n, K), dtype=torch.int32, device=DEV)
    tab = torch.zeros((2, n), dtype=torch.int32, device=DEV)
    pf = torch.tensor([[0.5, 0.1, 0.6, 0.2, 0.5, 0.5, 0.25]] * G, device=DEV)
    pi = torch.tensor([[30, 2, 0]] * G, dtype=torch.int32, device=DEV)
    out = _poison(G, n, T)
    before = [t.clone() for t in (*out, *state.tensors())]
    st = torch.cuda.current_stream().cuda_stream
    ptr = dict(boxes=boxes, scores=scores, labels=labels, slot=tab[0], reset=tab[1], pf=pf, pi=pi, tbox=state.box,
               tscore=state.score, tmeta=state.meta, seq=state.seq, oid=out[0], obox=out[1], orow=out[2], count=out[3])
    ptr = {k: v.data_ptr() for k, v in ptr.items()}

    def call(n=n, K=K, S=1, T=T, G=G, **p):
        q = {**ptr, **p}
        return hip_lib.rtdetr_track_sweep(q["boxes"], q["scores"], q["labels"], None, q["slot"], q["reset"], n, K, S, T,
                                          G, q["pf"], q["pi"], q["tbox"], q["tscore"], q["tmeta"], q["seq"], q["oid"],
                                          q["obox"], q["orow"], q["count"], None, st)

    L.launch_counts(reset=True)
    bad = [dict(G=0), dict(G=1025), dict(T=257), dict(K=1025), dict(pf=None), dict(pi=None), dict(T=0), dict(n=1025),
           dict(S=1025), dict(S=0), dict(K=-1), dict(n=-1), dict(boxes=ptr["boxes"] + 4), dict(obox=ptr["obox"] + 4),
           dict(tbox=ptr["tbox"] + 4), dict(tmeta=ptr["tmeta"] + 4)]
    bad += [{k: None} for k in ptr]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert hip_lib.moe_last_error().decode().startswith("rtdetr_track_sweep"), kw
    torch.cuda.synchronize()
    assert not L.launch_counts()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32))
               for a, b in zip((*out, *state.tensors()), before))
    assert call(n=0) == 0 and not L.launch_counts()  # no frames: no launch
    assert call() == 0
    torch.cuda.synchronize()
    assert L.launch_counts(reset=True) == {"track_sweep": 1}
    assert out[3].tolist() == [[0] * n] * G and (out[0] == -1).all() and (out[2] == -1).all() and not out[1].any()
    # the typed wrapper refuses what the C entry cannot see
    args = [TrackArgs(max_tracks=T)] * G
    with pytest.raises(L.MoEKernelError):
        L.track_sweep(state, boxes, scores, labels, None, tab[0], tab[1], args[:2])
    with pytest.raises(L.MoEKernelError):
        L.track_sweep(state, boxes, scores, labels, None, tab[0], tab[1], [a.as_dict() for a in args])
    with pytest.raises(L.MoEKernelError):
        L.track_sweep(state, boxes, scores[:, :7], labels, None, tab[0], tab[1], args)
    with pytest.raises(L.MoEKernelError):
        L.track_sweep(state, boxes, scores, labels, None, tab[0].cpu(), tab[1], args)
    broken = TrackArgs(max_tracks=T)
    broken.min_hits = 0  # past the constructor's check
    with pytest.raises(L.MoEKernelError):
        L.track_sweep(state, boxes, scores, labels, None, tab[0], tab[1], [broken] * G)
    assert not L.launch_counts()
    assert "rtdetr_track_sweep" in L.SIGNATURES and L.PROF_KINDS[22] == "track_sweep"


def test_sweep_on_the_gpu_equals_the_cpu_end_to_end(hip_lib, tmp_path, monkeypatch):
    from scripts import tune_tracker
    from src.moe import _lib as L
    from src.rtdetr_moe import tune

    c = case(65, 2)
    base = {"max_tracks": 64}
    want = tune.sweep(c["dets"], c["gt"], GRID16, base=base, hota=True, device="cpu")
    L.launch_counts(reset=True)
    got = tune.sweep(c["dets"], c["gt"], GRID16, base=base, hota=True, device=DEV)
    counts = L.launch_counts(reset=True)
    assert counts.get("track_sweep") == 1 and counts.get("mot_eval", 0) >= 1 and counts.get("hota", 0) >= 3, counts
    assert got == want
    assert len({json.dumps(m["COMBINED"]) for m in got["metrics"]}) >= 8
    monkeypatch.setenv("MOE_TRACK_SWEEP", "0")
    off = tune.sweep(c["dets"], c["gt"], GRID16, base=base, hota=True, device=DEV)
    assert "track_sweep" not in L.launch_counts(reset=True) and off == want
    monkeypatch.delenv("MOE_TRACK_SWEEP")
    # the command line, on files
    (tmp_path / "det").mkdir()
    (tmp_path / "det" / (KEY + ".txt")).write_text(tune.det_lines(c["dets"][KEY]))
    (tmp_path / "gt" / KEY / "gt").mkdir(parents=True)
    lines = [f"{f},{int(i)},{float(b[0])!r},{float(b[1])!r},{float(b[2]) - float(b[0])!r},{float(b[3]) - float(b[1])!r},"
             f"1,1,1\n" for f, (boxes, ids, _) in c["gt"][KEY].items() for b, i in zip(boxes, ids)]
    (tmp_path / "gt" / KEY / "gt" / "gt.txt").write_text("".join(lines))
    res = tune_tracker.main(["--det", str(tmp_path / "det"), "--gt", str(tmp_path / "gt"), "--grid", json.dumps(GRID16),
                             "--tracker", json.dumps(base), "--hota", "--device", "0", "--out", str(tmp_path / "out"),
                             "--write-best"])
    assert L.launch_counts(reset=True).get("track_sweep") == 2  # the sweep, and the best configuration's tracks
    saved = json.loads((tmp_path / "out" / "tracker_sweep.json").read_text())
    assert saved["best"] == res["best"] == want["best"]
    assert saved["configs"][saved["best"]]["max_tracks"] == 64
    # the whole file is the CPU's sweep of the same files (the ground truth's text rounds its widths once more)
    from src.rtdetr_moe import moteval

    files = tune.sweep(tune.load_det(tmp_path / "det", [KEY]), moteval.load_gt(tmp_path / "gt", [KEY]), GRID16,
                       base=base, hota=True, device="cpu")
    assert saved == json.loads(json.dumps(files))
    best = tune.track_sweep_reference(c["dets"], [tune.expand_grid(GRID16, base)[want["best"]]], 64)[0][KEY]
    text = (tmp_path / "out" / "mot" / (KEY + ".txt")).read_text()
    assert text == tune.mot_text(best, c["dets"][KEY]) and len(text.splitlines()) == int(best["count"].sum()) >= 215
