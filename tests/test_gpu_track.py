"""rtdetr_track_update (_lib.track_update) against track.track_reference: out_id,
out_boxes (as bits), count and the whole state after the launch, exactly (no
tolerance: the kernel restates the reference's fp32 arithmetic operation by
operation, and its greedy association takes the reference's pairs in the
reference's order).  The outputs are pre-filled with garbage."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from track_cases import check_hand_case, draw_sequence, hand_cases, run_reference

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

# (K, T, F, objects, n_valid mode, seed): K on both sides of a wave and of the 256-thread stride, at 1 and at the
# limit; T = 1, 4 (fewer slots than objects), one wave, four waves; F = 1, 2, 16, 40.  max_age = 3 everywhere, so
# that slots expire within 40 frames.  Seeds tuned on the CPU reference for the preconditions below.
SHAPES = [
    (1, 1, 16, 1, "null", 0),
    (5, 4, 16, 8, "given", 1),
    (63, 64, 40, 20, "given", 2),
    (64, 64, 16, 20, "null", 3),
    (65, 256, 40, 30, "partial", 4),
    (65, 64, 1, 20, "given", 5),
    (65, 64, 16, 20, "zero", 5),
    (300, 64, 16, 40, "given", 6),
    (300, 256, 2, 40, "null", 7),
    (300, 4, 40, 8, "partial", 8),
    (1024, 256, 16, 60, "given", 9),
    (1024, 1, 2, 3, "null", 10),
]
# every combination of the options at K = 65 (two labels, so that class_agnostic matters)
OPTIONS = [dict(class_agnostic=a, min_hits=h, match_iou=m, **({"track_low": 0.5} if off else {}))
           for a in (False, True) for h in (1, 2) for m in (0.0, 0.2) for off in (False, True)]


def _args(**kw):
    from src.rtdetr_moe.track import TrackArgs

    return TrackArgs(**{"max_age": 3, **kw})


def _draw(K, F, objects, seed, n_labels=1):
    return draw_sequence(objects, F, K, seed=seed, jitter=2.0, miss=0.12, low_share=0.2, fp=min(3, max(K // 8, 0)),
                         leave={0: F // 2} if F >= 16 else None, n_labels=n_labels)


def _n_valid(seq, mode):
    if mode == "null":
        return None
    if mode == "zero":
        return np.zeros_like(seq["n_valid"])
    nv = seq["n_valid"].copy()
    if mode == "partial":
        nv[1::3] = nv[1::3] // 2  # every third frame loses its weaker half
        nv[2::7] = 10 ** 6        # clamped to K
        nv[5::11] = -4            # clamped to 0
    return nv


def _garbage(F, K):
    return (torch.full((F, K), 12345, dtype=torch.int32, device=DEV),
            torch.full((F, K, 4), float("nan"), device=DEV), torch.full((F,), 999, dtype=torch.int32, device=DEV))


def _launch(L, state, seqs, order, slots, resets, nvs, args):
    """One launch over the frames ``order`` = [(sequence number, frame)], -> numpy (out_id, out_box, count)."""
    t = lambda key, dt: torch.from_numpy(np.stack([seqs[q][key][f] for q, f in order])).to(dt).to(DEV)  # noqa: E731
    boxes, scores, labels = t("boxes", torch.float32), t("scores", torch.float32), t("labels", torch.int32)
    nv = None
    if nvs is not None:
        nv = torch.tensor([int(nvs[q][f]) for q, f in order], dtype=torch.int32, device=DEV)
    F, K = scores.shape
    out = L.track_update(state, boxes, scores, labels, nv, torch.tensor(slots, dtype=torch.int32, device=DEV),
                         torch.tensor(resets, dtype=torch.int32, device=DEV), args, out=_garbage(F, K))
    return tuple(o.cpu().numpy() for o in out)


def _same(got, ref, frames=None):
    oid, obox, cnt = got
    sel = slice(None) if frames is None else frames
    assert np.array_equal(cnt, ref["count"][sel]), (cnt.tolist(), ref["count"][sel].tolist())
    assert np.array_equal(oid, ref["out_id"][sel]), np.argwhere(oid != ref["out_id"][sel])[:8].tolist()
    a, b = obox.view(np.int32), np.ascontiguousarray(ref["out_box"][sel]).view(np.int32)
    assert np.array_equal(a, b), np.argwhere(a != b)[:8].tolist()


def _preconditions(e, K, T, F, mode, args):
    """Asserted on the reference before the GPU is touched: the comparison must not pass on nothing."""
    print(e)
    if mode == "zero":
        assert e["reported"] == 0 and e["births"] == 0
        return
    assert e["births"] >= 1 and (F == 1 and args.min_hits > 1 or e["reported"] >= 1)
    if F >= 16 and K >= 63 and T >= 64:
        assert e["refound"] >= 1 and e["tentative_freed"] >= (1 if args.min_hits > 1 else 0)
        assert (e["stage2"] >= 1) == (args.track_low < args.track_high)
    if F == 40:
        assert e["expired"] >= 1
    if T == 4:
        assert e["dropped"] >= 1


@pytest.mark.parametrize("K,T,F,objects,mode,seed", SHAPES)
def test_drawn_sequences(hip_lib, K, T, F, objects, mode, seed):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackState, states_equal

    args = _args(max_tracks=T)
    seq = _draw(K, F, objects, seed)
    nv = _n_valid(seq, mode)
    ref = run_reference(seq, args, T, n_valid=nv)
    _preconditions(ref["events"], K, T, F, mode, args)
    state = TrackState(1, T, DEV)
    start = state.snapshot()
    got = _launch(L, state, [seq], [(0, f) for f in range(F)], [0] * F, [0] * F, None if nv is None else [nv], args)
    _same(got, ref)
    assert states_equal(state.export(0), ref["state"])
    # a relaunch from the restored state gives the same bits
    end = state.snapshot()
    state.restore(start)
    again = _launch(L, state, [seq], [(0, f) for f in range(F)], [0] * F, [0] * F, None if nv is None else [nv], args)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, again))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(state.snapshot(), end))


@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_option_grid(hip_lib, opt):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackState, states_equal

    K, T, F = 65, 64, 16
    args = _args(max_tracks=T, **opt)
    seq = _draw(K, F, 20, 11, n_labels=2)
    seq["labels"][:, ::2] ^= 1  # a detector that is unsure of the class: only class_agnostic keeps those tracks
    ref = run_reference(seq, args, T)
    _preconditions(ref["events"], K, T, F, "given", args)
    state = TrackState(1, T, DEV)
    got = _launch(L, state, [seq], [(0, f) for f in range(F)], [0] * F, [0] * F, [seq["n_valid"]], args)
    _same(got, ref)
    assert states_equal(state.export(0), ref["state"])


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c["name"])
def test_hand_cases(hip_lib, case):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackState, states_equal

    args = _args(max_tracks=case["T"], **case["args"])
    seq = case["seq"]
    ref = run_reference(seq, args, case["T"])
    assert (ref["events"]["ties"] >= 1) == (case["ties"] >= 1)
    F = seq["scores"].shape[0]
    state = TrackState(1, case["T"], DEV)
    got = _launch(L, state, [seq], [(0, f) for f in range(F)], [0] * F, [0] * F, [seq["n_valid"]], args)
    check_hand_case(case, dict(out_id=got[0]))
    _same(got, ref)
    assert states_equal(state.export(0), ref["state"])


def test_chunk_invariance(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackState, states_equal

    K, T, F = 300, 64, 16
    args = _args(max_tracks=T)
    seq = _draw(K, F, 40, 6)
    ref = run_reference(seq, args, T)
    assert ref["events"]["stage2"] >= 1 and ref["events"]["refound"] >= 1
    for chunks in ([range(16)], [range(1), range(1, 16)], [range(f, f + 1) for f in range(16)]):
        state = TrackState(1, T, DEV)
        parts = [_launch(L, state, [seq], [(0, f) for f in c], [0] * len(c), [0] * len(c), [seq["n_valid"]], args)
                 for c in chunks]
        _same(tuple(np.concatenate([p[j] for p in parts]) for j in range(3)), ref)
        assert states_equal(state.export(0), ref["state"])


def test_three_sequences_interleaved_and_an_idle_slot(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackState, states_equal

    K, T = 65, 64
    args = _args(max_tracks=T)
    seqs = [_draw(K, F, 20, 20 + q) for q, F in enumerate((8, 6, 4))]
    refs = [run_reference(s, args, T) for s in seqs]
    assert all(r["events"]["reported"] >= 10 for r in refs)
    order = [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (2, 1), (1, 2), (0, 3), (0, 4), (2, 2), (1, 3), (1, 4),
             (2, 3), (0, 5), (1, 5), (0, 6), (0, 7)]
    slot_of = {0: 3, 1: 0, 2: 2}  # slot 1 has no frames
    state = TrackState(4, T, DEV)
    state.load(1, refs[0]["state"])  # somebody's tracks, which must stay as they are
    idle = state.export(1)
    got = _launch(L, state, seqs, order, [slot_of[q] for q, _ in order], [0] * len(order),
                  [s["n_valid"] for s in seqs], args)
    for q, ref in enumerate(refs):
        rows = [i for i, (qq, _) in enumerate(order) if qq == q]
        _same(tuple(g[rows] for g in got), ref)
        assert states_equal(state.export(slot_of[q]), ref["state"])
    assert states_equal(state.export(1), idle) and states_equal(idle, refs[0]["state"])


def test_frame_reset_mid_launch_equals_a_fresh_state(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackState, states_equal

    K, T = 65, 64
    args = _args(max_tracks=T)
    a, b = _draw(K, 5, 20, 30), _draw(K, 6, 20, 31)
    ref_a, ref_b = run_reference(a, args, T), run_reference(b, args, T)
    assert ref_a["state"]["next_id"] > 5 and ref_b["events"]["reported"] >= 10
    state = TrackState(1, T, DEV)
    order = [(0, f) for f in range(5)] + [(1, f) for f in range(6)]
    got = _launch(L, state, [a, b], order, [0] * 11, [0] * 5 + [1] + [0] * 5, [a["n_valid"], b["n_valid"]], args)
    _same(tuple(g[:5] for g in got), ref_a)
    _same(tuple(g[5:] for g in got), ref_b)
    assert states_equal(state.export(0), ref_b["state"])
    # a reset on the launch's first frame: the stale state is never read
    got = _launch(L, state, [b], [(0, f) for f in range(6)], [0] * 6, [1] + [0] * 5, [b["n_valid"]], args)
    _same(got, ref_b)
    assert states_equal(state.export(0), ref_b["state"])


def test_out_of_range_slot_gives_empty_rows_and_no_state_change(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackState, states_equal

    K, T = 65, 64
    args = _args(max_tracks=T)
    seq = _draw(K, 6, 20, 32)
    ref = run_reference(seq, args, T, chunks=[[0, 2, 3]])
    state = TrackState(2, T, DEV)
    before = state.export(1)
    got = _launch(L, state, [seq], [(0, f) for f in range(6)], [0, -1, 0, 0, 2, 1 << 20], [0] * 6, [seq["n_valid"]],
                  args)
    _same(tuple(g[[0, 2, 3]] for g in got), ref, frames=[0, 2, 3])
    for f in (1, 4, 5):
        assert got[2][f] == 0 and (got[0][f] == -1).all() and not got[1][f].view(np.int32).any()
    assert states_equal(state.export(0), ref["state"]) and states_equal(state.export(1), before)


def test_empty_launches(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackState, new_state, states_equal

    args = _args(max_tracks=4)
    state = TrackState(1, 4, DEV)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)  # noqa: E731
    L.launch_counts(reset=True)
    out = L.track_update(state, z(0, 8, 4), z(0, 8), z(0, 8, dt=torch.int32), None, z(0, dt=torch.int32),
                         z(0, dt=torch.int32), args)
    assert tuple(out[0].shape) == (0, 8) and not L.launch_counts()  # F == 0: no launch
    # K == 0: the frames still age the tracks
    seq = draw_sequence(2, 2, 4, seed=1)
    ref = run_reference(seq, args, 4)
    _launch(L, state, [seq], [(0, 0), (0, 1)], [0, 0], [0, 0], [seq["n_valid"]], args)
    assert states_equal(state.export(0), ref["state"]) and (ref["state"]["hits"] == 2).sum() == 2
    out = L.track_update(state, z(5, 0, 4), z(5, 0), z(5, 0, dt=torch.int32), None, z(5, dt=torch.int32),
                         z(5, dt=torch.int32), args)
    assert out[2].tolist() == [0] * 5
    assert states_equal(state.export(0), new_state(4) | {"next_id": 3})  # max_age 3: expired after four empty frames
    assert L.launch_counts(reset=True) == {"track": 2}


def test_bad_arguments_return_an_error_without_a_launch(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackState

    F, K, T = 2, 8, 4
    state = TrackState(1, T, DEV)
    boxes, scores = torch.zeros((F, K, 4), device=DEV), torch.zeros((F, K), device=DEV)
    labels = torch.zeros((F, K), dtype=torch.int32, device=DEV)
    tab = torch.zeros((2, F), dtype=torch.int32, device=DEV)
    out = _garbage(F, K)
    before = [t.clone() for t in (*out, *state.tensors())]
    st = torch.cuda.current_stream().cuda_stream
    nan = float("nan")
    ptr = dict(boxes=boxes, scores=scores, labels=labels, slot=tab[0], reset=tab[1], tbox=state.box,
               tscore=state.score, tmeta=state.meta, seq=state.seq, oid=out[0], obox=out[1], count=out[2])
    ptr = {k: v.data_ptr() for k, v in ptr.items()}

    def call(F=F, K=K, S=1, T=T, high=0.5, low=0.1, new=0.6, m1=0.2, m2=0.5, max_age=30, min_hits=2, alpha=0.5,
             beta=0.25, **p):
        q = {**ptr, **p}
        return hip_lib.rtdetr_track_update(q["boxes"], q["scores"], q["labels"], None, q["slot"], q["reset"], F, K, S,
                                           T, high, low, new, m1, m2, max_age, min_hits, alpha, beta, 0, q["tbox"],
                                           q["tscore"], q["tmeta"], q["seq"], q["oid"], q["obox"], q["count"], st)

    L.launch_counts(reset=True)
    bad = [dict(K=1025), dict(T=257), dict(T=0), dict(F=1025), dict(S=1025), dict(S=0), dict(K=-1), dict(F=-1),
           dict(high=nan), dict(low=nan), dict(new=nan), dict(m1=nan), dict(m2=nan), dict(alpha=nan), dict(beta=nan),
           dict(max_age=-1), dict(min_hits=0), dict(boxes=ptr["boxes"] + 4), dict(obox=ptr["obox"] + 4)]
    bad += [{k: None} for k in ptr]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert hip_lib.moe_last_error().decode().startswith("rtdetr_track_update"), kw
    torch.cuda.synchronize()
    assert not L.launch_counts()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32))
               for a, b in zip((*out, *state.tensors()), before))
    assert call() == 0
    torch.cuda.synchronize()
    assert L.launch_counts(reset=True) == {"track": 1}
    # the typed wrapper refuses what the C entry cannot see
    args = _args(max_tracks=T)
    with pytest.raises(L.MoEKernelError):
        L.track_update(state, boxes, scores, labels.long(), None, tab[0], tab[1], args)
    with pytest.raises(L.MoEKernelError):
        L.track_update(state, boxes, scores[:, :7], labels, None, tab[0], tab[1], args)
    with pytest.raises(L.MoEKernelError):
        L.track_update(state, boxes, scores, labels, None, tab[0, :1], tab[1], args)
    with pytest.raises(L.MoEKernelError):
        L.track_update(state, boxes, scores, labels, None, tab[0].cpu(), tab[1], args)
    assert not L.launch_counts()
    assert "rtdetr_track_update" in L.SIGNATURES and L.PROF_KINDS[20] == "track"
