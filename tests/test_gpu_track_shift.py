"""rtdetr_track_update_shift (_lib.track_update(shift=...)) against
track.track_reference(shift=...): ids, boxes as bits, count and the whole state,
exactly; with NULL it is rtdetr_track_update bit for bit."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from motion_cases import pan_sequence, run_reference_shift
from track_cases import draw_sequence, identities

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _launch(L, state, seq, frames, args, shift, slots=None, resets=None):
    t = lambda key, dt: torch.from_numpy(np.ascontiguousarray(seq[key][frames])).to(dt).to(DEV)  # noqa: E731
    F, K = seq["scores"][frames].shape
    out = (torch.full((F, K), 12345, dtype=torch.int32, device=DEV), torch.full((F, K, 4), float("nan"), device=DEV),
           torch.full((F,), 999, dtype=torch.int32, device=DEV))
    tab = lambda v: torch.tensor(v if v is not None else [0] * F, dtype=torch.int32, device=DEV)  # noqa: E731
    sh = None if shift is None else torch.from_numpy(np.ascontiguousarray(shift[frames], np.float32)).to(DEV)
    got = L.track_update(state, t("boxes", torch.float32), t("scores", torch.float32), t("labels", torch.int32),
                         t("n_valid", torch.int32), tab(slots), tab(resets), args, out=out, shift=sh)
    return tuple(o.cpu().numpy() for o in got)


def _same(got, ref, frames):
    oid, obox, cnt = got
    assert np.array_equal(cnt, ref["count"][frames]), (cnt.tolist(), ref["count"][frames].tolist())
    assert np.array_equal(oid, ref["out_id"][frames]), np.argwhere(oid != ref["out_id"][frames])[:8].tolist()
    a, b = obox.view(np.int32), np.ascontiguousarray(ref["out_box"][frames]).view(np.int32)
    assert np.array_equal(a, b), np.argwhere(a != b)[:8].tolist()


def test_the_pan_case(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackArgs, TrackState, states_equal

    seq, shifts = pan_sequence()
    args = TrackArgs()
    ref = run_reference_shift(seq, args, args.max_tracks, shifts)
    ids, switches = identities(seq, ref["out_id"])
    assert all(len(v) == 1 for v in ids.values()) and switches == 0 and int(ref["count"].sum()) == 152
    for chunks in ([slice(0, 20)], [slice(0, 7), slice(7, 8), slice(8, 20)]):
        state = TrackState(1, args.max_tracks, DEV)
        L.launch_counts(reset=True)
        for part in chunks:
            _same(_launch(L, state, seq, part, args, shifts), ref, part)
        assert L.launch_counts(reset=True) == {"track": len(chunks)}
        assert states_equal(state.export(0), ref["state"])
    # without the shift the kernel loses the tracks as the reference does
    bare = run_reference_shift(seq, args, args.max_tracks, None)
    state = TrackState(1, args.max_tracks, DEV)
    _same(_launch(L, state, seq, slice(0, 20), args, None), bare, slice(0, 20))
    assert identities(seq, bare["out_id"])[1] > 0


@pytest.mark.parametrize("K,T,seed", [(65, 64, 2), (300, 256, 6), (5, 4, 1)])
def test_random_shifts_on_the_noisy_case(hip_lib, K, T, seed):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackArgs, TrackState, states_equal

    F = 24
    seq = draw_sequence(20, F, K, seed=seed, jitter=2.0, miss=0.12, low_share=0.2, fp=min(3, K // 8), leave={0: 12})
    rng = np.random.default_rng(seed)
    shifts = (rng.normal(0, 6.0, (F, 2)) * (rng.random((F, 1)) < 0.7)).astype(np.float32)  # some frames exactly 0
    args = TrackArgs(max_age=3, max_tracks=T)
    ref = run_reference_shift(seq, args, T, shifts)
    assert int(ref["count"].sum()) >= 20 and (shifts == 0).all(1).any() and (shifts != 0).all(1).any()
    state = TrackState(2, T, DEV)
    untouched = state.export(0)
    # slot 1 of two; in two launches
    for part in (slice(0, 9), slice(9, F)):
        n = len(range(*part.indices(F)))
        _same(_launch(L, state, seq, part, args, shifts, slots=[1] * n), ref, part)
    assert states_equal(state.export(1), ref["state"]) and states_equal(state.export(0), untouched)
    assert not states_equal(ref["state"], run_reference_shift(seq, args, T, None)["state"])  # the shifts mattered


def test_null_is_rtdetr_track_update_bit_for_bit(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe.track import TrackArgs, TrackState

    seq = draw_sequence(20, 24, 65, seed=2, jitter=2.0, miss=0.12, low_share=0.2, fp=3, leave={0: 12})
    args = TrackArgs(max_age=3)
    t = lambda key, dt: torch.from_numpy(seq[key]).to(dt).to(DEV)  # noqa: E731
    ops = (t("boxes", torch.float32), t("scores", torch.float32), t("labels", torch.int32), t("n_valid", torch.int32))
    tab = torch.zeros(24, dtype=torch.int32, device=DEV)
    states, outs = [], []
    for entry in ("rtdetr_track_update", "rtdetr_track_update_shift"):
        state = TrackState(1, args.max_tracks, DEV)
        out = (torch.empty((24, 65), dtype=torch.int32, device=DEV), torch.empty((24, 65, 4), device=DEV),
               torch.empty(24, dtype=torch.int32, device=DEV))
        common = (*(o.data_ptr() for o in ops), tab.data_ptr(), tab.data_ptr(), 24, 65, 1, args.max_tracks,
                  args.track_high, args.track_low, args.new_thr, args.match_iou, args.second_iou, args.max_age,
                  args.min_hits, args.alpha, args.beta, 0, *(x.data_ptr() for x in state.tensors()),
                  *(o.data_ptr() for o in out))
        extra = (None,) if entry.endswith("_shift") else ()
        assert getattr(L.lib(), entry)(*common, *extra, None) == 0, L.lib().moe_last_error()
        torch.cuda.synchronize()
        states.append([x.cpu() for x in state.tensors()])
        outs.append([o.cpu() for o in out])
    assert int(outs[0][2].sum()) >= 100
    for a, b in zip(states[0] + outs[0], states[1] + outs[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the refusals are the same function's
    assert L.lib().rtdetr_track_update_shift(*common[:6], 24, 1025, *common[8:], None, None) != 0
    assert "rtdetr_track_update_shift" in L.lib().moe_last_error().decode()
