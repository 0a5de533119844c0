"""motion.shift_reference / sequence_shifts on the CPU: the estimator finds the
shift that was put in, the gate refuses frames without structure, and a batch
may be cut into launches anywhere."""
from __future__ import annotations

import numpy as np
import pytest

from motion_cases import SHIFTS, cumulative, noise_frames, scene, view, views


def _m():
    from src.rtdetr_moe import motion

    return motion


@pytest.mark.parametrize("shift", SHIFTS)
def test_the_shift_put_in_is_found(shift):
    sc = scene(96 + 160, 160 + 160, seed=3)
    prev, cur = view(sc, 96, 160, 0, 0, seed=1), view(sc, 96, 160, *shift, seed=2)
    got, status, sads = _m().shift_reference(cur, prev, 12, 100, (0.0, 1.0))
    assert (got, status) == (shift, 1), (got, status, sads)
    assert sads[1] <= sads[0] and sads[2] > 0  # coarse sums on the coarse image, the fine one on the grey image


def test_full_size_at_the_default_radius():
    sc = scene(704 + 160, 1248 + 160, seed=4)
    prev, cur = view(sc, 704, 1248, 0, 0, seed=1), view(sc, 704, 1248, 37, -5, seed=2)
    got, status, _ = _m().shift_reference(cur, prev, 48, 100, (0.0, 1.0))
    assert (got, status) == ((37, -5), 1)


@pytest.mark.parametrize("kind", ["uniform", "dark"])
def test_the_gate_refuses_noise(kind):
    prev, cur = noise_frames(96, 160, kind)
    got, status, sads = _m().shift_reference(cur, prev, 12, 100, (0.0, 1.0))
    assert (got, status) == ((0, 0), 2) and sads[2] == 0 and sads[1] <= sads[0], (got, status, sads)
    open_, status, _ = _m().shift_reference(cur, prev, 12, 0, (0.0, 1.0))
    assert status == 1 and open_ != (0, 0), open_  # without the gate the noise picks a shift


def test_flat_frames_tie_to_zero_and_small_frames_have_no_estimate():
    flat = np.full((96, 160, 3), 0.5, np.float32)
    assert _m().shift_reference(flat, flat, 12, 100, (0.0, 1.0)) == ((0, 0), 1, (0, 0, 0))
    small = scene(30, 40)
    assert _m().shift_reference(small, small, 12, 100, (0.0, 1.0)) == ((0, 0), 0, (0, 0, 0))
    # 40 rows (and 40 columns) at radius 4 are the fewest with a window: 10 coarse pixels less one a side
    assert _m().shift_reference(scene(40, 56), scene(40, 56), 4, 100)[1] == 1
    assert _m().shift_reference(scene(39, 56), scene(39, 56), 4, 100)[1] == 0
    assert _m().shift_reference(scene(40, 40), scene(40, 40), 4, 100)[1] == 1
    assert _m().shift_reference(scene(40, 39), scene(40, 39), 4, 100)[1] == 0


def test_grey_and_coarse_are_the_stated_integers():
    m = _m()
    img = np.array([[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, 0.25, 0.75], [-1.0, 2.0, float("nan")]]], np.float32)
    q = [[0, 0, 0], [255, 255, 255], [128, 64, 191], [0, 255, 0]]  # int(v * 255 + 0.5), clamped; NaN -> 0
    want = [(77 * r + 150 * g + 29 * b + 128) >> 8 for r, g, b in q]
    assert m.grey_u8(img).tolist() == [want] and m.grey_u8(img).dtype == np.uint8
    g = np.arange(9 * 10, dtype=np.uint8).reshape(9, 10)
    c = m.coarse_u8(g)
    assert c.shape == (2, 2) and int(c[1, 1]) == (int(g[4:8, 4:8].astype(int).sum()) + 8) >> 4


STEPS = [(0, 0), (5, -3), (-8, 2), (0, 0), (12, 7), (-4, -4), (3, 0), (0, 9), (-11, 1), (3, 2)]


def _batch(seed=5, steps=STEPS):
    return views(96, 160, cumulative(steps), seed=seed)


def _run(images, slots, resets, chunks, S=2, **kw):
    m = _m()
    state = m.new_motion_state(S, *images.shape[1:3])
    shift, info = np.zeros((len(images), 2), np.int32), np.zeros((len(images), 4), np.int32)
    for part in chunks:
        shift[part], info[part] = m.sequence_shifts(images[part], np.asarray(slots)[part], np.asarray(resets)[part],
                                                    state, 12, 100, **kw)
    return shift, info, state


def test_any_split_into_launches_gives_the_same_shifts():
    images = _batch()
    F = len(images)
    slots, resets = [0] * F, [1] + [0] * (F - 1)
    whole = _run(images, slots, resets, [slice(0, F)])
    assert whole[0].tolist() == [[0, 0]] + [list(s) for s in STEPS[1:]]
    assert whole[1][:, 0].tolist() == [0] + [1] * (F - 1)
    for chunks in ([slice(0, 1), slice(1, F)], [slice(0, 4), slice(4, 5), slice(5, F)],
                   [slice(f, f + 1) for f in range(F)]):
        part = _run(images, slots, resets, chunks)
        assert np.array_equal(part[0], whole[0]) and np.array_equal(part[1], whole[1])
        assert np.array_equal(part[2]["grey"], whole[2]["grey"]) and np.array_equal(part[2]["valid"], whole[2]["valid"])
    assert whole[2]["valid"].tolist() == [1, 0]
    assert np.array_equal(whole[2]["grey"][0], _m().grey_u8(images[-1]))


def test_reset_interleaved_slots_and_a_slot_out_of_range():
    a, b = _batch(seed=6), _batch(seed=7, steps=[(-s[0], s[1]) for s in STEPS])
    # slot 0: a's frames; slot 1: b's; frame 4 belongs to nobody; slot 0 is reset at a's frame 3
    order = [("a", 0), ("b", 0), ("a", 1), ("b", 1), ("x", 0), ("a", 2), ("a", 3), ("b", 2), ("a", 4)]
    images = np.stack([{"a": a, "b": b, "x": a}[k][f] for k, f in order])
    slots = [{"a": 0, "b": 1, "x": 7}[k] for k, _ in order]
    resets = [int((k, f) in (("a", 0), ("b", 0), ("a", 3))) for k, f in order]
    shift, info, state = _run(images, slots, resets, [slice(0, len(order))])
    want = []
    for k, f in order:
        if k == "x" or f == 0 or (k, f) == ("a", 3):
            want.append([0, 0])
        else:
            want.append([STEPS[f][0] * (1 if k == "a" else -1), STEPS[f][1]])
    assert shift.tolist() == want
    assert info[:, 0].tolist() == [0 if w == [0, 0] and (k == "x" or f == 0 or (k, f) == ("a", 3)) else 1
                                   for w, (k, f) in zip(want, order)]
    assert state["valid"].tolist() == [1, 1]
    assert np.array_equal(state["grey"][0], _m().grey_u8(a[4])) and np.array_equal(state["grey"][1],
                                                                                   _m().grey_u8(b[2]))
    two = _run(images, slots, resets, [slice(0, 3), slice(3, len(order))])
    assert np.array_equal(two[0], shift) and np.array_equal(two[1], info)


def test_rows_keep_the_window_off_a_static_bottom():
    h, w = 160, 160
    sc = scene(h + 160, w + 160, seed=8)
    prev, cur = view(sc, h, w, 0, 0, seed=1), view(sc, h, w, 9, -6, seed=2)
    cur[107:] = prev[107:]  # the bonnet: the bottom third does not move
    m = _m()
    assert m.shift_reference(cur, prev, 12, 100, (0.0, 0.6))[:2] == ((9, -6), 1)
    assert m.shift_reference(cur, prev, 12, 100, (0.7, 1.0))[:2] == ((0, 0), 1)
    with pytest.raises(ValueError):
        m.shift_reference(cur, prev, 12, 100, (0.6, 0.6))
    for radius in (0, 6, 68):
        with pytest.raises(ValueError):
            m.shift_reference(cur, prev, radius, 100)
    with pytest.raises(ValueError):
        m.shift_reference(cur, prev, 12, 1000)
