"""rtdetr_frame_shift (_lib.frame_shift) against motion.sequence_shifts: the
shifts, the status and the three SADs of every frame and the exported state,
exactly (integer arithmetic from the first step on: no tolerance).  The padding
of the model's input holds garbage, and so do the outputs before the launch."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from motion_cases import SHIFTS, cumulative, noise_frames, views

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _upload(images, pad_hw):
    """fp32 [F, h, w, 3] -> the model's input: channels-last [F, 3, pad_h, pad_w], the padding 0.77."""
    F, h, w, _ = images.shape
    full = np.full((F, pad_hw[0], pad_hw[1], 3), 0.77, np.float32)
    full[:, :h, :w] = images
    return torch.from_numpy(full).to(DEV).permute(0, 3, 1, 2)


def _compare(images, pad_hw, slots, resets, chunks, S, radius, gate=0.1, rows=(0.0, 1.0), start=None):
    """The launches ``chunks`` (slices of the frames) on the GPU and on the host -> the reference's (shift, info)."""
    from src.moe import _lib as L
    from src.rtdetr_moe import motion

    F, h, w, _ = images.shape
    ref = motion.new_motion_state(S, h, w) if start is None else {k: v.copy() for k, v in start.items()}
    state = motion.MotionState(S, h, w, DEV, frames=1)  # grows with the launches
    if start is not None:
        state.load(start)
    slots, resets = np.asarray(slots, np.int32), np.asarray(resets, np.int32)
    want_s, want_i = np.zeros((F, 2), np.int32), np.zeros((F, 4), np.int32)
    for part in chunks:
        want_s[part], want_i[part] = motion.sequence_shifts(images[part], slots[part], resets[part], ref, radius,
                                                            round(1000 * gate), rows)
        n = len(slots[part])
        out = (torch.full((n, 2), 12345, dtype=torch.int32, device=DEV),
               torch.full((n, 4), -777, dtype=torch.int32, device=DEV))
        tabs = (torch.from_numpy(slots[part]).to(DEV), torch.from_numpy(resets[part]).to(DEV))
        got_s, got_i = L.frame_shift(state, _upload(images[part], pad_hw), (h, w), *tabs, radius, gate, rows, out=out)
        assert np.array_equal(got_i.cpu().numpy(), want_i[part]), (got_i.cpu().tolist(), want_i[part].tolist())
        assert np.array_equal(got_s.cpu().numpy(), want_s[part]), (got_s.cpu().tolist(), want_s[part].tolist())
        exp = state.export()
        assert np.array_equal(exp["valid"], ref["valid"]), (exp["valid"], ref["valid"])
        assert np.array_equal(exp["grey"], ref["grey"]), np.argwhere(exp["grey"] != ref["grey"])[:8].tolist()
    return want_s, want_i, ref


def test_the_smallest_size_with_a_window(hip_lib):
    images = views(40, 56, cumulative([(0, 0), (3, -2)]), seed=1)
    # F = 1 twice: the first frame finds no stored image (prev_valid 0), the second the first
    s, i, _ = _compare(images, (64, 64), [0, 0], [0, 0], [slice(0, 1), slice(1, 2)], 1, 4)
    assert i[:, 0].tolist() == [0, 1] and s[1].tolist() == [3, -2]
    # a row or a column fewer: no window, status 0, and the state is stored all the same
    for h, w in ((39, 56), (40, 39), (30, 40)):
        s, i, ref = _compare(views(h, w, [(0, 0), (1, 1)], seed=2), (64, 64), [0, 0], [0, 0], [slice(0, 2)], 1, 4)
        assert not i.any() and not s.any() and ref["valid"].tolist() == [1]


@pytest.mark.parametrize("pad_hw", [(96, 128), (70, 103)], ids=["vector_loads", "scalar_loads"])
def test_remainders_interleaved_slots_reset_and_a_slot_out_of_range(hip_lib, pad_hw):
    steps = [(0, 0), (5, -3), (-8, 2), (7, 7), (-2, -9)]
    a, b, c = (views(70, 101, cumulative(steps), seed=s) for s in (3, 4, 5))
    # S = 4: slots 0, 2 and 3 interleaved, slot 1 idle (loaded as valid: it must stay as it is); a frame of nobody's
    # (slot 9, slot -1); slot 2 is reset at its third frame
    order = [(a, 0, 0), (b, 0, 2), (c, 0, 3), (a, 1, 0), (a, 0, 9), (b, 1, 2), (c, 1, 3), (b, 2, 2), (a, 2, 0),
             (b, 3, 2), (c, 2, -1), (c, 2, 3), (a, 3, 0), (b, 4, 2), (c, 3, 3), (a, 4, 0)]
    images = np.stack([src[f] for src, f, _ in order])
    slots = [s for _, _, s in order]
    resets = [int(src is b and f == 2) for src, f, _ in order]
    from src.rtdetr_moe import motion

    start = motion.new_motion_state(4, 70, 101)
    start["grey"][1], start["valid"][1] = 99, 1
    for chunks in ([slice(0, 16)], [slice(0, 5), slice(5, 16)], [slice(0, 1), slice(1, 3), slice(3, 8), slice(8, 16)]):
        s, i, ref = _compare(images, pad_hw, slots, resets, chunks, 4, 8, start=start)
        assert ref["valid"].tolist() == [1, 1, 1, 1] and (ref["grey"][1] == 99).all()
        for (src, f, slot), got, info in zip(order, s.tolist(), i.tolist()):
            known = 0 <= slot < 4 and f > 0 and not (src is b and f == 2)
            assert info[0] == int(known) and got == (list(steps[f]) if known else [0, 0]), (f, slot, got, info)


def test_the_cpu_list_of_shifts_in_one_launch_and_in_two(hip_lib):
    steps = SHIFTS + [(-x, -y) for x, y in SHIFTS]  # F = 16
    images = views(96, 160, cumulative(steps), seed=6)
    one = _compare(images, (96, 160), [0] * 16, [1] + [0] * 15, [slice(0, 16)], 1, 12)
    assert one[0].tolist() == [[0, 0]] + [list(s) for s in steps[1:]] and one[1][:, 0].tolist() == [0] + [1] * 15
    two = _compare(images, (96, 160), [0] * 16, [1] + [0] * 15, [slice(0, 7), slice(7, 16)], 1, 12)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    # a relaunch from a loaded state: the second half alone, from the reference's state after the first
    from src.rtdetr_moe import motion

    half = motion.new_motion_state(1, 96, 160)
    motion.sequence_shifts(images[:8], [0] * 8, [1] + [0] * 7, half, 12, 100)
    rest = _compare(images[8:], (96, 160), [0] * 8, [0] * 8, [slice(0, 8)], 1, 12, start=half)
    assert np.array_equal(rest[0], one[0][8:]) and np.array_equal(rest[1], one[1][8:])


def test_the_default_radius(hip_lib):
    images = views(320, 640, cumulative([(0, 0), (37, -5)]), seed=7)
    s, i, _ = _compare(images, (320, 640), [0, 0], [1, 0], [slice(0, 2)], 1, 48)
    assert s.tolist() == [[0, 0], [37, -5]] and i[:, 0].tolist() == [0, 1]


def test_ties_gated_frames_and_rows(hip_lib):
    flat = np.full((2, 96, 160, 3), 0.5, np.float32)
    s, i, _ = _compare(flat, (96, 160), [0, 0], [0, 0], [slice(0, 2)], 1, 12)
    assert s.tolist() == [[0, 0], [0, 0]] and i.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]]
    for kind in ("uniform", "dark"):
        frames = noise_frames(96, 160, kind)
        s, i, _ = _compare(frames, (96, 160), [0, 0], [0, 0], [slice(0, 2)], 1, 12)
        assert i[1, 0] == 2 and i[1, 3] == 0 and i[1, 1] > 0 and not s.any()
        s, i, _ = _compare(frames, (96, 160), [0, 0], [0, 0], [slice(0, 2)], 1, 12, gate=0.0)
        assert i[1, 0] == 1 and s[1].any()
    # a static bottom third: the rows above it give the top's shift, the rows inside it none
    moving = views(160, 160, cumulative([(0, 0), (9, -6)]), seed=8)
    moving[1, 107:] = moving[0, 107:]
    s, _, _ = _compare(moving, (160, 160), [0, 0], [0, 0], [slice(0, 2)], 1, 12, rows=(0.0, 0.6))
    assert s[1].tolist() == [9, -6]
    s, i, _ = _compare(moving, (160, 160), [0, 0], [0, 0], [slice(0, 2)], 1, 12, rows=(0.7, 1.0))
    assert s[1].tolist() == [0, 0] and i[1, 0] == 1
    _, i, _ = _compare(moving, (160, 160), [0, 0], [0, 0], [slice(0, 2)], 1, 12, rows=(0.9, 1.0))  # 4 coarse rows
    assert not i.any()


def test_three_launches_whatever_the_batch(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe import motion

    images = views(96, 160, [(0, 0)] * 16, seed=9)
    counts = []
    for F in (1, 16):
        state = motion.MotionState(1, 96, 160, DEV, frames=F)
        tab = torch.zeros(F, dtype=torch.int32, device=DEV)
        L.launch_counts(reset=True)
        L.frame_shift(state, _upload(images[:F], (96, 160)), (96, 160), tab, tab, 12, 0.1)
        counts.append(L.launch_counts(reset=True))
    assert counts[0] == counts[1] == {"motion": 3}, counts
    state = motion.MotionState(1, 96, 160, DEV)
    empty = torch.zeros(0, dtype=torch.int32, device=DEV)
    s, i = L.frame_shift(state, _upload(images[:0], (96, 160)), (96, 160), empty, empty)
    assert tuple(s.shape) == (0, 2) and tuple(i.shape) == (0, 4) and not L.launch_counts(reset=True)


def test_refusals_before_any_launch(hip_lib):
    from src.moe import _lib as L
    from src.rtdetr_moe import motion

    state = motion.MotionState(2, 96, 160, DEV)
    img = _upload(np.zeros((2, 96, 160, 3), np.float32), (96, 160))
    tab = torch.zeros(2, dtype=torch.int32, device=DEV)
    L.launch_counts(reset=True)
    for kw in (dict(radius=6), dict(radius=0), dict(radius=68), dict(gate=1.0), dict(gate=-0.1),
               dict(rows=(0.5, 0.5))):
        with pytest.raises(L.MoEKernelError):
            L.frame_shift(state, img, (96, 160), tab, tab, **kw)
    with pytest.raises(L.MoEKernelError):
        L.frame_shift(state, img, (96, 128), tab, tab)  # not the state's size
    with pytest.raises(L.MoEKernelError):
        L.frame_shift(state, img.contiguous(), (96, 160), tab, tab)  # not channels-last
    with pytest.raises(ValueError):
        motion.MotionState(1, 2049, 64, DEV)
    with pytest.raises(ValueError):
        motion.MotionState(1, 2048, 2047 + 2, DEV)
    # the C entry itself
    p = lambda t: t.data_ptr()  # noqa: E731
    st = (state.prev_grey, state.prev_coarse, state.prev_valid, state.work_grey, state.work_coarse, state.sums)
    out = (torch.zeros((2, 2), dtype=torch.int32, device=DEV), torch.zeros((2, 4), dtype=torch.int32, device=DEV))

    def call(F=2, oh=96, ow=160, ph=96, pw=160, S=2, radius=48, gate=100, images=p(img), slot=p(tab), work=4,
             grey=p(st[0]), shift=p(out[0])):
        return L.lib().rtdetr_frame_shift(images, F, oh, ow, ph, pw, slot, p(tab), S, radius, gate, 0, 24, grey,
                                          p(st[1]), p(st[2]), p(st[3]), p(st[4]), p(st[5]), work, shift, p(out[1]),
                                          None)

    for kw, word in ((dict(radius=50), "radius"), (dict(radius=0), "radius"), (dict(gate=1000), "gate"),
                     (dict(ph=95), "pad_h"), (dict(pw=159), "pad_w"), (dict(oh=2049, ph=2049), "2048"),
                     (dict(oh=2048, ow=2047 + 2, ph=2048, pw=2049), "2^22"), (dict(F=1025), "F <= 1024"),
                     (dict(S=1025), "S <= 1024"), (dict(S=0), "S >= 1"), (dict(images=None), "NULL"),
                     (dict(slot=None), "NULL"), (dict(grey=None), "NULL"), (dict(shift=None), "NULL"),
                     (dict(work=3), "F + S")):
        assert call(**kw) != 0, kw
        assert word in L.lib().moe_last_error().decode(), (kw, L.lib().moe_last_error())
    assert call(F=0, images=None, slot=None) == 0
    assert not L.launch_counts(reset=True)
