"""rtdetr_resize_pad_u8_flip (_lib.resize_pad(..., flip=...)): a slot with a
non-zero flag is, bit for bit, what rtdetr_resize_pad_u8 writes for a
host-mirrored copy of the same pixels, and a slot with 0 is
rtdetr_resize_pad_u8 on the same descriptor.

The shapes are those of tests/test_gpu_resize.py, restated: both forms of the
kernel (the tiled LDS form up to a reduction of 8 per axis, the direct form
past it), sources smaller than one tap window, an odd width at identity scale,
non-integer taps and large coordinates.  Against preprocess.resize_reference of
the mirrored frame the tolerance is that file's 5e-6 on the [0, 1] scale, for
its reason: a convex combination of at most 26 taps per pass with fp32
accumulation, (26 + 3) 6e-8 for two passes is 3.5e-6.  Largest error measured
on the MI355X: 1.7e-7 (the direct form at 12.5x; the unmirrored kernel measures 1.6e-7).  Every input is valid."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 5e-6

# source (h, w), content (h, w), padded (h, w)
CASES = [
    ((37, 53), (37, 53), (64, 64)),         # identity; odd width, odd row bytes (159)
    ((271, 483), (88, 156), (96, 160)),     # ZOD's 3.08x; non-integer taps
    ((64, 96), (32, 48), (32, 64)),         # exact 2x; right padding only
    ((50, 70), (120, 200), (128, 224)),     # upscaling; support 1
    ((30, 200), (64, 96), (64, 96)),        # up in y, down in x; no padding
    ((1, 1), (32, 32), (32, 32)),           # sources smaller than one tap window
    ((5, 7), (32, 32), (32, 32)),
    ((256, 512), (32, 64), (32, 64)),       # the 8x limit of the tiled form
    ((8, 4000), (8, 1300), (32, 1312)),     # large coordinates
    ((300, 200), (24, 16), (32, 32)),       # 12.5x: the direct form
    ((40, 330), (40, 33), (64, 64)),        # 10x in x only: the direct form, identity in y
]


def _content(h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


def _mirrored(frame):
    return torch.from_numpy(frame.numpy()[:, ::-1].copy())


def _pack(frames):
    from src.rtdetr_moe.preprocess import pack_frames

    return pack_frames([f.numpy() for f in frames])


def _flags(*v):
    return torch.tensor(v, dtype=torch.int32)


@pytest.fixture(scope="module")
def L(hip_lib):
    from src.moe import _lib

    return _lib


def test_symbol_is_exported_and_bound(L):
    assert hasattr(L.lib(), "rtdetr_resize_pad_u8_flip")
    assert len(L.SIGNATURES["rtdetr_resize_pad_u8_flip"][1]) == len(L.SIGNATURES["rtdetr_resize_pad_u8"][1]) + 1


@pytest.mark.parametrize("src,out,pad", CASES)
def test_mirrored_slot_equals_the_existing_kernel_on_host_mirrored_pixels(L, src, out, pad):
    from src.rtdetr_moe.preprocess import resize_reference

    x = _content(*src, seed=src[0] * 10007 + src[1])
    buf, desc = _pack([x])
    mbuf, mdesc = _pack([_mirrored(x)])
    assert torch.equal(desc, mdesc)
    L.launch_counts(reset=True)
    got = L.resize_pad(buf.cuda(), desc, out, pad, flip=_flags(1))
    assert L.launch_counts() == {"resize": 1}
    assert tuple(got.shape) == (1, 3, *pad) and got.dtype == torch.float32
    assert got.is_contiguous(memory_format=torch.channels_last)
    want = L.resize_pad(mbuf.cuda(), mdesc, out, pad)
    assert torch.equal(got, want)
    # a slot with 0 is the existing kernel on the same descriptor
    plain = L.resize_pad(buf.cuda(), desc, out, pad)
    assert torch.equal(L.resize_pad(buf.cuda(), desc, out, pad, flip=_flags(0)), plain)
    # the stated rule: the project's resize of the mirrored bytes
    got = got.cpu()
    ref = resize_reference(_mirrored(x), out[0], out[1], pad[0], pad[1])
    err = float((got[0].double() - ref).abs().max())
    print(f"{src} -> {out} ({pad}) mirrored: max |got - reference| = {err:.3e}")
    assert err <= TOL
    assert (got[0, :, out[0]:, :] == 0).all() and (got[0, :, :, out[1]:] == 0).all()
    if src == out:
        assert torch.equal(got[0, :, :out[0], :out[1]], _mirrored(x).permute(2, 0, 1).float() / 255.0)


def test_batch_of_mixed_flags_different_sizes_and_an_empty_slot(L):
    out, pad = (88, 156), (96, 160)
    frames = [_content(271, 483, 1), _content(37, 53, 2), _content(64, 96, 3), _content(900, 200, 4)]
    flags = [1, 0, 1, 1, 1]  # the last slot is empty; the fourth frame takes the direct form (10.2x in y)
    buf, desc = _pack(frames)
    desc = torch.cat([desc, torch.zeros((1, 4), dtype=torch.int64)])
    L.launch_counts(reset=True)
    got = L.resize_pad(buf.cuda(), desc, out, pad, flip=_flags(*flags))
    assert L.launch_counts() == {"resize": 1}
    plain = L.resize_pad(buf.cuda(), desc, out, pad)
    mbuf, mdesc = _pack([_mirrored(f) for f in frames])
    mirrored = L.resize_pad(mbuf.cuda(), torch.cat([mdesc, torch.zeros((1, 4), dtype=torch.int64)]), out, pad)
    for i, f in enumerate(flags):
        assert torch.equal(got[i], (mirrored if f else plain)[i]), i
    assert (got[4] == 0).all()
    assert not torch.equal(got[0], plain[0])
    # any non-zero value is a flag
    assert torch.equal(L.resize_pad(buf.cuda(), desc, out, pad, flip=_flags(-1, 0, 7, 1 << 30, 0))[:4], got[:4])


def test_crop_with_row_stride_and_unaligned_offset_mirrors_inside_its_window(L):
    out, pad = (32, 48), (32, 64)
    fh, fw, x0, y0, tw, th = 40, 50, 5, 3, 21, 17
    frame = _content(fh, fw, 5)
    crop = frame[y0:y0 + th, x0:x0 + tw]
    stride = 3 * fw
    row = torch.tensor([[y0 * stride + 3 * x0, th, tw, stride]], dtype=torch.int64)
    buf = frame.reshape(-1).clone()
    got = L.resize_pad(buf.cuda(), row, out, pad, flip=_flags(1))
    cbuf, cdesc = _pack([_mirrored(crop)])  # a host copy of the mirrored crop
    want = L.resize_pad(cbuf.cuda(), cdesc, out, pad)
    assert torch.equal(got, want)
    # everything outside the crop poisoned: the result does not move
    poisoned = torch.full_like(frame, 255)
    poisoned[y0:y0 + th, x0:x0 + tw] = crop
    assert torch.equal(L.resize_pad(poisoned.reshape(-1).cuda(), row, out, pad, flip=_flags(1)), want)
    poisoned[poisoned == 255] = 0
    poisoned[y0:y0 + th, x0:x0 + tw] = crop
    assert torch.equal(L.resize_pad(poisoned.reshape(-1).cuda(), row, out, pad, flip=_flags(1)), want)
    # an odd offset in front of the buffer
    shifted = torch.cat([torch.full((7,), 255, dtype=torch.uint8), buf])
    row7 = row.clone()
    row7[0, 0] += 7
    assert torch.equal(L.resize_pad(shifted.cuda(), row7, out, pad, flip=_flags(1)), want)


def test_every_element_written_once_and_nothing_outside(L):
    out, pad = (88, 156), (96, 160)
    frames = [_content(271, 483, 1), _content(50, 70, 2), _content(900, 200, 3)]
    buf, desc = _pack(frames)
    n = 3 * 3 * pad[0] * pad[1]
    guard = 4096
    big = torch.full((n + 2 * guard,), float("nan"), device="cuda")
    dst = big[guard:guard + n].view(3, pad[0], pad[1], 3).permute(0, 3, 1, 2)  # channels-last [3, 3, H, W]
    flags = _flags(1, 1, 1)
    got = L.resize_pad(buf.cuda(), desc, out, pad, out=dst, flip=flags)
    assert got.data_ptr() == dst.data_ptr()
    torch.cuda.synchronize()
    assert torch.isnan(big[:guard]).all() and torch.isnan(big[guard + n:]).all()
    assert not torch.isnan(dst).any()
    assert (dst[:, :, out[0]:, :] == 0).all() and (dst[:, :, :, out[1]:] == 0).all()
    first = dst.clone()
    L.resize_pad(buf.cuda(), desc, out, pad, out=dst, flip=flags)  # again into the same buffer: no accumulation
    assert torch.equal(dst, first)
    desc2 = desc.clone()
    desc2[1] = 0  # a slot goes empty in a reused buffer: rewritten with zeros, flag or not
    L.resize_pad(buf.cuda(), desc2, out, pad, out=dst, flip=flags)
    assert torch.equal(dst[0], first[0]) and (dst[1] == 0).all() and torch.equal(dst[2], first[2])


def test_launch_under_graph_capture(L):
    out, pad = (32, 48), (32, 64)
    a, b = _content(64, 96, 1), _content(50, 70, 2)
    nbytes = max(a.numel(), b.numel())
    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    desc = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    flip = torch.zeros(1, dtype=torch.int32, device="cuda")
    dst = torch.empty((1, 3, *pad), device="cuda").contiguous(memory_format=torch.channels_last)

    def load(frame, flag):
        buf, d = _pack([frame])
        L.check_resize_desc(d, nbytes)
        src[:buf.numel()].copy_(buf)
        desc.copy_(d)
        flip.fill_(flag)

    def want(frame, flag):
        buf, d = _pack([_mirrored(frame) if flag else frame])
        return L.resize_pad(buf.cuda(), d, out, pad)

    load(a, 1)
    L.resize_pad(src, None, out, pad, out=dst, desc_dev=desc, flip=flip)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.resize_pad(src, None, out, pad, out=dst, desc_dev=desc, flip=flip)
    for frame, flag in ((b, 1), (a, 0), (a, 1)):  # the replay reads the flags where they stand
        load(frame, flag)
        dst.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(dst, want(frame, flag))


def test_invalid_arguments_raise_without_a_launch(L):
    x = _content(16, 16, 0)
    buf, desc = _pack([x])
    dbuf = buf.cuda()
    L.launch_counts(reset=True)
    with pytest.raises(L.MoEKernelError, match="pad >= out"):
        L.resize_pad(dbuf, desc, (32, 32), (32, 16), flip=_flags(1))
    with pytest.raises(L.MoEKernelError, match="GPU tensor"):
        L.resize_pad(buf, desc, (32, 32), (32, 32), flip=_flags(1))
    with pytest.raises(L.MoEKernelError, match="outside"):  # the same host-side bound check of the descriptors
        L.resize_pad(dbuf, torch.tensor([[1, 16, 16, 48]], dtype=torch.int64), (32, 32), (32, 32), flip=_flags(1))
    with pytest.raises(L.MoEKernelError, match="flip must be"):
        L.resize_pad(dbuf, desc, (32, 32), (32, 32), flip=_flags(1, 0))
    with pytest.raises(L.MoEKernelError, match="flip must be"):
        L.resize_pad(dbuf, desc, (32, 32), (32, 32), flip=torch.ones(1, dtype=torch.int64))
    # the C entry's own checks
    f = L.lib().rtdetr_resize_pad_u8_flip
    ddesc, dflip = desc.cuda(), _flags(1).cuda()
    dst = torch.empty(3 * 32 * 32, device="cuda")
    args = (dbuf.data_ptr(), ddesc.data_ptr())
    assert f(*args, None, 1, 32, 32, 32, 32, dst.data_ptr(), None) != 0 and b"NULL flip" in L.lib().moe_last_error()
    assert f(*args, None, 0, 32, 32, 32, 32, dst.data_ptr(), None) != 0  # refused whatever B is
    fl = dflip.data_ptr()
    assert f(*args, fl, 1, 32, 32, 16, 32, dst.data_ptr(), None) != 0 and b"pad_h >= out_h" in L.lib().moe_last_error()
    assert f(*args, fl, 1, 0, 32, 32, 32, dst.data_ptr(), None) != 0
    assert f(*args, fl, -1, 32, 32, 32, 32, dst.data_ptr(), None) != 0
    assert f(None, ddesc.data_ptr(), fl, 1, 32, 32, 32, 32, dst.data_ptr(), None) != 0
    assert f(*args, fl, 1, 32, 32, 32, 32, None, None) != 0
    assert f(None, None, fl, 0, 32, 32, 32, 32, None, None) == 0  # B == 0: success without a launch
    assert ctypes.sizeof(ctypes.c_longlong) == 8
    assert L.launch_counts() == {}
