"""rtdetr_resize_pad_u8 (_lib.resize_pad) against preprocess.resize_reference.

Tolerance 5e-6 on the [0, 1] scale: each pass is a convex combination of at
most 18 taps of values <= 255 with fp32 accumulation, about (18 + 3) 6e-8 255
per pass, 7e-4 grey levels for the two passes, 2.6e-6 after / 255.  A kernel
that does its coordinate arithmetic in fp32 is off by 4.3e-5 on the 8 x 4000
case.  The identity case is compared for equality with x.float() / 255.
Two more pairs take the kernel's other path, the direct form of a reduction
above 8 per axis (26 and 21 taps: (26 + 3) 6e-8 for two passes is 3.5e-6, under
the same bound).  Largest errors observed on the MI355X: 1.6e-7 (DESIGN.md
section 20 has the table).  Every input is valid."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 5e-6

# source (h, w), content (h, w), padded (h, w)
CASES = [
    ((37, 53), (37, 53), (64, 64)),         # identity; odd row bytes (159)
    ((271, 483), (88, 156), (96, 160)),     # ZOD's 3.08x; non-integer taps
    ((64, 96), (32, 48), (32, 64)),         # exact 2x; right padding only
    ((50, 70), (120, 200), (128, 224)),     # upscaling; support 1
    ((30, 200), (64, 96), (64, 96)),        # up in y, down in x; no padding
    ((1, 1), (32, 32), (32, 32)),           # sources smaller than one tap window
    ((5, 7), (32, 32), (32, 32)),
    ((256, 512), (32, 64), (32, 64)),       # the 8x limit of the tiled form
    ((8, 4000), (8, 1300), (32, 1312)),     # large coordinates: fp32 index math fails here
    ((300, 200), (24, 16), (32, 32)),       # 12.5x: past the tiled form's limit, the direct form
    ((40, 330), (40, 33), (64, 64)),        # 10x in x only: the direct form, identity in y
]


def _content(h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


def _pack(frames):
    from src.rtdetr_moe.preprocess import pack_frames

    return pack_frames([f.numpy() for f in frames])


def _reference(frame, out, pad):
    from src.rtdetr_moe.preprocess import resize_reference

    return resize_reference(frame, out[0], out[1], pad[0], pad[1])


@pytest.fixture(scope="module")
def L(hip_lib):
    from src.moe import _lib

    return _lib


@pytest.mark.parametrize("src,out,pad", CASES)
def test_resize_against_the_reference(L, src, out, pad):
    x = _content(*src, seed=src[0] * 10007 + src[1])
    buf, desc = _pack([x])
    L.launch_counts(reset=True)
    got = L.resize_pad(buf.cuda(), desc, out, pad)
    assert L.launch_counts() == {"resize": 1}
    assert tuple(got.shape) == (1, 3, *pad) and got.dtype == torch.float32
    assert got.is_contiguous(memory_format=torch.channels_last)
    got = got.cpu()
    ref = _reference(x, out, pad)
    err = float((got[0].double() - ref).abs().max())
    print(f"{src} -> {out} ({pad}): max |got - reference| = {err:.3e}")
    assert err <= TOL
    assert (got[0, :, out[0]:, :] == 0).all() and (got[0, :, :, out[1]:] == 0).all()
    if src == out:
        assert torch.equal(got[0, :, :out[0], :out[1]], x.permute(2, 0, 1).float() / 255.0)


def test_batch_of_different_sizes_and_an_empty_slot(L):
    out, pad = (88, 156), (96, 160)
    frames = [_content(271, 483, 1), _content(37, 53, 2), _content(64, 96, 3)]
    buf, desc = _pack(frames)
    desc = torch.cat([desc, torch.zeros((1, 4), dtype=torch.int64)])  # a fourth, empty slot
    L.launch_counts(reset=True)
    got = L.resize_pad(buf.cuda(), desc, out, pad)
    assert L.launch_counts() == {"resize": 1}
    got = got.cpu()
    assert tuple(got.shape) == (4, 3, *pad)
    for i, f in enumerate(frames):
        assert float((got[i].double() - _reference(f, out, pad)).abs().max()) <= TOL
    assert (got[3] == 0).all()
    # each image of the batch is the image of its own launch
    for i, f in enumerate(frames):
        b1, d1 = _pack([f])
        assert torch.equal(L.resize_pad(b1.cuda(), d1, out, pad).cpu()[0], got[i])


def test_row_stride_and_unaligned_offset(L):
    out, pad = (88, 156), (96, 160)
    x = _content(271, 483, 7)
    h, w = x.shape[:2]
    buf, desc = _pack([x])
    want = L.resize_pad(buf.cuda(), desc, out, pad).cpu()
    stride = 3 * w + 7
    loose = torch.full((5 + h * stride,), 255, dtype=torch.uint8)
    rows = loose[5:].view(h, stride)
    rows[:, :3 * w] = x.reshape(h, 3 * w)
    got = L.resize_pad(loose.cuda(), torch.tensor([[5, h, w, stride]], dtype=torch.int64), out, pad).cpu()
    assert torch.equal(got, want)


def test_every_element_written_once_and_nothing_outside(L):
    out, pad = (88, 156), (96, 160)
    frames = [_content(271, 483, 1), _content(50, 70, 2)]
    buf, desc = _pack(frames)
    n = 2 * 3 * pad[0] * pad[1]
    guard = 4096
    big = torch.full((n + 2 * guard,), float("nan"), device="cuda")
    dst = big[guard:guard + n].view(2, pad[0], pad[1], 3).permute(0, 3, 1, 2)  # channels-last [2, 3, H, W]
    got = L.resize_pad(buf.cuda(), desc, out, pad, out=dst)
    assert got.data_ptr() == dst.data_ptr()
    torch.cuda.synchronize()
    assert torch.isnan(big[:guard]).all() and torch.isnan(big[guard + n:]).all()
    assert not torch.isnan(dst).any()
    assert (dst[:, :, out[0]:, :] == 0).all() and (dst[:, :, :, out[1]:] == 0).all()
    first = dst.clone()
    L.resize_pad(buf.cuda(), desc, out, pad, out=dst)  # again into the same buffer: no accumulation
    assert torch.equal(dst, first)
    for i, f in enumerate(frames):
        assert float((first[i].cpu().double() - _reference(f, out, pad)).abs().max()) <= TOL
    # a slot goes empty in a reused buffer: its image is rewritten with zeros
    desc2 = desc.clone()
    desc2[1] = 0
    L.resize_pad(buf.cuda(), desc2, out, pad, out=dst)
    assert torch.equal(dst[0], first[0]) and (dst[1] == 0).all()


def test_launch_under_graph_capture(L):
    out, pad = (32, 48), (32, 64)
    a, b = _content(64, 96, 1), _content(50, 70, 2)
    nbytes = max(a.numel(), b.numel())
    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    desc = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    dst = torch.empty((1, 3, *pad), device="cuda").contiguous(memory_format=torch.channels_last)

    def load(frame):
        buf, d = _pack([frame])
        L.check_resize_desc(d, nbytes)
        src[:buf.numel()].copy_(buf)
        desc.copy_(d)

    load(a)
    L.resize_pad(src, None, out, pad, out=dst, desc_dev=desc)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.resize_pad(src, None, out, pad, out=dst, desc_dev=desc)
    for frame in (b, a):
        load(frame)
        dst.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert float((dst[0].cpu().double() - _reference(frame, out, pad)).abs().max()) <= TOL


def test_invalid_arguments_raise_without_a_launch(L):
    x = _content(16, 16, 0)
    buf, desc = _pack([x])
    dbuf = buf.cuda()
    L.launch_counts(reset=True)
    with pytest.raises(L.MoEKernelError, match="pad >= out"):
        L.resize_pad(dbuf, desc, (32, 32), (32, 16))
    with pytest.raises(L.MoEKernelError, match="GPU tensor"):
        L.resize_pad(buf, desc, (32, 32), (32, 32))
    with pytest.raises(L.MoEKernelError, match="outside"):
        L.resize_pad(dbuf, torch.tensor([[1, 16, 16, 48]], dtype=torch.int64), (32, 32), (32, 32))
    with pytest.raises(L.MoEKernelError, match="channels-last"):
        L.resize_pad(dbuf, desc, (32, 32), (32, 32), out=torch.empty((1, 3, 32, 32), device="cuda"))
    # the C entry's own checks
    import ctypes

    f = L.lib().rtdetr_resize_pad_u8
    ddesc = desc.cuda()
    dst = torch.empty(3 * 32 * 32, device="cuda")
    args = (dbuf.data_ptr(), ddesc.data_ptr())
    assert f(*args, 1, 32, 32, 16, 32, dst.data_ptr(), None) != 0 and b"pad_h >= out_h" in L.lib().moe_last_error()
    assert f(*args, 1, 0, 32, 32, 32, dst.data_ptr(), None) != 0
    assert f(*args, -1, 32, 32, 32, 32, dst.data_ptr(), None) != 0
    assert f(None, ddesc.data_ptr(), 1, 32, 32, 32, 32, dst.data_ptr(), None) != 0
    assert f(None, None, 0, 32, 32, 32, 32, None, None) == 0  # B == 0: success without a launch
    assert ctypes.sizeof(ctypes.c_longlong) == 8
    assert L.launch_counts() == {}
