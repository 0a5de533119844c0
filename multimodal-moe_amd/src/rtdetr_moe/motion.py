"""Camera-motion compensation for engine.track (TrackArgs.cmc): the global
image shift between two consecutive frames of a sequence, stated once.

* ``shift_reference``: one pair of frames, plain numpy.  The HIP kernels behind
  rtdetr_frame_shift (_lib.frame_shift) compute the same shift and the same
  three sums bit for bit and are tested against it.
* ``sequence_shifts``: the rule over a batch of frames with the tracker's
  frame_slot / frame_reset tables; it is also the estimator of the CPU device
  and of MOE_PREDICT_TRACK=0.
* ``MotionState``: the device buffers rtdetr_frame_shift keeps between launches
  (every slot's last grey image), with an export to / a load from the
  reference's arrays.

The rule.  It measures on the model's input of the full-frame pass, fp32
[out_h, out_w, 3] in [0, 1], the content area without the padding.  Integer
arithmetic from the first step on:
 1. Grey.  Per channel t = v * 255.0f + 0.5f (one fp32 multiply, one fp32 add,
    no FMA), q = int(min(t, 255.0f)) if t >= 0 else 0 (truncation; a NaN gives
    0): clamp(int(t), 0, 255).  g = (77 R + 150 G + 29 B + 128) >> 8, uint8.
 2. Coarse image.  Hc = out_h // 4, Wc = out_w // 4, c = (sum of the 4x4 block
    + 8) >> 4; a remainder of rows or columns is left out.
 3. Coarse search.  R = radius // 4 coarse pixels (radius: input pixels, a
    multiple of 4 in [4, 64]).  The window is columns [R, Wc - R) and rows
    [max(R, r0), min(Hc - R, r1)), r0 = floor(rows[0] Hc), r1 = ceil(rows[1]
    Hc).  Fewer than 8 columns or 8 rows: status 0, shift (0, 0).  Otherwise,
    for every (dx, dy) in [-R, R]^2, SAD = sum |c_cur[y, x] - c_prev[y - dy,
    x - dx]| over the window: content that moved right by dx gives +dx.  The
    winner is the smallest SAD; ties go to the smaller |dx| + |dy|, then the
    smaller |dy|, then the lower dy, then the lower dx.  Gate (per mille, in
    [0, 999]): if the winner is not (0, 0) and 1000 SAD_win > (1000 - gate)
    SAD(0, 0) in 64-bit integers: status 2, shift (0, 0), no fine search.
 4. Fine search, on g.  Shifts (4 dxc + ox, 4 dyc + oy), ox, oy in [-2, 2];
    margin M = 4 R + 2; the window is columns [M, out_w - M) and rows [max(M,
    4 r0), min(out_h - M, 4 r1)), the same minimum size (else status 0, the
    coarse sums reported); the same order of preference on the total shift.
    Status 1, the shift in input pixels.
The model is ONE translation per frame: it captures the image motion of yaw and
pitch; it does not capture the expansion about the focus of expansion in
straight driving (the shift comes out near 0 there and the tracks' velocity
filter does the work), and it does not capture roll.
"""
from __future__ import annotations

import math

import numpy as np

MOTION_MAX_HW, MOTION_MAX_PIXELS = 2048, 1 << 22  # rtdetr_frame_shift's limits: each side, out_h * out_w
MOTION_MAX_F, MOTION_MAX_S = 1024, 1024
MIN_WINDOW = 8
NO_ESTIMATE, ESTIMATED, GATED = 0, 1, 2  # status


def check_search(radius, gate) -> tuple:
    """-> (radius, gate in per mille) or a ValueError: radius a multiple of 4 in [4, 64], gate in [0, 0.999]."""
    if isinstance(radius, bool) or int(radius) != radius or int(radius) % 4 or not 4 <= int(radius) <= 64:
        raise ValueError(f"radius must be a multiple of 4 in [4, 64], got {radius!r}")
    g = float(gate)
    if g != g or not 0 <= round(1000 * g) <= 999:
        raise ValueError(f"gate must be in [0, 0.999], got {gate!r}")
    return int(radius), int(round(1000 * g))


def check_rows(rows) -> tuple:
    """-> (top, bottom) as floats or a ValueError: 0 <= top < bottom <= 1."""
    try:
        t, b = (float(v) for v in rows)
    except (TypeError, ValueError):
        raise ValueError(f"rows must be (top, bottom), got {rows!r}") from None
    if not 0.0 <= t < b <= 1.0:
        raise ValueError(f"rows must be 0 <= top < bottom <= 1, got {rows!r}")
    return t, b


def coarse_rows(rows, out_h) -> tuple:
    """(r0, r1): the rows of the coarse image that ``rows`` (fractions of the height) allows."""
    t, b = check_rows(rows)
    hc = int(out_h) // 4
    return int(math.floor(t * hc)), int(math.ceil(b * hc))


def grey_u8(img) -> np.ndarray:
    """The rule's step 1: fp32 [..., h, w, 3] -> uint8 [..., h, w]."""
    v = np.asarray(img, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = v * np.float32(255.0) + np.float32(0.5)
        q = np.where(t >= 0, np.minimum(t, np.float32(255.0)), np.float32(0.0)).astype(np.int32)
    return ((77 * q[..., 0] + 150 * q[..., 1] + 29 * q[..., 2] + 128) >> 8).astype(np.uint8)


def coarse_u8(grey) -> np.ndarray:
    """The rule's step 2: uint8 [..., h, w] -> uint8 [..., h // 4, w // 4]."""
    g = np.asarray(grey)
    hc, wc = g.shape[-2] // 4, g.shape[-1] // 4
    s = g[..., :4 * hc, :4 * wc].astype(np.int32).reshape(g.shape[:-2] + (hc, 4, wc, 4)).sum((-3, -1))
    return ((s + 8) >> 4).astype(np.uint8)


def _search(cur, prev, x0, x1, y0, y1, shifts):
    """The SADs of ``shifts`` [(dx, dy)] over the window and the winner's index by the rule's order."""
    win = cur[y0:y1, x0:x1].astype(np.int32)
    p = prev.astype(np.int32)
    sads = [int(np.abs(win - p[y0 - dy:y1 - dy, x0 - dx:x1 - dx]).sum()) for dx, dy in shifts]
    best = min(range(len(shifts)), key=lambda i: (sads[i], abs(shifts[i][0]) + abs(shifts[i][1]), abs(shifts[i][1]),
                                                 shifts[i][1], shifts[i][0]))
    return sads, best


def grey_shift(g_cur, g_prev, radius, gate, r0, r1, c_cur=None, c_prev=None):
    """shift_reference on grey images (uint8 [h, w]); ``gate`` in per mille, r0 / r1 coarse rows."""
    h, w = g_cur.shape
    c_cur = coarse_u8(g_cur) if c_cur is None else c_cur
    c_prev = coarse_u8(g_prev) if c_prev is None else c_prev
    hc, wc = c_cur.shape
    R = radius // 4
    x0, x1, y0, y1 = R, wc - R, max(R, r0), min(hc - R, r1)
    if x1 - x0 < MIN_WINDOW or y1 - y0 < MIN_WINDOW:
        return (0, 0), NO_ESTIMATE, (0, 0, 0)
    shifts = [(dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
    sads, best = _search(c_cur, c_prev, x0, x1, y0, y1, shifts)
    sad0, sadc, (dxc, dyc) = sads[shifts.index((0, 0))], sads[best], shifts[best]
    if (dxc, dyc) != (0, 0) and 1000 * sadc > (1000 - gate) * sad0:
        return (0, 0), GATED, (sad0, sadc, 0)
    M = 4 * R + 2
    x0, x1, y0, y1 = M, w - M, max(M, 4 * r0), min(h - M, 4 * r1)
    if x1 - x0 < MIN_WINDOW or y1 - y0 < MIN_WINDOW:
        return (0, 0), NO_ESTIMATE, (sad0, sadc, 0)
    shifts = [(4 * dxc + ox, 4 * dyc + oy) for oy in range(-2, 3) for ox in range(-2, 3)]
    sads, best = _search(g_cur, g_prev, x0, x1, y0, y1, shifts)
    return shifts[best], ESTIMATED, (sad0, sadc, sads[best])


def shift_reference(cur, prev, radius=48, gate=100, rows=(0.0, 1.0)):
    """The rule on one pair of frames: ``cur`` / ``prev`` fp32 [out_h, out_w, 3]
    (arrays or tensors), ``radius`` in input pixels, ``gate`` in per mille,
    ``rows`` the fractions of the height the windows may use.
    -> ((dx, dy) in input pixels, status 0 no estimate / 1 estimated / 2 gated,
    (SAD(0, 0), the coarse winner's SAD, the fine winner's SAD))."""
    radius, _ = check_search(radius, 0.0)
    gate = int(gate)
    if not 0 <= gate <= 999:
        raise ValueError(f"gate must be in [0, 999] per mille, got {gate}")
    cur, prev = np.asarray(cur, dtype=np.float32), np.asarray(prev, dtype=np.float32)
    if cur.ndim != 3 or cur.shape[-1] != 3 or cur.shape != prev.shape:
        raise ValueError("cur and prev must be [out_h, out_w, 3] of one size")
    r0, r1 = coarse_rows(rows, cur.shape[0])
    return grey_shift(grey_u8(cur), grey_u8(prev), radius, gate, r0, r1)


def new_motion_state(S: int, out_h: int, out_w: int) -> dict:
    """An empty state of S slots: every slot's last grey image and whether it has one."""
    return {"grey": np.zeros((int(S), int(out_h), int(out_w)), np.uint8), "valid": np.zeros(int(S), np.int32)}


def sequence_shifts(images, frame_slot, frame_reset, state, radius=48, gate=100, rows=(0.0, 1.0)):
    """The rule over a batch: ``images`` fp32 [F, out_h, out_w, 3]; frame_slot /
    frame_reset [F] as the tracker's.  Frame f's predecessor is the nearest
    earlier frame of the batch with the same slot, or else the slot's stored
    grey image if it has one; frame_reset[f] means no predecessor (status 0,
    shift (0, 0)).  Afterwards every slot stores the grey image of its last
    frame.  A frame whose slot is outside [0, S) gets (0, 0) and touches
    nothing.  Updates ``state`` (new_motion_state) in place
    -> (shift int32 [F, 2], info int32 [F, 4]: status and the three SADs)."""
    images = np.asarray(images, dtype=np.float32)
    F = images.shape[0]
    S, h, w = state["grey"].shape
    if images.shape[1:] != (h, w, 3):
        raise ValueError(f"images must be [F, {h}, {w}, 3], got {images.shape}")
    radius, _ = check_search(radius, 0.0)
    r0, r1 = coarse_rows(rows, h)
    shift, info = np.zeros((F, 2), np.int32), np.zeros((F, 4), np.int32)
    last = {}  # slot -> (grey, coarse) of its latest frame of this batch
    for f in range(F):
        s = int(frame_slot[f])
        if not 0 <= s < S:
            continue
        g = grey_u8(images[f])
        c = coarse_u8(g)
        pred = None
        if not int(frame_reset[f]):
            if s in last:
                pred = last[s]
            elif state["valid"][s]:
                pred = (state["grey"][s], None)
        if pred is not None:
            (dx, dy), status, sads = grey_shift(g, pred[0], radius, int(gate), r0, r1, c, pred[1])
            shift[f] = dx, dy
            info[f] = (status,) + tuple(sads)
        last[s] = (g, c)
    for s, (g, _) in last.items():
        state["grey"][s], state["valid"][s] = g, 1
    return shift, info


class MotionState:
    """S slots' last grey images on the device, between launches of
    rtdetr_frame_shift (the layout include/moe_hip.h documents), and the
    launches' workspace, allocated once for up to ``frames`` frames a launch
    (default S; a larger launch grows it):
      prev_grey   uint8 [S, out_h, out_w]   the slot's last frame, grey
      prev_coarse uint8 [S, Hc, Wc]         its coarse image
      prev_valid  int32 [S]                 1: the slot has one
      work_grey   uint8 [frames + S, out_h, out_w], work_coarse likewise: the
                  launch's frames, then a copy of each slot's image as the
                  launch found it
      sums        int32 [frames, 33 * 33 + 25 + 7]: the SADs, plan and ticket
    About 3 bytes a pixel and slot at frames = S."""

    SUMS = 33 * 33 + 25 + 7

    def __init__(self, S: int, out_h: int, out_w: int, device, frames: int | None = None):
        import torch

        self.S, self.out_h, self.out_w = int(S), int(out_h), int(out_w)
        if not 1 <= self.S <= MOTION_MAX_S:
            raise ValueError(f"MotionState: need 1 <= S <= {MOTION_MAX_S}")
        if not (1 <= self.out_h <= MOTION_MAX_HW and 1 <= self.out_w <= MOTION_MAX_HW
                and self.out_h * self.out_w <= MOTION_MAX_PIXELS):
            raise ValueError(f"MotionState: out_h and out_w must be in [1, {MOTION_MAX_HW}] with at most "
                             f"{MOTION_MAX_PIXELS} pixels, got {out_h} x {out_w}")
        self.hc, self.wc = self.out_h // 4, self.out_w // 4
        self.device = torch.device(device)
        self.prev_grey = torch.zeros((self.S, self.out_h, self.out_w), dtype=torch.uint8, device=self.device)
        self.prev_coarse = torch.zeros((self.S, self.hc, self.wc), dtype=torch.uint8, device=self.device)
        self.prev_valid = torch.zeros(self.S, dtype=torch.int32, device=self.device)
        self.frames = 0
        self.reserve(self.S if frames is None else int(frames))

    def reserve(self, frames: int):
        """The workspace for launches of up to ``frames`` frames."""
        import torch

        if frames <= self.frames:
            return
        if frames > MOTION_MAX_F:
            raise ValueError(f"MotionState: at most {MOTION_MAX_F} frames a launch, got {frames}")
        self.frames = frames
        n = frames + self.S
        self.work_grey = torch.empty((n, self.out_h, self.out_w), dtype=torch.uint8, device=self.device)
        self.work_coarse = torch.empty((n, self.hc, self.wc), dtype=torch.uint8, device=self.device)
        self.sums = torch.zeros((frames, self.SUMS), dtype=torch.int32, device=self.device)

    def export(self) -> dict:
        """The reference's arrays (new_motion_state's layout)."""
        return {"grey": self.prev_grey.cpu().numpy().copy(), "valid": self.prev_valid.cpu().numpy().copy()}

    def load(self, state: dict):
        """From the reference's arrays; the coarse images are made here."""
        import torch

        grey = np.ascontiguousarray(state["grey"], dtype=np.uint8)
        if grey.shape != tuple(self.prev_grey.shape):
            raise ValueError(f"MotionState.load: grey must be {tuple(self.prev_grey.shape)}, got {grey.shape}")
        self.prev_grey.copy_(torch.from_numpy(grey))
        self.prev_coarse.copy_(torch.from_numpy(coarse_u8(grey)))
        self.prev_valid.copy_(torch.from_numpy((np.asarray(state["valid"]) != 0).astype(np.int32)))
