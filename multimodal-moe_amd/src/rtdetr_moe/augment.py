"""Training-time batch augmentation: scale / translate jitter, horizontal flip
and HSV jitter of a whole batch, images and boxes, on the device.

The reference trains through Ultralytics' ``RTDETR.train``, which applies
these by default (``scale=0.5, translate=0.1, fliplr=0.5, hsv_h/s/v=0.015/0.7/
0.4``).  Here they are opt-in through the ``-aug`` model-spec token
(moe/config.py) or ``TrainStep(augment=True)``.

Parameters.  Per image, drawn on the HOST from one seeded ``torch.Generator``
per ``BatchAugment`` (seed * 1000 + rank: ranks differ, a run is
reproducible), packed into an fp32 table ``[B, 16]`` (``make_table``):

    [0..5]  forward 2x3 matrix   x' = m0 x + m1 y + m2,  y' = m3 x + m4 y + m5
    [6..11] its inverse
    [12] dh   [13] gs   [14] gv   [15] s

Geometry (Ultralytics ``random_perspective`` with degrees, shear and
perspective 0) over the content rectangle w x h, the top-left part of the
padded tensor: s ~ U(1 - scale, 1 + scale), tx ~ U(0.5 - translate, 0.5 +
translate) w, ty likewise with h, M = T(tx, ty) S(s) T(-w/2, -h/2); with
probability fliplr followed by x -> w - x.  Both matrices are computed in
float64.

Colour: dh ~ U(-hsv_h, hsv_h), gs ~ 1 + U(-hsv_s, hsv_s), gv ~ 1 + U(-hsv_v,
hsv_v); per pixel RGB -> HSV, h' = frac(h + dh), s' = min(1, s gs), v' =
min(1, v gv), HSV -> RGB.  The hue shift is ADDITIVE on the circle;
Ultralytics' uint8 look-up table multiplies the hue, which jumps at the red
wrap.  dh = 0 and gs = gv = 1 skips the colour step (the identity
then reproduces the source exactly).

Sampling: output pixel centre (x + .5, y + .5) goes through the inverse matrix;
bilinear over the four neighbouring source pixel centres, each tap outside the
content rectangle contributing ``fill`` (114/255): continuous in the
coordinates.  Colour is applied after sampling, not to pixels with no tap
inside the content (they are exactly ``fill``), and padding rows / columns are
0 as the loader leaves them.

Boxes: the padded targets of ``criterion.pad_targets`` (cxcywh normalised to
the padded tensor).  Each valid box: to content pixels (xyxy), both corners
through the forward matrix, min / max, clip to [0, w] x [0, h]; kept iff new
width >= 2 px, new height >= 2 px, aspect ratio < 100 and area_new /
(area_old s^2) > 0.1 (Ultralytics' ``box_candidates`` constants, written
without divisions: max(nw, nh) < 100 min(nw, nh), nw nh > 0.1 area_old s^2).
Survivors are compacted to the front in their order, ``PAD_BOX`` / label 0
behind them; the new ``n_valid`` and its batch sum (a device scalar) come
with them, so the host never learns the counts.

``augment_reference`` is the plain-torch form (any float dtype, any device):
the CPU training path and the tests' reference.  ``BatchAugment`` runs the two
HIP kernels (csrc/augment.hip) on the GPU and ``augment_reference`` on the CPU.

Mosaic (the ``-mosaic[<p>]`` spec token, ``TrainStep(mosaic=p)``,
``BatchAugment(mosaic=p)``; Ultralytics' ``_mosaic4`` with border -s/2 in
front of ``random_perspective``).  Four images per training frame, the same
pipeline with a four-image canvas in the middle.

Canvas: 2h x 2w pixels, background ``fill``.  Per output image n the host
draws an integer centre xc = floor(w/2 + u w), yc = floor(h/2 + u' h) (xc in
[w/2, 3w/2)) and four source indices into the SAME batch: top-left = n itself,
top-right, bottom-left, bottom-right uniform over [0, b), repeats allowed.
Deviation from the reference: partners come from the step's own batch on the
rank, not from the whole dataset.  Canvas pixel (X, Y), 0 <= X < 2w, 0 <= Y <
2h: the quadrant is right iff X >= xc, bottom iff Y >= yc; its origin is ox =
xc if right else xc - w, oy = yc if bottom else yc - h; the pixel reads source
pixel (X - ox, Y - oy) of that quadrant's image.  The read is valid iff the
quadrant is not empty (index >= 0) and 0 <= X - ox < w, 0 <= Y - oy < h; every
other tap, any outside the canvas included, contributes ``fill``.  This is
``_mosaic4``'s slicing: the top-left image's bottom-right corner sits at the
centre, the top-right image's bottom-left corner, and so on, cropped by the
canvas.

Geometry: M = T(tx, ty) S(s) T(-w, -h) -- the canvas centre goes to the
origin -- then the optional x -> w - x; s, tx, ty, the flip and the colour
terms are drawn exactly as above (``make_table(..., centre=(w, h))``; the
default centre (w/2, h/2) gives the plain rows bit for bit).  An output pixel
centre goes through the inverse matrix to canvas coordinates and is sampled
bilinearly over the four neighbouring canvas pixel centres by the tap rule
above (each tap resolves its own quadrant).  Colour after sampling; a pixel
with no valid tap is exactly ``fill`` and gets no colour; padding is 0.

Rows without mosaic (probability 1 - p, or p set to 0 for the last epochs) are
the degenerate case of the same table: top-left = n, xc = w, yc = h, the other
three quadrants empty (-1), the matrix about (w/2, h/2): canvas coordinates
inside the top-left quadrant are then source coordinates, and the row gives the
plain result (for boxes inside the content rectangle, which is what a loader
produces: the canvas clip below does not touch them).

Table: fp32 [B, 24] (``MOSAIC_COLS``).  Columns 0..15 as above, the matrices
mapping canvas <-> output; [16] xc, [17] yc; [18..21] the top-left, top-right,
bottom-left, bottom-right source indices as integer-valued floats, -1 for
empty; [22..23] 0.

Random stream: the mosaic uniforms (apply, xc, yc, three partners) come from a
second ``torch.rand`` call on the same generator, made only when the mosaic
probability is positive; the seven draws above keep their positions.

Boxes, for output image n: the quadrants in the order TL, TR, BL, BR, within a
quadrant the source image's slots j < n_valid[src] in order.  Each box: to
content pixels (xyxy) as above, shifted by (ox, oy), clipped to the canvas
[0, 2w] x [0, 2h]; area_ref = the clipped area times s^2; both corners through
the forward matrix, min / max, clip to [0, w] x [0, h]; the same keep test.
Survivors are compacted in that order into an output of capacity ``M_out`` (the
input capacity is ``M_in``), ``PAD_BOX`` / label 0 behind them.  Past ``M_out``
survivors are dropped and n_valid is ``M_out``; the host prevents that: it knows
the raw counts and drew the partners, so need = max_n sum_q count[src[n][q]]
(``BatchAugment.need``) bounds the survivors without a device read.

``mosaic_reference`` is the plain-torch form, ``mosaic_images_hip`` /
``mosaic_boxes_hip`` wrap the HIP kernels.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .criterion import PAD_BOX

TABLE_COLS = 16
MOSAIC_COLS = 24


@dataclass
class AugmentParams:
    """Magnitudes (Ultralytics' defaults) and the fill value of out-of-frame taps."""
    scale: float = 0.5
    translate: float = 0.1
    fliplr: float = 0.5
    hsv_h: float = 0.015
    hsv_s: float = 0.7
    hsv_v: float = 0.4
    fill: float = 114.0 / 255.0


def _f64(v):
    return torch.as_tensor(v, dtype=torch.float64).reshape(-1)


def make_table(s, tx, ty, flip, dh, gs, gv, content_hw, centre=None) -> torch.Tensor:
    """fp32 [B, 16] from per-image parameters (sequences or tensors of length
    B): scale s, translation (tx, ty) in content pixels (the point ``centre``
    of the input frame goes there), flip flags, and the colour terms.
    ``centre``: (x, y), numbers or per-image sequences; default the image
    centre (w/2, h/2), a mosaic row takes the canvas centre (w, h).  Matrices
    in float64."""
    h, w = content_hw
    s, tx, ty, dh, gs, gv = map(_f64, (s, tx, ty, dh, gs, gv))
    cx, cy = (w / 2.0, h / 2.0) if centre is None else (_f64(centre[0]), _f64(centre[1]))
    flip = torch.as_tensor(flip).reshape(-1).to(torch.bool)
    zero = torch.zeros_like(s)
    a, c = s, tx - s * cx                     # x' = s x + (tx - s cx)
    e, f = s, ty - s * cy
    a, c = torch.where(flip, -a, a), torch.where(flip, w - c, c)   # then x' -> w - x'
    # inverse: x = (x' - c) / a, y = (y' - f) / e
    ia, ic = 1.0 / a, -c / a
    ie, i_f = 1.0 / e, -f / e
    cols = [a, zero, c, zero, e, f, ia, zero, ic, zero, ie, i_f, dh, gs, gv, s]
    return torch.stack(cols, dim=1).to(torch.float32)


def make_mosaic_table(s, tx, ty, flip, dh, gs, gv, content_hw, apply=None, xc=None, yc=None,
                      partners=None) -> torch.Tensor:
    """fp32 [B, 24]: ``make_table``'s columns and the mosaic ones.  Rows with
    ``apply`` (bool, length B; default none) are mosaic rows: centre (xc, yc),
    sources (n, partners[n, 0..2]) for the top-left, top-right, bottom-left and
    bottom-right quadrant, the matrix about the canvas centre (w, h).  Every
    other row is degenerate: centre (w, h), top-left n alone, the matrix about
    (w/2, h/2), which is the plain row."""
    h, w = content_hw
    B = _f64(s).numel()
    on = torch.zeros(B, dtype=torch.bool) if apply is None else torch.as_tensor(apply).reshape(-1).to(torch.bool)
    full = lambda v: torch.full((B,), float(v), dtype=torch.float64)  # noqa: E731
    base = make_table(s, tx, ty, flip, dh, gs, gv, content_hw,
                      centre=(torch.where(on, full(w), full(w / 2.0)), torch.where(on, full(h), full(h / 2.0))))
    xc = torch.where(on, full(w) if xc is None else _f64(xc), full(w))
    yc = torch.where(on, full(h) if yc is None else _f64(yc), full(h))
    if partners is None:
        partners = torch.full((B, 3), -1.0, dtype=torch.float64)
    partners = torch.as_tensor(partners, dtype=torch.float64).reshape(B, 3)
    partners = torch.where(on.reshape(B, 1), partners, torch.full_like(partners, -1.0))
    own = torch.arange(B, dtype=torch.float64)
    extra = torch.stack([xc, yc, own, partners[:, 0], partners[:, 1], partners[:, 2], full(0), full(0)], dim=1)
    return torch.cat([base, extra.to(torch.float32)], dim=1)


def identity_table(B, content_hw) -> torch.Tensor:
    h, w = content_hw
    one, zero = [1.0] * B, [0.0] * B
    return make_table(one, [w / 2.0] * B, [h / 2.0] * B, [False] * B, zero, one, one, content_hw)


def _draw_terms(gen, B, content_hw, padded_hw, p):
    """(s, tx, ty, flip, dh, gs, gv) of B images: seven uniform draws per image, one call."""
    h, w = content_hw
    if h > padded_hw[0] or w > padded_hw[1]:
        raise ValueError(f"content {tuple(content_hw)} exceeds the padded tensor {tuple(padded_hw)}")
    u = torch.rand((B, 7), generator=gen, dtype=torch.float64)
    sym = lambda col, mag: (2.0 * u[:, col] - 1.0) * mag  # noqa: E731  U(-mag, mag)
    s = 1.0 + sym(0, p.scale)
    tx = (0.5 + sym(1, p.translate)) * w
    ty = (0.5 + sym(2, p.translate)) * h
    flip = u[:, 3] < p.fliplr
    return s, tx, ty, flip, sym(4, p.hsv_h), 1.0 + sym(5, p.hsv_s), 1.0 + sym(6, p.hsv_v)


def draw_params(gen: torch.Generator, B: int, content_hw, padded_hw, p: AugmentParams | None = None) -> torch.Tensor:
    """One table row per image from the host generator ``gen`` (seven uniform
    draws per image, one call)."""
    return make_table(*_draw_terms(gen, B, content_hw, padded_hw, p or AugmentParams()), content_hw)


def draw_mosaic(gen: torch.Generator, b: int, content_hw, p: float):
    """The mosaic draws of a batch of ``b``: six uniforms per image in ONE call
    of their own (apply, xc, yc, three partners) -> (apply bool [b], xc [b],
    yc [b], partners [b, 3]; float64, integer-valued).  xc = floor(w/2 + u w),
    yc = floor(h/2 + u h), a partner = floor(u b): uniform over the batch."""
    h, w = content_hw
    u = torch.rand((b, 6), generator=gen, dtype=torch.float64)
    apply = u[:, 0] < p
    xc = torch.floor(w / 2.0 + u[:, 1] * w)
    yc = torch.floor(h / 2.0 + u[:, 2] * h)
    partners = torch.floor(u[:, 3:6] * b).clamp(max=b - 1)
    return apply, xc, yc, partners


def draw_mosaic_params(gen: torch.Generator, B: int, content_hw, padded_hw, mosaic: float,
                       p: AugmentParams | None = None) -> torch.Tensor:
    """One [B, 24] table: ``draw_params``' seven draws, then -- only when
    ``mosaic`` > 0 -- ``draw_mosaic``'s call; with ``mosaic`` = 0 every row is
    degenerate and the generator advances as ``draw_params`` advances it."""
    terms = _draw_terms(gen, B, content_hw, padded_hw, p or AugmentParams())
    if not mosaic > 0:
        return make_mosaic_table(*terms, content_hw)
    return make_mosaic_table(*terms, content_hw, *draw_mosaic(gen, B, content_hw, mosaic))


# ---------------------------------------------------------------------------
# plain-torch reference (CPU training path, test reference)
# ---------------------------------------------------------------------------
def _hsv_jitter(rgb, dh, gs, gv):
    """rgb [B,3,h,w]; dh, gs, gv [B,1,1]."""
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    mx = torch.maximum(r, torch.maximum(g, b))
    mn = torch.minimum(r, torch.minimum(g, b))
    d = mx - mn
    zero = torch.zeros_like(mx)
    s = torch.where(mx > 0, d / torch.where(mx > 0, mx, torch.ones_like(mx)), zero)
    is_r, is_g = mx == r, mx == g
    num = torch.where(is_r, g - b, torch.where(is_g, b - r, r - g))
    off = torch.where(is_r, zero, torch.where(is_g, zero + 2.0, zero + 4.0))
    h6 = torch.where(d > 0, off + num / torch.where(d > 0, d, torch.ones_like(d)), zero)
    hh = h6 / 6.0 + dh
    hh = hh - torch.floor(hh)
    s2 = torch.clamp(s * gs, max=1.0)
    v2 = torch.clamp(mx * gv, max=1.0)
    c = v2 * s2
    out = []
    for n in (5.0, 3.0, 1.0):
        k = n + 6.0 * hh
        k = torch.where(k >= 6.0, k - 6.0, k)
        a = torch.clamp(torch.minimum(k, 4.0 - k), 0.0, 1.0)
        out.append(v2 - c * a)
    return torch.stack(out, dim=1)


def reference_images(images, table, content_hw, fill=AugmentParams.fill, dtype=torch.float32):
    """The image half of ``augment_reference``: [B,3,Hp,Wp] in ``dtype``."""
    B, C, Hp, Wp = images.shape
    h, w = content_hw
    dev = images.device
    src = images[:, :, :h, :w]
    src = src.to(dtype) / 255.0 if images.dtype == torch.uint8 else src.to(dtype)
    src = src.reshape(B, C, h * w)
    t = table.to(device=dev, dtype=dtype)
    col = lambda i: t[:, i].reshape(B, 1, 1)  # noqa: E731
    xc = (torch.arange(w, device=dev, dtype=dtype) + 0.5).reshape(1, 1, w)
    yc = (torch.arange(h, device=dev, dtype=dtype) + 0.5).reshape(1, h, 1)
    u = (col(6) * xc + col(7) * yc) + col(8)
    v = (col(9) * xc + col(10) * yc) + col(11)
    fx, fy = u - 0.5, v - 0.5
    flx, fly = torch.floor(fx), torch.floor(fy)
    ax, ay = fx - flx, fy - fly
    inside = (flx >= -1) & (flx <= w - 1) & (fly >= -1) & (fly <= h - 1)   # some tap inside the content
    xi = torch.where(inside, flx, torch.zeros_like(flx)).to(torch.int64)
    yi = torch.where(inside, fly, torch.zeros_like(fly)).to(torch.int64)
    fillv = torch.full((), fill, dtype=dtype, device=dev)

    def tap(dx, dy):
        x, y = xi + dx, yi + dy
        ok = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
        idx = (y.clamp(0, h - 1) * w + x.clamp(0, w - 1)).reshape(B, 1, h * w).expand(B, C, h * w)
        val = src.gather(2, idx).reshape(B, C, h, w)
        return torch.where(ok.unsqueeze(1), val, fillv)

    w00, w01 = ((1.0 - ax) * (1.0 - ay)).unsqueeze(1), (ax * (1.0 - ay)).unsqueeze(1)
    w10, w11 = ((1.0 - ax) * ay).unsqueeze(1), (ax * ay).unsqueeze(1)
    val = tap(0, 0) * w00 + tap(1, 0) * w01 + tap(0, 1) * w10 + tap(1, 1) * w11
    active = ((t[:, 12] != 0) | (t[:, 13] != 1) | (t[:, 14] != 1)).reshape(B, 1, 1, 1)
    if bool(active.any()):
        val = torch.where(active, _hsv_jitter(val, col(12), col(13), col(14)), val)
    val = torch.where(inside.unsqueeze(1), val, fillv)
    out = torch.zeros((B, C, Hp, Wp), dtype=dtype, device=dev)
    out[:, :, :h, :w] = val
    return out


def box_terms(boxes, table, content_hw, padded_hw, dtype=torch.float32):
    """The mapped, clipped boxes and the terms of the keep test, per slot
    ([B, M] each): new xyxy in content pixels, new width / height, and
    ``area_ref`` = area_old s^2."""
    t = table.to(device=boxes.device, dtype=dtype)
    return _mapped_terms(*_content_xyxy(boxes.to(dtype), padded_hw), t, content_hw)


def _content_xyxy(bx, padded_hw):
    """cxcywh normalised to the padded tensor -> (x1, y1, x2, y2) in px."""
    Hp, Wp = padded_hw
    x1, x2 = (bx[..., 0] - 0.5 * bx[..., 2]) * Wp, (bx[..., 0] + 0.5 * bx[..., 2]) * Wp
    y1, y2 = (bx[..., 1] - 0.5 * bx[..., 3]) * Hp, (bx[..., 1] + 0.5 * bx[..., 3]) * Hp
    return x1, y1, x2, y2


def _mapped_terms(x1, y1, x2, y2, t, content_hw):
    """Boxes [B, N] (xyxy px in the frame the forward matrices of ``t`` take)
    -> ``box_terms``' dictionary."""
    h, w = content_hw
    col = lambda i: t[:, i].reshape(-1, 1)  # noqa: E731
    X1, X2 = col(0) * x1 + col(1) * y1 + col(2), col(0) * x2 + col(1) * y2 + col(2)
    Y1, Y2 = col(3) * x1 + col(4) * y1 + col(5), col(3) * x2 + col(4) * y2 + col(5)
    nx1, nx2 = torch.minimum(X1, X2).clamp(0, w), torch.maximum(X1, X2).clamp(0, w)
    ny1, ny2 = torch.minimum(Y1, Y2).clamp(0, h), torch.maximum(Y1, Y2).clamp(0, h)
    return {"x1": nx1, "y1": ny1, "x2": nx2, "y2": ny2, "w": nx2 - nx1, "h": ny2 - ny1,
            "area_ref": (x2 - x1) * (y2 - y1) * (col(15) * col(15))}


def reference_boxes(boxes, labels, n_valid, table, content_hw, padded_hw, dtype=torch.float32):
    """The box half of ``augment_reference``: (boxes [B,M,4] in ``dtype``,
    labels int64 [B,M], n_valid int32 [B], total fp32 scalar)."""
    B, M = labels.shape
    q = box_terms(boxes, table, content_hw, padded_hw, dtype)
    slot = torch.arange(M, device=boxes.device).reshape(1, M)
    return _keep_and_compact(q, slot < n_valid.reshape(B, 1).to(torch.int64), labels, padded_hw, M, dtype)


def _keep_and_compact(q, valid, labels, padded_hw, M_out, dtype):
    """The keep test on ``box_terms``' dictionary ([B, N] slots, ``valid`` the
    occupied ones, ``labels`` theirs), survivors compacted in slot order into
    [B, M_out] (the first M_out of them), PAD_BOX / label 0 behind."""
    Hp, Wp = padded_hw
    nw, nh = q["w"], q["h"]
    B, N = nw.shape
    dev = nw.device
    keep = valid & (nw >= 2) & (nh >= 2) \
        & (torch.maximum(nw, nh) < 100 * torch.minimum(nw, nh)) & (nw * nh > 0.1 * q["area_ref"])
    new = torch.stack([(q["x1"] + q["x2"]) * 0.5 / Wp, (q["y1"] + q["y2"]) * 0.5 / Hp, nw / Wp, nh / Hp], dim=-1)
    order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)   # survivors first, in their order
    count = keep.sum(dim=1).clamp(max=M_out)
    new, lab = new.gather(1, order.unsqueeze(-1).expand(B, N, 4)), labels.gather(1, order)
    if N < M_out:   # fewer slots than capacity: the tail is padding anyway
        new = torch.cat([new, new.new_zeros((B, M_out - N, 4))], dim=1)
        lab = torch.cat([lab, lab.new_zeros((B, M_out - N))], dim=1)
    new, lab = new[:, :M_out], lab[:, :M_out]
    live = torch.arange(M_out, device=dev).reshape(1, M_out) < count.reshape(B, 1)
    pad = torch.tensor(PAD_BOX, dtype=dtype, device=dev)
    out_b = torch.where(live.unsqueeze(-1), new, pad)
    out_l = torch.where(live, lab, torch.zeros_like(lab))
    return out_b, out_l, count.to(torch.int32), count.sum().to(torch.float32)


def augment_reference(images, boxes, labels, n_valid, table, content_hw, fill=AugmentParams.fill,
                      dtype=torch.float32):
    """Plain-torch augmentation of a batch in ``dtype`` (any float type) on the
    inputs' device.  images [B,3,Hp,Wp] uint8 (scaled by 1/255) or float, any
    layout; boxes / labels / n_valid the padded targets; table [B,16].
    -> (images [B,3,Hp,Wp], boxes [B,M,4], labels [B,M], n_valid int32 [B],
    total fp32 scalar)."""
    padded_hw = tuple(images.shape[-2:])
    img = reference_images(images, table, content_hw, fill, dtype)
    return (img, *reference_boxes(boxes, labels, n_valid, table, content_hw, padded_hw, dtype))


def _mosaic_cols(table, B_src, dev):
    """(xc [B], yc [B], sources [B, 4]) of a mosaic table as int64; an index
    outside [0, B_src) is an empty quadrant (-1)."""
    if table.dim() != 2 or table.shape[1] != MOSAIC_COLS:
        raise ValueError(f"a mosaic table is [B, {MOSAIC_COLS}], got {tuple(table.shape)}")
    ti = table.to(device=dev, dtype=torch.float64)
    q = ti[:, 18:22]
    q = torch.where((q >= 0) & (q < B_src), q, torch.full_like(q, -1.0)).to(torch.int64)
    return ti[:, 16].to(torch.int64), ti[:, 17].to(torch.int64), q


def mosaic_reference_images(images, table, content_hw, fill=AugmentParams.fill, dtype=torch.float32):
    """The image half of ``mosaic_reference``: images [B_src,3,Hp,Wp], table
    [B, 24] -> [B,3,Hp,Wp] in ``dtype``."""
    Bs, C, Hp, Wp = images.shape
    B = table.shape[0]
    h, w = content_hw
    dev = images.device
    src = images[:, :, :h, :w]
    src = src.to(dtype) / 255.0 if images.dtype == torch.uint8 else src.to(dtype)
    src = src.permute(0, 2, 3, 1).reshape(Bs * h * w, C)          # one row per source pixel
    cxm, cym, quad = _mosaic_cols(table, Bs, dev)
    cxm, cym = cxm.reshape(B, 1, 1), cym.reshape(B, 1, 1)
    quad = [quad[:, i].reshape(B, 1, 1) for i in range(4)]
    t = table.to(device=dev, dtype=dtype)
    col = lambda i: t[:, i].reshape(B, 1, 1)  # noqa: E731
    xc = (torch.arange(w, device=dev, dtype=dtype) + 0.5).reshape(1, 1, w)
    yc = (torch.arange(h, device=dev, dtype=dtype) + 0.5).reshape(1, h, 1)
    u = (col(6) * xc + col(7) * yc) + col(8)                      # canvas coordinates
    v = (col(9) * xc + col(10) * yc) + col(11)
    fx, fy = u - 0.5, v - 0.5
    flx, fly = torch.floor(fx), torch.floor(fy)
    ax, ay = fx - flx, fy - fly
    near = (flx >= -1) & (flx <= 2 * w - 1) & (fly >= -1) & (fly <= 2 * h - 1)   # some tap on the canvas
    X0 = torch.where(near, flx, torch.zeros_like(flx)).to(torch.int64)
    Y0 = torch.where(near, fly, torch.zeros_like(fly)).to(torch.int64)
    fillv = torch.full((), fill, dtype=dtype, device=dev)

    def tap(dx, dy):
        X, Y = X0 + dx, Y0 + dy
        right, bottom = X >= cxm, Y >= cym
        sx, sy = X - torch.where(right, cxm, cxm - w), Y - torch.where(bottom, cym, cym - h)
        idx = torch.where(bottom, torch.where(right, quad[3], quad[2]), torch.where(right, quad[1], quad[0]))
        ok = near & (X >= 0) & (X < 2 * w) & (Y >= 0) & (Y < 2 * h) & (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h) \
            & (idx >= 0)
        flat = (idx.clamp(min=0) * h + sy.clamp(0, h - 1)) * w + sx.clamp(0, w - 1)
        val = src.index_select(0, flat.reshape(-1)).reshape(B, h, w, C).permute(0, 3, 1, 2)
        return torch.where(ok.unsqueeze(1), val, fillv), ok

    w00, w01 = ((1.0 - ax) * (1.0 - ay)).unsqueeze(1), (ax * (1.0 - ay)).unsqueeze(1)
    w10, w11 = ((1.0 - ax) * ay).unsqueeze(1), (ax * ay).unsqueeze(1)
    (t00, k00), (t01, k01), (t10, k10), (t11, k11) = tap(0, 0), tap(1, 0), tap(0, 1), tap(1, 1)
    val = t00 * w00 + t01 * w01 + t10 * w10 + t11 * w11
    active = ((t[:, 12] != 0) | (t[:, 13] != 1) | (t[:, 14] != 1)).reshape(B, 1, 1, 1)
    if bool(active.any()):
        val = torch.where(active, _hsv_jitter(val, col(12), col(13), col(14)), val)
    val = torch.where((k00 | k01 | k10 | k11).unsqueeze(1), val, fillv)    # no valid tap: fill, no colour
    out = torch.zeros((B, C, Hp, Wp), dtype=dtype, device=dev)
    out[:, :, :h, :w] = val
    return out


def mosaic_box_terms(boxes, n_valid, table, content_hw, padded_hw, dtype=torch.float32):
    """``box_terms`` of the mosaic: per output image 4 M_in slots, quadrant-
    major (TL, TR, BL, BR, each the source's slots in order) -> (terms [B,
    4 M_in] each, occupied [B, 4 M_in] bool, sources [B, 4] int64)."""
    h, w = content_hw
    Bs, M = boxes.shape[:2]
    dev = boxes.device
    B = table.shape[0]
    cxm, cym, quad = _mosaic_cols(table, Bs, dev)
    t = table.to(device=dev, dtype=dtype)
    qs = quad.clamp(min=0)
    x1, y1, x2, y2 = _content_xyxy(boxes.to(dtype)[qs], padded_hw)          # [B, 4, M]
    right = torch.tensor([False, True, False, True], device=dev).reshape(1, 4)
    bottom = torch.tensor([False, False, True, True], device=dev).reshape(1, 4)
    ox = torch.where(right, cxm.reshape(B, 1), cxm.reshape(B, 1) - w).to(dtype).unsqueeze(-1)
    oy = torch.where(bottom, cym.reshape(B, 1), cym.reshape(B, 1) - h).to(dtype).unsqueeze(-1)
    flat = lambda v, o, hi: (v + o).clamp(0, hi).reshape(B, 4 * M)  # noqa: E731  shifted, clipped to the canvas
    terms = _mapped_terms(flat(x1, ox, 2 * w), flat(y1, oy, 2 * h), flat(x2, ox, 2 * w), flat(y2, oy, 2 * h), t,
                          content_hw)
    count = torch.where(quad >= 0, n_valid.to(torch.int64).clamp(0, M)[qs], torch.zeros_like(qs))
    occupied = torch.arange(M, device=dev).reshape(1, 1, M) < count.unsqueeze(-1)
    return terms, occupied.reshape(B, 4 * M), quad


def mosaic_reference_boxes(boxes, labels, n_valid, table, content_hw, padded_hw, M_out=None, dtype=torch.float32):
    """The box half of ``mosaic_reference``: inputs [B_src, M_in, ...], table
    [B, 24] -> (boxes [B,M_out,4] in ``dtype``, labels int64 [B,M_out],
    n_valid int32 [B], total fp32 scalar); M_out defaults to M_in."""
    M = labels.shape[1]
    B = table.shape[0]
    terms, occupied, quad = mosaic_box_terms(boxes, n_valid, table, content_hw, padded_hw, dtype)
    lab = labels[quad.clamp(min=0)].reshape(B, 4 * M)
    return _keep_and_compact(terms, occupied, lab, padded_hw, M if M_out is None else int(M_out), dtype)


def mosaic_reference(images, boxes, labels, n_valid, table, content_hw, M_out=None, fill=AugmentParams.fill,
                     dtype=torch.float32):
    """Plain-torch mosaic augmentation of a batch in ``dtype`` on the inputs'
    device: ``augment_reference`` with a [B, 24] table and an output capacity
    M_out (default M_in).  -> (images, boxes [B,M_out,4], labels [B,M_out],
    n_valid int32 [B], total fp32 scalar)."""
    padded_hw = tuple(images.shape[-2:])
    img = mosaic_reference_images(images, table, content_hw, fill, dtype)
    return (img, *mosaic_reference_boxes(boxes, labels, n_valid, table, content_hw, padded_hw, M_out, dtype))


# ---------------------------------------------------------------------------
# HIP wrappers
# ---------------------------------------------------------------------------
_SRC_DTYPES = {torch.uint8: 0, torch.float32: 1}
_DST_DTYPES = {torch.bfloat16: 0, torch.float32: 1}


def _need_gpu(t, name):
    from ..moe._lib import MoEKernelError

    if not t.is_cuda:
        raise MoEKernelError(f"{name} must be a GPU tensor (HIP path has no CPU fallback)")


def augment_images_hip(src, table, out, content_hw, fill=AugmentParams.fill):
    """train_augment_images: src [B,3,Hp,Wp] uint8 / fp32 with any strides ->
    out (bf16 / fp32, channels_last, same shape)."""
    from ..moe import _lib as L

    for t, n in ((src, "src"), (table, "table"), (out, "out")):
        _need_gpu(t, n)
    if src.dtype not in _SRC_DTYPES or out.dtype not in _DST_DTYPES:
        raise L.MoEKernelError(f"augment_images: src {src.dtype} / out {out.dtype} not supported "
                               "(uint8 or fp32 in, bf16 or fp32 out)")
    B, C, Hp, Wp = src.shape
    if C != 3 or tuple(out.shape) != (B, C, Hp, Wp) or not out.is_contiguous(memory_format=torch.channels_last):
        raise L.MoEKernelError("augment_images: out must be a channels_last [B,3,Hp,Wp] tensor of src's shape")
    if table.dtype != torch.float32 or tuple(table.shape) != (B, TABLE_COLS) or not table.is_contiguous():
        raise L.MoEKernelError(f"augment_images: table must be a contiguous fp32 [{B}, {TABLE_COLS}] tensor")
    sn, sc, sh, sw = src.stride()
    L._check(L.lib().train_augment_images(L._ptr(src), _SRC_DTYPES[src.dtype], sn, sc, sh, sw, L._ptr(out),
                                          _DST_DTYPES[out.dtype], L._ptr(table), B, Hp, Wp, int(content_hw[0]),
                                          int(content_hw[1]), float(fill), L._stream()), "train_augment_images")
    return out


def augment_boxes_hip(boxes, labels, n_valid, table, content_hw, padded_hw, out=None):
    """train_augment_boxes -> (boxes, labels, n_valid, total), written into
    ``out`` (the same four tensors) when given."""
    from ..moe import _lib as L

    for t, n in ((boxes, "boxes"), (labels, "labels"), (n_valid, "n_valid"), (table, "table")):
        _need_gpu(t, n)
    L._need(boxes, torch.float32, "boxes")
    L._need(labels, torch.int64, "labels")
    L._need(n_valid, torch.int32, "n_valid")
    L._need(table, torch.float32, "table")
    B, M = labels.shape
    if tuple(boxes.shape) != (B, M, 4) or n_valid.numel() != B or tuple(table.shape) != (B, TABLE_COLS):
        raise L.MoEKernelError("augment_boxes: want boxes [B,M,4], labels [B,M], n_valid [B], table [B,16]")
    if out is None:
        out = (torch.empty_like(boxes), torch.empty_like(labels), torch.empty_like(n_valid),
               torch.empty((), dtype=torch.float32, device=boxes.device))
    ob, ol, onv, total = out
    L._need(ob, torch.float32, "boxes_out")
    L._need(ol, torch.int64, "labels_out")
    L._need(onv, torch.int32, "n_valid_out")
    L._need(total, torch.float32, "total_out")
    if tuple(ob.shape) != (B, M, 4) or tuple(ol.shape) != (B, M) or onv.numel() != B or total.numel() != 1:
        raise L.MoEKernelError("augment_boxes: output shapes differ from the inputs'")
    L._check(L.lib().train_augment_boxes(L._ptr(boxes), L._ptr(labels), L._ptr(n_valid), L._ptr(table), B, M,
                                         int(padded_hw[0]), int(padded_hw[1]), int(content_hw[0]),
                                         int(content_hw[1]), L._ptr(ob), L._ptr(ol), L._ptr(onv), L._ptr(total),
                                         L._stream()), "train_augment_boxes")
    return ob, ol, onv, total


def mosaic_images_hip(src, table, out, content_hw, fill=AugmentParams.fill):
    """train_mosaic_images: src [B_src,3,Hp,Wp] uint8 / fp32 with any strides,
    table [B, 24] -> out (bf16 / fp32, channels_last, [B,3,Hp,Wp])."""
    from ..moe import _lib as L

    for t, n in ((src, "src"), (table, "table"), (out, "out")):
        _need_gpu(t, n)
    if src.dtype not in _SRC_DTYPES or out.dtype not in _DST_DTYPES:
        raise L.MoEKernelError(f"mosaic_images: src {src.dtype} / out {out.dtype} not supported "
                               "(uint8 or fp32 in, bf16 or fp32 out)")
    Bs, C, Hp, Wp = src.shape
    B = out.shape[0]
    if C != 3 or tuple(out.shape) != (B, C, Hp, Wp) or not out.is_contiguous(memory_format=torch.channels_last):
        raise L.MoEKernelError("mosaic_images: out must be a channels_last [B,3,Hp,Wp] tensor of src's image shape")
    if table.dtype != torch.float32 or tuple(table.shape) != (B, MOSAIC_COLS) or not table.is_contiguous():
        raise L.MoEKernelError(f"mosaic_images: table must be a contiguous fp32 [{B}, {MOSAIC_COLS}] tensor")
    sn, sc, sh, sw = src.stride()
    L._check(L.lib().train_mosaic_images(L._ptr(src), _SRC_DTYPES[src.dtype], sn, sc, sh, sw, Bs, L._ptr(out),
                                         _DST_DTYPES[out.dtype], L._ptr(table), B, Hp, Wp, int(content_hw[0]),
                                         int(content_hw[1]), float(fill), L._stream()), "train_mosaic_images")
    return out


def mosaic_boxes_hip(boxes, labels, n_valid, table, content_hw, padded_hw, M_out=None, out=None):
    """train_mosaic_boxes: inputs [B,M_in,...] -> (boxes [B,M_out,4], labels
    [B,M_out], n_valid, total), written into ``out`` (the same four tensors,
    whose shape gives M_out) when given; M_out defaults to M_in."""
    from ..moe import _lib as L

    for t, n in ((boxes, "boxes"), (labels, "labels"), (n_valid, "n_valid"), (table, "table")):
        _need_gpu(t, n)
    L._need(boxes, torch.float32, "boxes")
    L._need(labels, torch.int64, "labels")
    L._need(n_valid, torch.int32, "n_valid")
    L._need(table, torch.float32, "table")
    B, M = labels.shape
    if tuple(boxes.shape) != (B, M, 4) or n_valid.numel() != B or tuple(table.shape) != (B, MOSAIC_COLS):
        raise L.MoEKernelError(f"mosaic_boxes: want boxes [B,M,4], labels [B,M], n_valid [B], table [B,{MOSAIC_COLS}]")
    if out is None:
        Mo = M if M_out is None else int(M_out)
        out = (torch.empty((B, Mo, 4), dtype=torch.float32, device=boxes.device),
               torch.empty((B, Mo), dtype=torch.int64, device=boxes.device), torch.empty_like(n_valid),
               torch.empty((), dtype=torch.float32, device=boxes.device))
    ob, ol, onv, total = out
    L._need(ob, torch.float32, "boxes_out")
    L._need(ol, torch.int64, "labels_out")
    L._need(onv, torch.int32, "n_valid_out")
    L._need(total, torch.float32, "total_out")
    Mo = ol.shape[1] if ol.dim() == 2 else -1
    if (M_out is not None and Mo != int(M_out)) or tuple(ob.shape) != (B, Mo, 4) or tuple(ol.shape) != (B, Mo) \
            or onv.numel() != B or total.numel() != 1:
        raise L.MoEKernelError("mosaic_boxes: want boxes_out [B,M_out,4], labels_out [B,M_out], n_valid_out [B] "
                               "and a scalar total")
    L._check(L.lib().train_mosaic_boxes(L._ptr(boxes), L._ptr(labels), L._ptr(n_valid), L._ptr(table), B, M, Mo,
                                        int(padded_hw[0]), int(padded_hw[1]), int(content_hw[0]),
                                        int(content_hw[1]), L._ptr(ob), L._ptr(ol), L._ptr(onv), L._ptr(total),
                                        L._stream()), "train_mosaic_boxes")
    return ob, ol, onv, total


# ---------------------------------------------------------------------------
# the stateful front end
# ---------------------------------------------------------------------------
class BatchAugment:
    """Owns the parameter generator, the pinned staging of the table and the
    output buffers of one training loop.  ``__call__`` draws a table (or takes
    ``table=``), uploads it and augments the batch: the two HIP kernels on the
    GPU, ``augment_reference`` on the CPU.  ``raw_targets(M)`` hands out the
    padded buffers a caller pads the incoming targets into (the kernels never
    compact in place).  ``B`` is the capacity: a shorter batch (the last one of
    an epoch when the loader keeps it) draws one row per image it has and uses
    the leading part of every buffer.

    ``mosaic``: the probability that an image becomes a four-image mosaic; it
    may be changed between steps.  Once it has been positive the object stays
    on the mosaic path -- [B, 24] tables, the mosaic kernels /
    ``mosaic_reference``, an output capacity ``M_out`` apart from the raw
    buffers' ``M_in`` (``out_targets``' shape, or ``M_out=``) -- and a later 0
    draws degenerate rows for the same kernels.  With 0 from the start nothing
    differs from the plain path."""

    _RING = 4  # pinned staging slots: a slot is reused only after its upload completed

    def __init__(self, B, content_hw, padded_hw, device, *, seed=0, rank=0, params: AugmentParams | None = None,
                 out_dtype=torch.float32, mosaic=0.0):
        self.B = int(B)
        self.content_hw = (int(content_hw[0]), int(content_hw[1]))
        self.padded_hw = (int(padded_hw[0]), int(padded_hw[1]))
        self.device = torch.device(device)
        self.params = params or AugmentParams()
        self.out_dtype = out_dtype
        self.generator = torch.Generator()
        self.generator.manual_seed(int(seed) * 1000 + int(rank))
        self.table_host = None   # the last table, on the host
        self.total = torch.zeros((), dtype=torch.float32, device=self.device)
        self._gpu = self.device.type == "cuda"
        self._events = [None] * self._RING
        self._slot = 0
        self._raw = None
        self._out_targets = None
        self._out_images = None
        self.mosaic_path = False
        self._mosaic = 0.0
        self._alloc_table(TABLE_COLS)
        self.mosaic = mosaic

    def _alloc_table(self, cols):
        self.cols = cols
        self.table = torch.empty((self.B, cols), dtype=torch.float32, device=self.device)
        self._staging = [torch.empty((self.B, cols), dtype=torch.float32).pin_memory()
                         for _ in range(self._RING)] if self._gpu else []

    @property
    def mosaic(self) -> float:
        return self._mosaic

    @mosaic.setter
    def mosaic(self, p):
        p = float(p)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"mosaic probability {p} outside [0, 1]")
        self._mosaic = p
        if p > 0 and not self.mosaic_path:
            self.mosaic_path = True
            if self._gpu:
                torch.cuda.current_stream().synchronize()   # uploads in flight read the old staging
            self._events = [None] * self._RING
            self._alloc_table(MOSAIC_COLS)

    def draw(self, b=None) -> torch.Tensor:
        """One table row per image of a batch of ``b`` (default: the capacity B)."""
        b = self.B if b is None else int(b)
        if self.mosaic_path:
            return draw_mosaic_params(self.generator, b, self.content_hw, self.padded_hw, self._mosaic, self.params)
        return draw_params(self.generator, b, self.content_hw, self.padded_hw, self.params)

    def need(self, counts, table=None) -> int:
        """The most boxes an output image of ``table`` (default: the last one
        uploaded) can hold, from the raw per-image ``counts`` on the host: max
        over n of the counts of its four sources (a plain table: max count)."""
        table = self.table_host if table is None else table
        counts = [int(c) for c in counts]
        if table is None or table.shape[1] != MOSAIC_COLS:
            return max(counts, default=0)
        src = table[:, 18:22].to(torch.int64).tolist()
        return max((sum(counts[i] for i in row if 0 <= i < len(counts)) for row in src), default=0)

    def upload(self, table: torch.Tensor) -> torch.Tensor:
        """Host table [b <= B, 16 or 24 (the mosaic path)] -> the leading rows
        of ``self.table`` (pinned, non-blocking on the GPU); returns those rows."""
        b = table.shape[0]
        if table.dim() != 2 or not 1 <= b <= self.B or table.shape[1] != self.cols:
            raise ValueError(f"augmentation table must be [1..{self.B}, {self.cols}], got {tuple(table.shape)}")
        self.table_host = table.detach().to("cpu", torch.float32)
        dst = self.table[:b]
        if not self._gpu:
            dst.copy_(self.table_host)
            return dst
        i = self._slot
        self._slot = (i + 1) % self._RING
        if self._events[i] is not None:
            self._events[i].synchronize()
        self._staging[i][:b].copy_(self.table_host)
        dst.copy_(self._staging[i][:b], non_blocking=True)
        self._events[i] = torch.cuda.Event()
        self._events[i].record()
        return dst

    def raw_targets(self, M, b=None):
        """(boxes [b,M,4], labels [b,M], n_valid [b]) to pad the incoming
        targets of a batch of ``b`` (default B) into (M is the mosaic path's M_in)."""
        if self._raw is None or self._raw[0].shape[1] != M:
            self._raw = (torch.empty((self.B, M, 4), dtype=torch.float32, device=self.device),
                         torch.empty((self.B, M), dtype=torch.int64, device=self.device),
                         torch.empty(self.B, dtype=torch.int32, device=self.device))
        return self._raw if b is None else tuple(t[:b] for t in self._raw)

    def _own_targets(self, M, b):
        if self._out_targets is None or self._out_targets[0].shape[1] != M:
            self._out_targets = (torch.empty((self.B, M, 4), dtype=torch.float32, device=self.device),
                                 torch.empty((self.B, M), dtype=torch.int64, device=self.device),
                                 torch.empty(self.B, dtype=torch.int32, device=self.device))
        return tuple(t[:b] for t in self._out_targets)

    def _own_images(self, b):
        if self._out_images is None:
            self._out_images = torch.empty((self.B, 3, *self.padded_hw), dtype=self.out_dtype, device=self.device,
                                           memory_format=torch.channels_last)
        return self._out_images[:b]

    def __call__(self, images, boxes, labels, n_valid, *, out_images=None, out_targets=None, table=None,
                 M_out=None):
        """-> (images, boxes, labels, n_valid, total).  ``out_images`` /
        ``out_targets`` (boxes, labels, n_valid): destinations (a graphed
        step's static buffers); default: this object's own buffers, on the
        mosaic path of capacity ``M_out`` (default: the inputs' M)."""
        b = images.shape[0]
        if not 1 <= b <= self.B or tuple(images.shape[1:]) != (3, *self.padded_hw):
            raise ValueError(f"BatchAugment was built for batches of up to {(self.B, 3, *self.padded_hw)}, "
                             f"got {tuple(images.shape)}")
        if labels.shape[0] != b:
            raise ValueError(f"{b} images but targets of {labels.shape[0]}")
        dev_table = self.upload(self.draw(b) if table is None else table)
        if dev_table.shape[0] != b:
            raise ValueError(f"a table of {dev_table.shape[0]} rows for a batch of {b}")
        M = labels.shape[1]
        if M_out is not None and not self.mosaic_path:
            raise ValueError("M_out belongs to the mosaic path (the plain kernels keep the inputs' M)")
        out_images = self._own_images(b) if out_images is None else out_images
        ob, ol, onv = self._own_targets(M if M_out is None else int(M_out), b) if out_targets is None else out_targets
        if self._gpu and self.mosaic_path:
            mosaic_images_hip(images, dev_table, out_images, self.content_hw, self.params.fill)
            mosaic_boxes_hip(boxes, labels, n_valid, dev_table, self.content_hw, self.padded_hw,
                             out=(ob, ol, onv, self.total))
        elif self._gpu:
            augment_images_hip(images, dev_table, out_images, self.content_hw, self.params.fill)
            augment_boxes_hip(boxes, labels, n_valid, dev_table, self.content_hw, self.padded_hw,
                              out=(ob, ol, onv, self.total))
        else:
            dt = out_images.dtype
            dt = dt if dt.is_floating_point else torch.float32
            if self.mosaic_path:
                img, rb, rl, rnv, total = mosaic_reference(images, boxes, labels, n_valid, dev_table, self.content_hw,
                                                           ol.shape[1], self.params.fill, dt)
            else:
                img, rb, rl, rnv, total = augment_reference(images, boxes, labels, n_valid, dev_table,
                                                            self.content_hw, self.params.fill, dt)
            out_images.copy_(img)
            ob.copy_(rb)
            ol.copy_(rl)
            onv.copy_(rnv)
            self.total.copy_(total)
        return out_images, ob, ol, onv, self.total


def targets_from_padded(boxes, labels, n_valid):
    """Padded targets -> the list of {"boxes", "labels"} the eager criterion
    takes (one host read of n_valid)."""
    counts = n_valid.tolist()
    return [{"boxes": boxes[b, :n].clone(), "labels": labels[b, :n].clone()} for b, n in enumerate(counts)]
