"""Numpy restatement of the batched augmentation (TEST INFRASTRUCTURE ONLY): the staged definition of
cvl_augment_batch (include/cvlite.h), every stage really materialised -- the canvas is built, the crop
sliced, the flip and the resize made on whole arrays -- plus the box pipeline and the composition of
the colour map, each written independently of cvlite/augment.py.  The resize is
oracle.preprocess_ref.resize_bilinear."""
import math

import numpy as np

from oracle.preprocess_ref import resize_bilinear

f32 = np.float32
BT601 = np.array([0.299, 0.587, 0.114], np.float64)
YIQ = np.array([[0.299, 0.587, 0.114],
                [0.595716, -0.274453, -0.321263],
                [0.211456, -0.522591, 0.311135]], np.float64)


def augment_image(src, canvas, crop, flip, out_hw, pad_hw, m, t, fill):
    """src [H,W,3] uint8 / fp32; canvas = (ch, cw, oy, ox); crop = (y0, x0, hh, ww); out_hw = (oh, ow);
    pad_hw = (ph, pw); m [3,3], t [3], fill [3] fp32 -> [ph, pw, 3] fp32."""
    a = np.asarray(src).astype(f32)
    H, W = a.shape[:2]
    ch, cw, oy, ox = canvas
    cv = np.empty((ch, cw, 3), f32)                       # 1. zoom-out
    cv[:] = np.asarray(fill, f32)
    cv[oy:oy + H, ox:ox + W] = a
    y0, x0, hh, ww = crop
    c = cv[y0:y0 + hh, x0:x0 + ww]                        # 2. crop
    assert c.shape[:2] == (hh, ww)
    if flip:                                              # 3. flip
        c = c[:, ::-1]
    r = resize_bilinear(c, out_hw[0], out_hw[1])          # 4. resize
    m = np.asarray(m, f32).reshape(3, 3)
    t = np.asarray(t, f32).reshape(3)
    v = np.empty_like(r)                                  # 5. colour, ((m0 r + m1 g) + m2 b) + t in fp32
    for k in range(3):
        v[..., k] = ((m[k, 0] * r[..., 0] + m[k, 1] * r[..., 1]) + m[k, 2] * r[..., 2]) + t[k]
    out = np.zeros((pad_hw[0], pad_hw[1], 3), f32)        # 6. normalise and pad
    out[:out_hw[0], :out_hw[1]] = v / f32(127.5) - f32(1.0)
    return out


def augment_plan(src, p):
    """augment_image of a cvlite.augment.Plan."""
    return augment_image(src, (p.ch, p.cw, p.oy, p.ox), (p.y0, p.x0, p.hh, p.ww), p.flip, (p.oh, p.ow), (p.ph, p.pw),
                         p.m, p.t, p.fill)


# ---- colour: step by step in float64 -------------------------------------------------------------------
def colour_steps(v, brightness=0.0, contrast=1.0, saturation=1.0, hue=0.0, perm=(0, 1, 2), contrast_first=True):
    """The photometric chain applied to pixels v [..., 3] one step at a time in float64: brightness,
    [contrast], saturation, hue, [contrast], permutation."""
    v = np.asarray(v, np.float64) + brightness
    if contrast_first:
        v = v * contrast
    grey = (v * BT601).sum(-1, keepdims=True)
    v = grey + saturation * (v - grey)
    a = math.radians(hue)
    yiq = v @ YIQ.T
    rot = np.stack([yiq[..., 0], math.cos(a) * yiq[..., 1] - math.sin(a) * yiq[..., 2],
                    math.sin(a) * yiq[..., 1] + math.cos(a) * yiq[..., 2]], -1)
    v = rot @ np.linalg.inv(YIQ).T
    if not contrast_first:
        v = v * contrast
    return v[..., list(perm)]


def apply_affine_f32(v, m, t):
    """The kernel's stage 5 on fp32 pixels [..., 3]."""
    v = np.asarray(v, f32)
    m, t = np.asarray(m, f32).reshape(3, 3), np.asarray(t, f32).reshape(3)
    return np.stack([((m[k, 0] * v[..., 0] + m[k, 1] * v[..., 1]) + m[k, 2] * v[..., 2]) + t[k] for k in range(3)], -1)


# ---- boxes ---------------------------------------------------------------------------------------------
def iou(patch, box):
    """IoU of two (x1, y1, x2, y2) rectangles, float64."""
    iw = max(0.0, min(float(patch[2]), float(box[2])) - max(float(patch[0]), float(box[0])))
    ih = max(0.0, min(float(patch[3]), float(box[3])) - max(float(patch[1]), float(box[1])))
    ua = (float(patch[2]) - float(patch[0])) * (float(patch[3]) - float(patch[1]))
    ub = (float(box[2]) - float(box[0])) * (float(box[3]) - float(box[1]))
    return iw * ih / (ua + ub - iw * ih)


def boxes_through(boxes_xyxy_norm, hw, canvas, crop, flip):
    """Normalised (x1, y1, x2, y2) boxes of an H x W source through zoom-out canvas = (ch, cw, oy, ox), crop
    = (y0, x0, hh, ww) and flip, one box at a time in fp32 -> ((yc, xc, h, w) normalised to the crop [n,4],
    kept indices)."""
    H, W = hw
    _, _, oy, ox = canvas
    y0, x0, hh, ww = crop
    out, keep = [], []
    for i, b in enumerate(np.asarray(boxes_xyxy_norm, f32).reshape(-1, 4)):
        x1, y1 = b[0] * f32(W) + f32(ox), b[1] * f32(H) + f32(oy)
        x2, y2 = b[2] * f32(W) + f32(ox), b[3] * f32(H) + f32(oy)
        cx, cy = (x1 + x2) / f32(2.0), (y1 + y2) / f32(2.0)
        if not (x0 < cx < x0 + ww and y0 < cy < y0 + hh):
            continue
        x1, x2 = (min(max(v, f32(x0)), f32(x0 + ww)) - f32(x0) for v in (x1, x2))
        y1, y2 = (min(max(v, f32(y0)), f32(y0 + hh)) - f32(y0) for v in (y1, y2))
        x1, x2, y1, y2 = x1 / f32(ww), x2 / f32(ww), y1 / f32(hh), y2 / f32(hh)
        if flip:
            x1, x2 = f32(1.0) - x2, f32(1.0) - x1
        out.append([(y1 + y2) / f32(2.0), (x1 + x2) / f32(2.0), y2 - y1, x2 - x1])
        keep.append(i)
    return np.array(out, f32).reshape(-1, 4), np.array(keep, np.int64)
