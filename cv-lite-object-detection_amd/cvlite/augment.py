"""Batched training augmentation on MI355X (cvlite extension, beyond the reference; DESIGN.md
"Batched augmentation"): photometric distortion, zoom-out and the IoU-constrained random crop of the
SSD / RetinaNet pipelines, with the flip, jittered resize, normalisation and pad of
data_preprocess.preprocess_data, for a whole batch of decoded images of different sizes in ONE
cvl_augment_batch launch (csrc/augment.hip).

  AugmentPolicy                        what is drawn; every part can be switched off on its own
  colour_affine(...)                   brightness / contrast / saturation / hue / permutation -> (M, t)
  plan_image(hw, boxes, labels, ...)   the draws of one image -> Plan (host only, numpy)
  plan_geometry(H, W, ...)             a Plan from explicit values, no draws
  run_plans(images, plans, out=None)   one descriptor table, one copy, one launch -> device images
  plan_table(plans)                    the host table torch.ops.cvlite.augment_images takes
  augment_batch(images, boxes, ...)    plan_image of every image + run_plans + the trainer's box arrays

Per image the pixels are defined as: zoom-out (source at an integer offset on a canvas of `fill`),
crop (an integer rectangle of the canvas), left-right flip of the crop, bilinear resize (the arithmetic
of cvl_resize_pad_normalize), colour v' = M v + t, / 127.5 - 1, zero pad.  The colour transform is
affine and is applied AFTER the resampling, to the fill too: brightness, contrast, saturation (a blend
with the BT.601 grey value), hue (a rotation about the grey axis in YIQ) and a channel permutation
compose into one 3x3 matrix and one offset on the host -- no HSV round trip per pixel, no clipping.
(mmdet's PhotoMetricDistortion works on the source pixels in HSV and its Expand fills with the plain
mean; the two agree where the colour map is the identity.)

Draw order per image (numpy Generator): the flip, the resize jitter (the two draws of
data_preprocess.preprocess_data / padded_size, in their order, so AugmentPolicy.identity() consumes
exactly the draws of today's path), the photometric parameters, the zoom-out, the crop.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .data_preprocess import _plan, box_targets

f32 = np.float32

BT601 = (0.299, 0.587, 0.114)
# RGB -> YIQ (NTSC); the hue rotation turns the (I, Q) plane and leaves Y, the grey axis, alone
_YIQ = np.array([[0.299, 0.587, 0.114],
                 [0.595716, -0.274453, -0.321263],
                 [0.211456, -0.522591, 0.311135]], np.float64)
_YIQ_INV = np.linalg.inv(_YIQ)

# cvl_augment_desc (include/cvlite.h), 144 bytes
DESC = np.dtype([("src", np.uint64), ("dst", np.uint64), ("src_u8", np.int32), ("H", np.int32), ("W", np.int32),
                 ("ch", np.int32), ("cw", np.int32), ("oy", np.int32), ("ox", np.int32),
                 ("y0", np.int32), ("x0", np.int32), ("hh", np.int32), ("ww", np.int32), ("flip", np.int32),
                 ("oh", np.int32), ("ow", np.int32), ("ph", np.int32), ("pw", np.int32),
                 ("m", np.float32, 9), ("t", np.float32, 3), ("fill", np.float32, 3), ("reserved", np.int32)],
                align=True)
assert DESC.itemsize == 144
MAX_BATCH = 4096          # CVL_AUGMENT_MAX_BATCH
_EYE, _ZERO3 = np.eye(3, dtype=f32), np.zeros(3, f32)
_INT_FIELDS = ("H", "W", "ch", "cw", "oy", "ox", "y0", "x0", "hh", "ww", "flip", "oh", "ow", "ph", "pw")
CROP_TRIES = 50


def _range(name, v):
    if v is None:
        return None
    lo, hi = (float(x) for x in v)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError("AugmentPolicy.%s must be (low, high) with low <= high, not %r" % (name, v))
    return (lo, hi)


class AugmentPolicy(object):
    """What augment_batch draws.  A part is off with: flip=0, brightness=0, contrast=None,
    saturation=None, hue=0, swap_channels=False (or photo_prob=0 for all five), expand=None (or
    expand_prob=0), min_ious=None.
      flip          probability of the left-right mirror
      brightness    delta ~ U(-brightness, brightness), added
      contrast      factor ~ U(low, high), multiplied (mmdet's PhotoMetricDistortion), drawn to act
                    before or after saturation / hue with equal probability
      saturation    factor ~ U(low, high): a blend with the BT.601 grey value
      hue           angle ~ U(-hue, hue) degrees about the grey axis in YIQ
      swap_channels a random permutation of the channels
      photo_prob    the probability each of those five is applied with
      expand        zoom-out ratio ~ U(low, high), with probability expand_prob, on a canvas of `fill`
      min_ious      MinIoURandomCrop's thresholds; min_crop the smallest patch side / image side"""

    def __init__(self, flip=0.5, brightness=32.0, contrast=(0.5, 1.5), saturation=(0.5, 1.5), hue=18.0,
                 swap_channels=True, photo_prob=0.5, expand=(1.0, 4.0), expand_prob=0.5,
                 fill=(123.675, 116.28, 103.53), min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop=0.3):
        self.flip, self.brightness, self.hue = float(flip), float(brightness), float(hue)
        self.contrast, self.saturation = _range("contrast", contrast), _range("saturation", saturation)
        self.swap_channels, self.photo_prob = bool(swap_channels), float(photo_prob)
        self.expand, self.expand_prob = _range("expand", expand), float(expand_prob)
        self.fill = tuple(float(v) for v in fill)
        self.min_ious = None if min_ious is None else tuple(float(v) for v in min_ious)
        self.min_crop = float(min_crop)
        for name in ("flip", "photo_prob", "expand_prob"):
            if not 0.0 <= getattr(self, name) <= 1.0:
                raise ValueError("AugmentPolicy.%s is a probability, not %r" % (name, getattr(self, name)))
        if not (self.brightness >= 0.0 and self.hue >= 0.0):
            raise ValueError("AugmentPolicy.brightness and hue are half-widths >= 0")
        if self.contrast is not None and self.contrast[0] < 0.0 or self.saturation is not None and self.saturation[0] < 0.0:
            raise ValueError("AugmentPolicy.contrast and saturation factors are >= 0")
        if self.expand is not None and self.expand[0] < 1.0:
            raise ValueError("AugmentPolicy.expand ratios are >= 1, not %r" % (expand,))
        if len(self.fill) != 3:
            raise ValueError("AugmentPolicy.fill holds one value per channel")
        if self.min_ious is not None and not all(0.0 < v < 1.0 for v in self.min_ious):
            raise ValueError("AugmentPolicy.min_ious lie strictly between 0 and 1, not %r" % (min_ious,))
        if not 0.0 < self.min_crop <= 1.0:
            raise ValueError("AugmentPolicy.min_crop must lie in (0, 1], not %r" % (min_crop,))

    @classmethod
    def identity(cls):
        """Flip only: the draws and the results of data_preprocess.preprocess_data."""
        return cls(flip=0.5, brightness=0.0, contrast=None, saturation=None, hue=0.0, swap_channels=False,
                   expand=None, min_ious=None)

    def __repr__(self):
        return "AugmentPolicy(%s)" % ", ".join("%s=%r" % kv for kv in sorted(vars(self).items()))


# -------------------------------------------------------------------------------------------------
# colour
# -------------------------------------------------------------------------------------------------
def hue_matrix(degrees):
    """Rotation by `degrees` about the grey axis in YIQ, as an RGB 3x3 (float64): I + YIQ^-1 (R - I) YIQ,
    so 0 degrees is the identity exactly."""
    a = math.radians(float(degrees))
    c, s = math.cos(a), math.sin(a)
    r = np.array([[0.0, 0.0, 0.0], [0.0, c - 1.0, -s], [0.0, s, c - 1.0]], np.float64)
    return np.eye(3) + _YIQ_INV @ r @ _YIQ


def saturation_matrix(factor):
    """v' = grey + factor * (v - grey), grey = BT.601 luma of v (float64 3x3)."""
    s = float(factor)
    return s * np.eye(3) + (1.0 - s) * np.outer(np.ones(3), np.array(BT601, np.float64))


def colour_affine(brightness=0.0, contrast=1.0, saturation=1.0, hue=0.0, perm=(0, 1, 2), contrast_first=True):
    """The composition, in the order brightness, [contrast], saturation, hue, [contrast], permutation, of
    v + brightness, v * contrast, saturation_matrix, hue_matrix and v'[i] = v[perm[i]] as one affine map
    v' = M v + t: composed in float64, rounded once to fp32 -> (M [3,3] fp32, t [3] fp32)."""
    A, c = np.eye(3), np.zeros(3)
    c = c + float(brightness)
    if contrast_first:
        A, c = A * float(contrast), c * float(contrast)
    for L in (saturation_matrix(saturation), hue_matrix(hue)):
        A, c = L @ A, L @ c
    if not contrast_first:
        A, c = A * float(contrast), c * float(contrast)
    p = [int(i) for i in perm]
    if sorted(p) != [0, 1, 2]:
        raise ValueError("perm must be a permutation of (0, 1, 2), not %r" % (perm,))
    return A[p].astype(f32), c[p].astype(f32)


def _draw_colour(policy, rng):
    p = policy.photo_prob
    kw = {}
    if policy.brightness > 0.0 and rng.uniform() < p:
        kw["brightness"] = rng.uniform(-policy.brightness, policy.brightness)
    if policy.contrast is not None and rng.uniform() < p:
        kw["contrast"] = rng.uniform(*policy.contrast)
        kw["contrast_first"] = bool(rng.integers(2))
    if policy.saturation is not None and rng.uniform() < p:
        kw["saturation"] = rng.uniform(*policy.saturation)
    if policy.hue > 0.0 and rng.uniform() < p:
        kw["hue"] = rng.uniform(-policy.hue, policy.hue)
    if policy.swap_channels and rng.uniform() < p:
        kw["perm"] = tuple(int(i) for i in rng.permutation(3))
    return kw


# -------------------------------------------------------------------------------------------------
# geometry
# -------------------------------------------------------------------------------------------------
def centres_inside(patch, boxes):
    """Which pixel boxes [N,4] have their centre STRICTLY inside the integer patch (x1, y1, x2, y2)."""
    b = np.asarray(boxes, f32).reshape(-1, 4)
    cx, cy = (b[:, 0] + b[:, 2]) / f32(2.0), (b[:, 1] + b[:, 3]) / f32(2.0)
    return (cx > patch[0]) & (cx < patch[2]) & (cy > patch[1]) & (cy < patch[3])


def draw_crop(ch, cw, boxes_px, policy, rng):
    """MinIoURandomCrop on a ch x cw canvas with pixel boxes [N,4] (N >= 1) -> (mode, patch): mode 1 = no
    crop (patch None); else the integer patch (x1, y1, x2, y2).  The mode is uniform over (1, *min_ious,
    0); up to CROP_TRIES tries per mode: width ~ U(min_crop * cw, cw), height likewise, rejected unless
    0.5 <= h / w <= 2 (for the drawn sizes and for the integer patch); a uniform offset; the integer
    patch rejected if empty, if the smallest IoU with any box is below the mode, or if no box centre lies
    strictly inside it; after CROP_TRIES failures the mode is drawn again.  (A mode that the boxes' areas
    rule out for every patch is drawn again at once: see `reach` below.)"""
    modes = (1.0,) + policy.min_ious + (0.0,)
    b = np.asarray(boxes_px, f32).reshape(-1, 4)
    # plain floats from here on (the fp32 corners and centres are exact in float64): the loop runs often
    centres = ((b[:, :2] + b[:, 2:]) / f32(2.0)).tolist()
    rects = [(x1, y1, x2, y2, (x2 - x1) * (y2 - y1)) for x1, y1, x2, y2 in b.astype(np.float64).tolist()]
    lo_w, lo_h = policy.min_crop * cw, policy.min_crop * ch
    # IoU <= smaller area / larger area, and no integer patch is smaller than (lo_w - 1) x (lo_h - 1): a mode
    # above `reach` fails all its tries whatever is drawn, so it is drawn again without spending them (the
    # same distribution of results; on a zoomed-out canvas this is most modes)
    least = max(lo_w - 1.0, 1.0) * max(lo_h - 1.0, 1.0)
    reach = min(r[4] / max(r[4], least) for r in rects) + 1e-9
    while True:
        mode = modes[int(rng.integers(len(modes)))]
        if mode == 1.0:
            return mode, None
        if mode > reach:
            continue
        for _ in range(CROP_TRIES):
            w, h = rng.uniform(lo_w, cw), rng.uniform(lo_h, ch)
            if h / w < 0.5 or h / w > 2.0:
                continue
            left, top = rng.uniform(0.0, cw - w), rng.uniform(0.0, ch - h)
            px1, py1, px2, py2 = patch = (int(left), int(top), int(left + w), int(top + h))
            pw_, ph_ = px2 - px1, py2 - py1
            if pw_ <= 0 or ph_ <= 0 or ph_ < 0.5 * pw_ or ph_ > 2.0 * pw_:
                continue
            if min(_iou(patch, pw_ * ph_, r) for r in rects) < mode:
                continue
            if not any(px1 < cx < px2 and py1 < cy < py2 for cx, cy in centres):
                continue
            return mode, patch


def _iou(patch, patch_area, rect):
    """IoU (float64) of the integer patch (x1, y1, x2, y2) with a box (x1, y1, x2, y2, area)."""
    iw = min(rect[2], patch[2]) - max(rect[0], patch[0])
    ih = min(rect[3], patch[3]) - max(rect[1], patch[1])
    inter = iw * ih if iw > 0.0 and ih > 0.0 else 0.0
    return inter / (rect[4] + patch_area - inter)


def crop_boxes(boxes_px, patch):
    """Pixel boxes [N,4] through the crop `patch` (x1, y1, x2, y2): those whose centre is not strictly
    inside are dropped, the rest clipped to the patch and translated to its origin -> (boxes, keep mask)."""
    b = np.asarray(boxes_px, f32).reshape(-1, 4)
    keep = centres_inside(patch, b)
    lo = np.array([patch[0], patch[1], patch[0], patch[1]], f32)
    hi = np.array([patch[2], patch[3], patch[2], patch[3]], f32)
    return (np.minimum(np.maximum(b[keep], lo), hi) - lo).astype(f32), keep


Plan = namedtuple("Plan", "H W ch cw oy ox y0 x0 hh ww flip oh ow ph pw m t fill new_shape boxes labels keep mode")
Plan.__doc__ = """One image's draws: the fields of cvl_augment_desc (canvas ch x cw with the source at (oy, ox),
crop (y0, x0, hh, ww), flip, resized oh x ow, padded ph x pw, colour m [3,3] / t [3], fill [3]) plus
new_shape (fp32 [2], the unpadded resized size = the trainer's img_dim), boxes [n,4] (yc, xc, h, w)
normalised to it, labels [n] int32, keep (the indices of the input boxes that survive) and the crop mode."""


def plan_geometry(H, W, canvas=None, crop=None, flip=False, m=None, t=None, fill=(0.0, 0.0, 0.0), size=None,
                  min_side=800.0, max_side=1333.0, stride=128.0, equal_dims=True, out_hw=None, pad_hw=None):
    """A Plan without boxes from explicit values (no draws): canvas = (ch, cw, oy, ox) or None, crop =
    (y0, x0, hh, ww) or None (the whole canvas).  The output size: size=S -> exactly (S, S) ("fixed");
    out_hw / pad_hw given -> those; else data_preprocess._plan's min / max side, stride and equal dims
    applied to the crop's size ("jitter", with the side already drawn: min_side)."""
    ch, cw, oy, ox = (H, W, 0, 0) if canvas is None else (int(v) for v in canvas)
    y0, x0, hh, ww = (0, 0, ch, cw) if crop is None else (int(v) for v in crop)
    if size is not None:
        oh = ow = ph = pw = int(size)
        new_shape = np.array([size, size], f32)
    elif out_hw is not None:
        oh, ow = (int(v) for v in out_hw)
        ph, pw = (oh, ow) if pad_hw is None else (int(v) for v in pad_hw)
        new_shape = np.array([oh, ow], f32)
    else:
        new_shape, _, ph, pw = _plan(hh, ww, None, min_side, max_side, stride, equal_dims, None)
        oh, ow = int(new_shape[0]), int(new_shape[1])
    m = np.eye(3, dtype=f32) if m is None else np.asarray(m, f32).reshape(3, 3)
    t = np.zeros(3, f32) if t is None else np.asarray(t, f32).reshape(3)
    return Plan(int(H), int(W), ch, cw, oy, ox, y0, x0, hh, ww, bool(flip), oh, ow, ph, pw, m, t,
                np.asarray(fill, f32).reshape(3), new_shape, np.zeros((0, 4), f32), np.zeros(0, np.int32),
                np.zeros(0, np.int64), 1.0)


def plan_image(hw, boxes_xyxy_norm, labels, policy, rng, jitter=None, min_side=800.0, max_side=1333.0, stride=128.0,
               equal_dims=True, size=None):
    """The draws of one image (host only, numpy, fp32 box arithmetic) -> Plan.  hw = (H, W) of the source;
    boxes_xyxy_norm [N,4] the sample's normalised (x1, y1, x2, y2) (the reference's `objects.bbox`);
    labels [N].  Draw order: flip, resize jitter, photometric parameters, zoom-out, crop (module
    docstring).  An image without boxes is never cropped and makes no crop draws.
    Boxes: translated by the zoom-out, dropped (with their labels) when their centre falls outside the
    crop, clipped to the crop and translated, then mirrored and expressed as (yc, xc, h, w) normalised to
    the unpadded resized size by data_preprocess.box_targets; with neither zoom-out nor crop the
    normalised input goes to box_targets untouched, so the identity policy gives its boxes bit for bit.
    Output size: size=None ("jitter") -> _plan's min / max side, stride and equal dims applied to the
    crop's size, the side drawn from `jitter` = (low, high) when given; size=S ("fixed") -> (S, S)."""
    H, W = int(hw[0]), int(hw[1])
    b = np.asarray(boxes_xyxy_norm, f32).reshape(-1, 4)
    lab = np.asarray(labels, np.int32).reshape(-1)
    flip = bool(rng.uniform() <= policy.flip) if policy.flip > 0.0 else False
    if size is None and jitter is not None:
        min_side = f32(rng.uniform(jitter[0], jitter[1]))
    kw = _draw_colour(policy, rng)
    m, t = colour_affine(**kw) if kw else (_EYE, _ZERO3)
    canvas = None
    if policy.expand is not None and policy.expand_prob > 0.0 and rng.uniform() < policy.expand_prob:
        ratio = rng.uniform(*policy.expand)
        ch, cw = int(H * ratio), int(W * ratio)
        ox, oy = int(rng.uniform(0.0, cw - W)), int(rng.uniform(0.0, ch - H))
        canvas = (ch, cw, oy, ox)
    ch, cw, oy, ox = (H, W, 0, 0) if canvas is None else canvas
    mode, patch = 1.0, None
    keep = np.arange(len(b))
    crops = policy.min_ious is not None and len(b) > 0
    if canvas is not None or crops:
        px = b * np.array([W, H, W, H], f32) + np.array([ox, oy, ox, oy], f32)
    if crops:
        mode, patch = draw_crop(ch, cw, px, policy, rng)
    if canvas is not None or patch is not None:
        patch = (0, 0, cw, ch) if patch is None else patch
        px, mask = crop_boxes(px, patch)
        keep = np.nonzero(mask)[0]
        ww, hh = patch[2] - patch[0], patch[3] - patch[1]
        b = (px / np.array([ww, hh, ww, hh], f32)).astype(f32)
        crop = (patch[1], patch[0], hh, ww)
    else:
        crop = None
    g = plan_geometry(H, W, canvas, crop, flip, m, t, policy.fill, size=size, min_side=min_side, max_side=max_side,
                      stride=stride, equal_dims=equal_dims)
    return g._replace(boxes=box_targets(b, flip), labels=lab[keep], keep=keep, mode=mode)


# -------------------------------------------------------------------------------------------------
# device
# -------------------------------------------------------------------------------------------------
def _device_image(image):
    if isinstance(image, np.ndarray) and not image.flags.writeable:      # PIL's decoded array
        image = image.copy()
    img = torch.as_tensor(image)
    if img.dtype not in (torch.uint8, torch.float32):
        img = img.float()
    img = img.cuda().contiguous()
    if img.dim() != 3 or int(img.shape[2]) != 3:
        raise ValueError("augment takes [H, W, 3] images, not %r" % (tuple(img.shape),))
    return img


def plan_table(plans):
    """The plans as a host uint8 [B, 144] tensor of cvl_augment_desc with the pointers left 0: the `table`
    argument of torch.ops.cvlite.augment_images."""
    table = np.zeros(len(plans), DESC)
    ints = np.array([p[:len(_INT_FIELDS)] for p in plans], np.int32)      # a column per field: few numpy calls
    for j, name in enumerate(_INT_FIELDS):
        table[name] = ints[:, j]
    table["m"] = np.stack([p.m for p in plans]).reshape(-1, 9)
    table["t"] = np.stack([p.t for p in plans])
    table["fill"] = np.stack([p.fill for p in plans])
    return torch.from_numpy(table.view(np.uint8).reshape(len(plans), DESC.itemsize))


def bind_table(table, images, outs):
    """Writes the source and destination of each image into the DESC array `table` (its sizes checked)."""
    src_hw, pad_hw = table[["H", "W"]].tolist(), table[["ph", "pw"]].tolist()
    for k, (img, o) in enumerate(zip(images, outs)):
        if tuple(img.shape[:2]) != src_hw[k]:
            raise ValueError("image %d is %dx%d, its plan was made for %dx%d" % ((k,) + tuple(img.shape[:2]) + src_hw[k]))
        if tuple(o.shape) != pad_hw[k] + (3,) or o.dtype != torch.float32 or not o.is_contiguous():
            raise ValueError("slot %d must be a contiguous fp32 [%d, %d, 3]" % ((k,) + pad_hw[k]))
    table["src"] = [img.data_ptr() for img in images]
    table["dst"] = [o.data_ptr() for o in outs]
    table["src_u8"] = [1 if img.dtype == torch.uint8 else 0 for img in images]


def pinned_table(table, images, outs):
    """A pinned copy of the host table [B, 144] with the images' and slots' pointers written in."""
    B = int(table.shape[0])
    if tuple(table.shape) != (B, DESC.itemsize) or table.dtype != torch.uint8 or table.is_cuda:
        raise ValueError("the table is a host uint8 [B, %d] tensor (plan_table)" % DESC.itemsize)
    if len(images) != B or len(outs) != B:
        raise ValueError("augment: %d images and %d slots for %d descriptors" % (len(images), len(outs), B))
    host = torch.empty((B, DESC.itemsize), dtype=torch.uint8, pin_memory=True)
    host.copy_(table)
    bind_table(host.numpy().view(DESC).reshape(B), images, outs)
    return host


def launch_table(host):
    """host: a pinned uint8 [B, 144] tensor of descriptors (pinned_table).  One asynchronous copy to the
    device and one cvl_augment_batch launch, both on the current stream."""
    device = host.to("cuda", non_blocking=True)
    _lib.call("cvl_augment_batch", _lib.c_void_p(host.data_ptr()), _lib.ptr(device), int(host.shape[0]), _lib.stream())


def run_plans(images, plans, out=None):
    """images: device uint8 / fp32 [H_i, W_i, 3] tensors (host arrays are uploaded); plans: their Plans.
    One table copy and one launch.  out: None (a fresh [ph_i, pw_i, 3] fp32 tensor per image, or views of
    ONE stacked [B, ph, pw, 3] tensor when every plan has the same padded size), a [B, ph, pw, 3] tensor,
    or a list of preallocated slots.  Returns (list of slots, the stacked tensor or None)."""
    B = len(plans)
    if not 1 <= B <= MAX_BATCH or len(images) != B:
        raise ValueError("augment takes 1..%d images with one plan each" % MAX_BATCH)
    _lib.require_cuda()
    imgs = [_device_image(im) for im in images]
    stacked = None
    if out is None:
        if len({(p.ph, p.pw) for p in plans}) == 1:
            stacked = torch.empty((B, plans[0].ph, plans[0].pw, 3), dtype=torch.float32, device=imgs[0].device)
            out = list(stacked.unbind(0))
        else:
            out = [torch.empty((p.ph, p.pw, 3), dtype=torch.float32, device=imgs[0].device) for p in plans]
    elif isinstance(out, torch.Tensor):
        stacked, out = out, list(out.unbind(0))
    _lib.require_cuda(*out)
    if len(out) != B:
        raise ValueError("augment: %d slots for %d images" % (len(out), B))
    launch_table(pinned_table(plan_table(plans), imgs, out))
    return out, stacked


def _per_image(v, B, pair=False):
    if v is not None and np.ndim(v) == (2 if pair else 1):
        if len(v) != B:
            raise ValueError("a per-image setting needs one entry per image")
        return list(v)
    return [v] * B


def augment_batch(images, boxes, labels, policy, rng, jitter=None, min_side=800.0, max_side=1333.0, stride=128.0,
                  equal_dims=True, size=None, n_max=16, out=None):
    """images: a list of device uint8 / fp32 [H_i, W_i, 3] tensors (cvlite.jpeg.decode_batch's output);
    boxes: per image [N_i, 4] normalised (x1, y1, x2, y2); labels: per image [N_i].  Plans every image
    (plan_image, in order, all draws from `rng`), then ONE table copy and ONE launch.  jitter / min_side /
    max_side: one setting or one per image.  size=None ("jitter" mode) -> a list of [S_i, S_i, 3] device
    images for JitterFCOSTrainer.step (written into the slots `out` when given); size=S ("fixed" mode) ->
    the stacked [B, S, S, 3] tensor (`out`: that tensor, or views of one).
    Returns (images, boxes [B, max(n_max, most boxes), 5] (yc, xc, h, w, cls) fp32, nbox [B] int32, img_dim
    [B, 2] fp32), the arrays on the host as train_fcos._raw_batch returns them."""
    if not isinstance(policy, AugmentPolicy):
        raise ValueError("policy must be an AugmentPolicy, not %r" % (policy,))
    B = len(images)
    jit, lo, hi = _per_image(jitter, B, pair=True), _per_image(min_side, B), _per_image(max_side, B)
    plans = [plan_image(images[k].shape[:2], boxes[k], labels[k], policy, rng, jitter=jit[k], min_side=lo[k],
                        max_side=hi[k], stride=stride, equal_dims=equal_dims, size=size) for k in range(B)]
    slots, stacked = run_plans(images, plans, out=out)
    n_max = max(int(n_max), max(len(p.boxes) for p in plans))
    bx = np.zeros((B, n_max, 5), f32)
    nb = np.zeros(B, np.int32)
    for k, p in enumerate(plans):
        bx[k, :len(p.boxes), :4] = p.boxes
        bx[k, :len(p.boxes), 4] = p.labels.astype(f32)
        nb[k] = len(p.boxes)
    dims = np.stack([p.new_shape for p in plans]).astype(f32)
    return (stacked if size is not None and stacked is not None else slots), bx, nb, dims
