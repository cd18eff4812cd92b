"""Test infrastructure: the reference dataset's seven random augmentations (unet-lite/yolo5-seg/seg_diceloss_yolov5.py:75-185,
320-325) restated in numpy, byte for byte what Pillow 12 computes for 8-bit RGB images and 8-bit label maps, plus the draw of the
per-sample plan.  Independent of yolo_dual_amd: the GPU stage (csrc/augment.hip) and ``draw_augmentations`` are tested against
this file, this file against fixtures Pillow wrote (tests/golden/aug_*.npz) and, where Pillow imports, against Pillow itself.

Images are uint8 ``[H][W][3]``, label maps uint8 ``[H][W]``; every op keeps the size.  Which arithmetic Pillow uses where:
  mirror / flip       index reversal
  rotate              Image.rotate builds the inverse affine matrix in double (entries rounded to 15 decimals); BILINEAR goes through
                      Geometry.c affine_transform + bilinear_filter (double, truncating store), NEAREST through affine_fixed (16.16)
  brightness/contrast Image.blend with a float alpha outside [0, 1] or inside it: single precision, clamp, truncate
  Gaussian blur       BoxBlur.c: three box passes per axis, 24-bit fixed-point weights, 32-bit unsigned accumulators
  crop                crop, then Image.resize back: Resample.c (22-bit coefficients, 8-bit intermediate) / ImagingScaleAffine"""
import math
import random

import numpy as np

OPS = ("fliplr", "flipud", "rotation", "brightness", "contrast", "blur", "crop")       # order of get_augmentations (:175-185)
f32 = np.float32


# ---- the plan -------------------------------------------------------------------------------------------------------------
def draw_plan(hyp, w, h, rng=random):
    """[(op, params)] of one sample, drawing from ``rng`` what _apply_augmentations and the classes' __call__ draw, in their order"""
    hyp = hyp or {}
    p = {"fliplr": hyp.get("fliplr", 0.5), "flipud": hyp.get("flipud", 0.2), "rotation": 0.3, "brightness": 0.3, "contrast": 0.3,
         "blur": 0.1, "crop": 0.3}
    deg = hyp.get("degrees", 15)
    plan = []
    for op in rng.sample(list(OPS), k=len(OPS)):
        if not rng.random() < p[op]:
            continue
        if op in ("fliplr", "flipud"):
            plan.append((op, ()))
        elif op == "rotation":
            plan.append((op, (rng.uniform(-deg, deg),)))
        elif op in ("brightness", "contrast"):
            plan.append((op, (rng.uniform(0.7, 1.3),)))
        elif op == "blur":
            plan.append((op, (rng.uniform(0.5, 2.0),)))
        else:
            scale = rng.uniform(0.7, 1.0)
            nw, nh = max(1, int(w * scale)), max(1, int(h * scale))
            x1 = rng.randint(0, w - nw)
            y1 = rng.randint(0, h - nh)
            plan.append((op, (x1, y1, nw, nh)))
    return plan


# ---- flips ----------------------------------------------------------------------------------------------------------------
def fliplr(a):
    return np.ascontiguousarray(a[:, ::-1])


def flipud(a):
    return np.ascontiguousarray(a[::-1])


# ---- rotation -------------------------------------------------------------------------------------------------------------
def rotate_matrix(w, h, angle):
    """Image.rotate's inverse matrix (a0..a5), translation folded in; ``angle`` already reduced modulo 360"""
    cx, cy = w / 2, h / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def _check_rotate(angle):
    angle = angle % 360.0
    if angle in (90.0, 180.0, 270.0):             # (360.0, which a tiny negative angle reduces to, is an identity matrix: generic path)
        raise ValueError("multiples of 90 degrees take Pillow's transpose paths, which are not restated")
    return angle


def rotate_image(img, angle):
    angle = _check_rotate(angle)
    if angle == 0:
        return img.copy()
    h, w, _ = img.shape
    A = rotate_matrix(w, h, angle)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    xin = A[0] * (xs + 0.5) + A[1] * (ys + 0.5) + A[2]
    yin = A[3] * (xs + 0.5) + A[4] * (ys + 0.5) + A[5]
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    xi, yi = xin - 0.5, yin - 0.5
    x, y = np.floor(xi).astype(np.int64), np.floor(yi).astype(np.int64)
    dx, dy = (xi - x)[..., None], (yi - y)[..., None]
    src = img.astype(np.float64)
    x0, x1, y0 = np.clip(x, 0, w - 1), np.clip(x + 1, 0, w - 1), np.clip(y, 0, h - 1)
    v1 = src[y0, x0] + (src[y0, x1] - src[y0, x0]) * dx
    y1ok = (y + 1 >= 0) & (y + 1 < h)
    y1 = np.clip(y + 1, 0, h - 1)
    v2 = src[y1, x0] + (src[y1, x1] - src[y1, x0]) * dx
    v2 = np.where(y1ok[..., None], v2, v1)
    out = (v1 + (v2 - v1) * dy).astype(np.uint8)                    # (UINT8)v1: truncation, the value is within [0, 255]
    out[~ok] = 0
    return out


def rotate_fixed(w, h, angle):
    """the six 16.16 integers of Geometry.c affine_fixed"""
    A = rotate_matrix(w, h, angle)
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return [fix(A[0]), fix(A[1]), fix(A[2] + A[0] * 0.5 + A[1] * 0.5), fix(A[3]), fix(A[4]), fix(A[5] + A[3] * 0.5 + A[4] * 0.5)]


def rotate_mask(mask, angle):
    angle = _check_rotate(angle)
    if angle == 0:
        return mask.copy()
    h, w = mask.shape
    a0, a1, a2, a3, a4, a5 = rotate_fixed(w, h, angle)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    xin = (a2 + a1 * ys + a0 * xs) >> 16
    yin = (a5 + a4 * ys + a3 * xs) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = np.zeros_like(mask)
    out[ok] = mask[yin[ok], xin[ok]]
    return out


# ---- brightness / contrast (ImageEnhance -> Image.blend) ------------------------------------------------------------------------
def _blend(deg, img, factor):
    d = deg.astype(f32)
    v = d + f32(factor) * (img.astype(f32) - d)
    return np.where(v <= 0, 0, np.where(v >= 255, 255, v)).astype(np.uint8)


def brightness(img, factor):
    return _blend(np.zeros((), np.uint8), img, factor)


def luminance(img):
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


def contrast_mean(img):
    lum = luminance(img)
    return int(float(int(lum.sum(dtype=np.int64))) / lum.size + 0.5)


def contrast(img, factor):
    return _blend(np.array(contrast_mean(img), np.uint8), img, factor)


# ---- Gaussian blur ------------------------------------------------------------------------------------------------------------
def box_radius(radius, passes=3):
    """BoxBlur.c _gaussian_blur_radius: float variables, double intermediates"""
    radius = f32(radius)
    sigma2 = f32(float(radius) * float(radius) / passes)
    L = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32((2 * float(l) + 1) * (float(l) * (float(l) + 1) - 3 * float(sigma2)))
    a = f32(float(a) / (6 * (float(sigma2) - (float(l) + 1) * (float(l) + 1))))
    return f32(float(l) + float(a))


def box_weights(fr):
    """(R, ww, fw) of one box pass of float radius ``fr``"""
    fr = f32(fr)
    r = int(fr)
    ww = int(np.uint32(f32(1 << 24) / f32(fr * f32(2) + f32(1))))
    fw = ((1 << 24) - (r * 2 + 1) * ww) // 2
    return r, ww, fw


def box_pass(img, r, ww, fw):
    """one horizontal pass (axis 1) over [H][W][C] bytes"""
    W = img.shape[1]
    x = np.arange(W)
    src = img.astype(np.uint64)
    acc = np.zeros(img.shape, dtype=np.uint64)
    for k in range(-r, r + 1):
        acc += src[:, np.clip(x + k, 0, W - 1)]
    far = src[:, np.clip(x - r - 1, 0, W - 1)] + src[:, np.clip(x + r + 1, 0, W - 1)]
    bulk = (acc * np.uint64(ww) + far * np.uint64(fw)) & np.uint64(0xFFFFFFFF)
    return (((bulk + np.uint64(1 << 23)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)).astype(np.uint8)


def gaussian_blur(img, radius):
    r, ww, fw = box_weights(box_radius(radius))
    o = img
    for _ in range(3):
        o = box_pass(o, r, ww, fw)
    o = o.transpose(1, 0, 2)
    for _ in range(3):
        o = box_pass(o, r, ww, fw)
    return np.ascontiguousarray(o.transpose(1, 0, 2))


# ---- crop + resize back -------------------------------------------------------------------------------------------------------
_PRECISION_BITS = 32 - 8 - 2


def bilinear_coeffs(in_size, out_size):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc, triangle filter: per output sample (first tap, integer weights)"""
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 1.0 * fscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ws, ww = [], 0.0
        for x in range(xmax):
            arg = abs((x + xmin - center + 0.5) * (1.0 / fscale))
            w = 1.0 - arg if arg < 1.0 else 0.0
            ws.append(w)
            ww += w
        if ww != 0.0:
            ws = [w / ww for w in ws]
        out.append((xmin, [int(math.trunc(0.5 + w * (1 << _PRECISION_BITS))) if w >= 0 else int(math.trunc(-0.5 + w * (1 << _PRECISION_BITS)))
                           for w in ws]))
    return out


def _resample_axis1(img, out_size):
    in_size = img.shape[1]
    out = np.empty((img.shape[0], out_size, img.shape[2]), np.uint8)
    for xx, (xmin, ks) in enumerate(bilinear_coeffs(in_size, out_size)):
        ss = np.full((img.shape[0], img.shape[2]), 1 << (_PRECISION_BITS - 1), np.int64)
        for t, k in enumerate(ks):
            ss += img[:, xmin + t].astype(np.int64) * k
        out[:, xx] = np.clip(ss >> _PRECISION_BITS, 0, 255)
    return out


def resize_bilinear(img, w, h):
    """Image.resize((w, h), BILINEAR) of an RGB image: horizontal pass, 8-bit intermediate, vertical pass; a pass whose size
    does not change is skipped"""
    o = img
    if o.shape[1] != w:
        o = _resample_axis1(o, w)
    if o.shape[0] != h:
        o = _resample_axis1(o.transpose(1, 0, 2), h).transpose(1, 0, 2)
    return np.ascontiguousarray(o)


def nearest_index(in_size, out_size):
    """Geometry.c ImagingScaleAffine: xo = a/2, then += a per output sample, truncated"""
    a = in_size / out_size
    xo, idx = a * 0.5, []
    for _ in range(out_size):
        idx.append(min(max(int(xo), 0), in_size - 1))
        xo += a
    return np.array(idx, np.int64)


def resize_nearest(mask, w, h):
    if mask.shape == (h, w):
        return mask.copy()
    return np.ascontiguousarray(mask[nearest_index(mask.shape[0], h)][:, nearest_index(mask.shape[1], w)])


def crop_image(img, x1, y1, nw, nh):
    h, w, _ = img.shape
    return resize_bilinear(img[y1:y1 + nh, x1:x1 + nw], w, h)


def crop_mask(mask, x1, y1, nw, nh):
    h, w = mask.shape
    return resize_nearest(mask[y1:y1 + nh, x1:x1 + nw], w, h)


# ---- a whole plan ---------------------------------------------------------------------------------------------------------------
def apply_op(img, mask, op, params):
    if op == "fliplr":
        return fliplr(img), fliplr(mask)
    if op == "flipud":
        return flipud(img), flipud(mask)
    if op == "rotation":
        return rotate_image(img, params[0]), rotate_mask(mask, params[0])
    if op == "brightness":
        return brightness(img, params[0]), mask
    if op == "contrast":
        return contrast(img, params[0]), mask
    if op == "blur":
        return gaussian_blur(img, params[0]), mask
    if op == "crop":
        return crop_image(img, *params), crop_mask(mask, *params)
    raise ValueError(f"unknown augmentation {op!r}")


def apply_plan(img, mask, plan):
    for op, params in plan:
        img, mask = apply_op(img, mask, op, params)
    return img, mask


def letterbox(img, mask, size, num_classes=12, fill=128):
    """_resize_and_pad (:327-349) + the format conversion of __getitem__ (:315-316): float32 [3][S][S] and int64 [S][S]"""
    h, w, _ = img.shape
    scale = min(size / w, size / h)
    nw, nh = int(w * scale), int(h * scale)
    pl, pt = (size - nw) // 2, (size - nh) // 2
    ci = np.full((size, size, 3), fill, np.uint8)
    cm = np.zeros((size, size), np.uint8)
    ci[pt:pt + nh, pl:pl + nw] = resize_bilinear(img, nw, nh)
    cm[pt:pt + nh, pl:pl + nw] = resize_nearest(mask, nw, nh)
    return ci.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0), np.clip(cm, 0, num_classes - 1).astype(np.int64)
