"""GPU half of the reference's per-sample input preparation.

Mirrors what ``JSONSegmentDataset.__getitem__`` does to a decoded sample (unet-lite/yolo5-seg/seg_diceloss_yolov5.py:72-185,
291-349; Resnet18/seg_diceloss_resnet18.py:84-149): the seven random augmentations (``AugmentGPU``: mirror, flip, rotation,
brightness, contrast, Gaussian blur, crop + resize back), then ``_resize_and_pad`` and the format conversion (``LetterboxGPU``:
aspect-preserving ``Image.resize(BILINEAR)`` of the image / ``Image.resize(NEAREST)`` of the label map, paste on a 128-grey / 0
canvas of ``img_size``, ``/255`` and HWC→CHW float32, labels as int64).  Decoding files and JSON parsing stay on the host (out of
scope), and so does the *draw* of a sample's augmentations (``draw_augmentations``: a few calls of ``random``, plain data out); what
is here starts from the decoded uint8 arrays and is bit-exact with Pillow (12.2.0 checked): the tables, matrices and weights Pillow
derives once per call are built here in double (or float) precision the way Pillow builds them, the HIP kernels do the per-pixel
arithmetic (``csrc/input.hip``, ``csrc/augment.hip``).  No CPU fallback: tensors are moved to the GPU, the kernels run there."""
from __future__ import annotations

import collections
import functools
import math
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .tape import _p, _stream

_PRECISION_BITS = 32 - 8 - 2          # Pillow Resample.c: PRECISION_BITS for 8 bits per channel


@functools.lru_cache(maxsize=4096)
def _bilinear_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc for the triangle ("bilinear") filter over the whole input range,
    all output samples at once; the tap weights of one sample are summed tap by tap (Pillow's order) before normalising."""
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = fscale                                   # filter support 1.0, stretched when down-scaling
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    cnt = xmax - xmin
    taps = np.arange(ksize, dtype=np.int64)[None, :]
    arg = np.abs((taps + xmin[:, None] - center[:, None] + 0.5) * (1.0 / fscale))
    w = np.where((arg < 1.0) & (taps < cnt[:, None]), 1.0 - arg, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for t in range(ksize):                             # sequential accumulation, like `ww += w` in the C loop
        ww = ww + w[:, t]
    k = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    coef = np.trunc(0.5 + k * float(1 << _PRECISION_BITS)).astype(np.int32)
    coef[taps.repeat(out_size, 0) >= cnt[:, None]] = 0
    bounds = np.stack([xmin, cnt], axis=1).astype(np.int32)
    if int((bounds[:, 0] + bounds[:, 1]).max()) > in_size:
        raise AssertionError("resample taps outside the source")
    return np.ascontiguousarray(bounds), np.ascontiguousarray(coef), ksize


@functools.lru_cache(maxsize=4096)
def _nearest_table(in_size: int, out_size: int) -> np.ndarray:
    """Geometry.c ImagingScaleAffine: xo = a/2, then `xo += a` per output sample — np.cumsum adds sequentially in double too"""
    a = in_size / out_size
    steps = np.full(out_size, a, dtype=np.float64)
    steps[0] = a * 0.5
    xo = np.cumsum(steps)
    return np.clip(np.trunc(xo).astype(np.int64), 0, in_size - 1).astype(np.int32)


def letterbox_geometry(w: int, h: int, img_size: int) -> Tuple[int, int, int, int]:
    """``(new_w, new_h, pad_left, pad_top)`` of _resize_and_pad (:327-339)"""
    scale = min(img_size / w, img_size / h)
    new_w, new_h = int(w * scale), int(h * scale)
    if new_w < 1 or new_h < 1:
        raise ValueError(f"image {w}x{h} collapses to {new_w}x{new_h} at img_size {img_size}")
    return new_w, new_h, (img_size - new_w) // 2, (img_size - new_h) // 2


def _as_u8(a, ndim: int) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    if t.dtype != torch.uint8 or t.dim() != ndim:
        raise TypeError(f"expected a uint8 array with {ndim} dimensions, got {t.dtype} {tuple(t.shape)}")
    return t


class _DeviceTables:
    """Device copies of the resampling tables, keyed (kind, n_in, n_out): "bil" -> (bounds, coef, ksize), "near" -> index table.
    Least-recently-used entries are dropped ONE at a time once ``capacity`` is reached.  The cache is not the owner a launch may
    rely on: a caller keeps the returned tensors in local variables until its kernel is enqueued (the raw pointer handed to the C
    side owns nothing); freeing after that is safe, the allocator reuses a block in stream order."""

    def __init__(self, device, capacity: int):
        self.device, self.capacity = device, int(capacity)
        self._d = collections.OrderedDict()

    def get(self, kind: str, n_in: int, n_out: int):
        key = (kind, n_in, n_out)
        t = self._d.get(key)
        if t is not None:
            self._d.move_to_end(key)
            return t
        if kind == "bil":
            b, k, ks = _bilinear_tables(n_in, n_out)
            t = (torch.from_numpy(b).to(self.device), torch.from_numpy(k).to(self.device), ks)
        else:
            t = torch.from_numpy(_nearest_table(n_in, n_out)).to(self.device)
        while len(self._d) >= self.capacity:
            self._d.popitem(last=False)
        self._d[key] = t
        return t

    def __len__(self):
        return len(self._d)


class LetterboxGPU:
    """``lb = LetterboxGPU(640, num_classes=12); img, mask = lb(img_u8_hwc, mask_u8_hw)`` — the arrays a
    ``JSONSegmentDataset.__getitem__`` holds after decoding (and augmenting) go in, what it returns comes out, on the GPU."""

    def __init__(self, img_size: int = 640, num_classes: int = 12, device=None, fill: int = 128):
        if not torch.cuda.is_available():
            raise RuntimeError("LetterboxGPU runs on the GPU only (yolo_dual_amd has no CPU fallback)")
        self.img_size = int(img_size)
        self.num_classes = int(num_classes)
        self.fill = int(fill)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._tables = _DeviceTables(self.device, 512)

    def _tab(self, kind: str, n_in: int, n_out: int):
        return self._tables.get(kind, n_in, n_out)

    _u8 = staticmethod(_as_u8)

    def __call__(self, img, mask=None, out_img: Optional[torch.Tensor] = None, out_mask: Optional[torch.Tensor] = None):
        S = self.img_size
        img = self._u8(img, 3)
        if img.shape[2] != 3:
            raise ValueError("image must be [H][W][3] RGB")
        h, w = int(img.shape[0]), int(img.shape[1])
        new_w, new_h, pl, pt = letterbox_geometry(w, h, S)
        img = img.to(self.device, non_blocking=True).contiguous()
        st = _stream()
        if out_img is None:
            out_img = torch.empty((3, S, S), dtype=torch.float32, device=self.device)
        elif tuple(out_img.shape) != (3, S, S) or out_img.dtype != torch.float32 or not out_img.is_contiguous():
            raise ValueError("out_img must be a contiguous float32 [3][S][S] tensor")
        xb = xk = yb = yk = None
        xks = yks = 0
        tmp = None
        if new_w != w:
            xb, xk, xks = self._tab("bil", w, new_w)
            tmp = torch.empty((h, new_w, 3), dtype=torch.uint8, device=self.device)
        if new_h != h:
            yb, yk, yks = self._tab("bil", h, new_h)
        L.call("ydl_letterbox_image", _p(img), h, w, _p(tmp) if tmp is not None else None, _p(out_img), S, new_w, new_h, pl, pt,
               _p(xb) if xb is not None else None, _p(xk) if xk is not None else None, xks,
               _p(yb) if yb is not None else None, _p(yk) if yk is not None else None, yks, self.fill, st)
        if mask is None:
            return out_img, None
        mask = self._u8(mask, 2)
        if (int(mask.shape[0]), int(mask.shape[1])) != (h, w):
            raise ValueError("mask and image sizes differ")
        mask = mask.to(self.device, non_blocking=True).contiguous()
        if out_mask is None:
            out_mask = torch.empty((S, S), dtype=torch.int64, device=self.device)
        elif tuple(out_mask.shape) != (S, S) or out_mask.dtype != torch.int64 or not out_mask.is_contiguous():
            raise ValueError("out_mask must be a contiguous int64 [S][S] tensor")
        xt, yt = self._tab("near", w, new_w), self._tab("near", h, new_h)      # held here until the launch is enqueued
        L.call("ydl_letterbox_mask", _p(mask), h, w, _p(out_mask), S, new_w, new_h, pl, pt, _p(xt), _p(yt), self.num_classes - 1, st)
        return out_img, out_mask

    def batch(self, imgs: Sequence, masks: Optional[Sequence] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """what the DataLoader's default collate makes of the per-sample tensors: (N,3,S,S) float32 and (N,S,S) int64"""
        n, S = len(imgs), self.img_size
        out_i = torch.empty((n, 3, S, S), dtype=torch.float32, device=self.device)
        out_m = torch.empty((n, S, S), dtype=torch.int64, device=self.device) if masks is not None else None
        for i in range(n):
            self(imgs[i], masks[i] if masks is not None else None, out_i[i], out_m[i] if out_m is not None else None)
        return out_i, out_m


# ---- the random augmentations ---------------------------------------------------------------------------------------------
AUG_OPS = ("fliplr", "flipud", "rotation", "brightness", "contrast", "blur", "crop")        # order of get_augmentations (:175-185)


def draw_augmentations(hyp, w: int, h: int, rng=random) -> List[Tuple[str, tuple]]:
    """The plan of one sample: ``[(op, params), ...]`` in the order the ops are applied.  Draws from ``rng`` exactly what
    ``_apply_augmentations`` (:320-325) and the augmentation classes draw, so that a seeded ``random`` gives the sample the reference
    would have made: ``random.sample`` of the seven ops, then per op ``random.random() < p`` and, only when it fires, its own draws.
    Parameters: rotation ``(angle,)``, brightness / contrast ``(factor,)``, blur ``(radius,)``, crop ``(x1, y1, new_w, new_h)``.
    ``w``, ``h``: the sample's size (the crop box is drawn against it).  ``hyp=None`` means the defaults of ``get_augmentations`` (fliplr 0.5, flipud 0.2, degrees 15)."""
    hyp = hyp or {}
    p = {"fliplr": hyp.get("fliplr", 0.5), "flipud": hyp.get("flipud", 0.2), "rotation": 0.3, "brightness": 0.3, "contrast": 0.3,
         "blur": 0.1, "crop": 0.3}
    degrees = hyp.get("degrees", 15)
    plan: List[Tuple[str, tuple]] = []
    for op in rng.sample(list(AUG_OPS), k=len(AUG_OPS)):
        if not rng.random() < p[op]:
            continue
        if op == "rotation":
            plan.append((op, (rng.uniform(-degrees, degrees),)))
        elif op in ("brightness", "contrast"):
            plan.append((op, (rng.uniform(0.7, 1.3),)))
        elif op == "blur":
            plan.append((op, (rng.uniform(0.5, 2.0),)))
        elif op == "crop":
            scale = rng.uniform(0.7, 1.0)
            new_w, new_h = max(1, int(w * scale)), max(1, int(h * scale))
            x1 = rng.randint(0, w - new_w)
            y1 = rng.randint(0, h - new_h)
            plan.append((op, (x1, y1, new_w, new_h)))
        else:
            plan.append((op, ()))
    return plan


def _rotate_matrix(w: int, h: int, angle: float) -> List[float]:
    """Image.rotate's inverse affine matrix for ``angle`` (already reduced modulo 360), centre (w/2, h/2), translation folded in"""
    cx, cy = w / 2, h / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def _rotate_fixed(m: Sequence[float]) -> List[int]:
    """Geometry.c affine_fixed: the matrix in 16.16 fixed point, half a pixel folded into the translation"""
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def _box_weights(radius: float, passes: int = 3) -> Tuple[int, int, int]:
    """BoxBlur.c: Gaussian radius -> float box radius (_gaussian_blur_radius: float variables, double intermediates), then the
    weights of one box pass: (R, ww, fw) with ww = uint32(2^24 / (2 fr + 1)), that division in single precision"""
    f32 = np.float32
    r = f32(radius)
    sigma2 = f32(float(r) * float(r) / passes)
    big_l = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(big_l) - 1.0) / 2.0))
    a = f32((2 * float(l) + 1) * (float(l) * (float(l) + 1) - 3 * float(sigma2)))
    a = f32(float(a) / (6 * (float(sigma2) - (float(l) + 1) * (float(l) + 1))))
    fr = f32(float(l) + float(a))
    R = int(fr)
    ww = int(np.uint32(f32(1 << 24) / f32(fr * f32(2) + f32(1))))
    return R, ww, ((1 << 24) - (R * 2 + 1) * ww) // 2


class AugmentGPU:
    """``aug = AugmentGPU(hyp); plan = aug.plan(w, h); img_u8, mask_u8 = aug(img_u8_hwc, mask_u8_hw, plan)`` — the reference
    dataset's ``_apply_augmentations`` on the GPU, byte for byte what Pillow gives for the same plan; ``lb(*aug(img, mask, plan))``
    with a ``LetterboxGPU`` is the whole ``__getitem__`` after decoding.  The plan is plain data (``draw_augmentations``); nothing
    is drawn on the device.  Every op is a launch on the current stream, ping-ponging between two scratch buffers the stage owns:
    the returned tensors are views of that scratch and hold until the next call (an op-free plan returns the inputs, on the device)."""

    def __init__(self, hyp=None, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("AugmentGPU runs on the GPU only (yolo_dual_amd has no CPU fallback)")
        self.hyp = dict(hyp) if hyp else {}
        if not 0 <= float(self.hyp.get("degrees", 15)) < 90:
            raise ValueError("degrees must be in [0, 90): Pillow rotates multiples of 90 degrees along another code path")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        # crop tables: one key per (kind, box side, image side) ever drawn, about 1000 at 960x720 (scale 0.7..1.0, four kinds)
        self._tables = _DeviceTables(self.device, 4096)
        self._img = [torch.empty(0, dtype=torch.uint8, device=self.device) for _ in range(3)]      # ping, pong, crop scratch
        self._mask = [torch.empty(0, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self._sum = torch.zeros(2, dtype=torch.int64, device=self.device)          # contrast: luminance sum, then the mean d

    def plan(self, w: int, h: int, rng=random) -> List[Tuple[str, tuple]]:
        return draw_augmentations(self.hyp, w, h, rng)

    def _scratch(self, bufs, i: int, n: int) -> torch.Tensor:
        if bufs[i].numel() < n:
            bufs[i] = torch.empty(n, dtype=torch.uint8, device=self.device)
        return bufs[i]

    def __call__(self, img, mask, plan):
        img, mask = _as_u8(img, 3), _as_u8(mask, 2)
        if img.shape[2] != 3:
            raise ValueError("image must be [H][W][3] RGB")
        h, w = int(img.shape[0]), int(img.shape[1])
        if (int(mask.shape[0]), int(mask.shape[1])) != (h, w):
            raise ValueError("mask and image sizes differ")
        if h < 1 or w < 1 or h >= 32768 or w >= 32768:
            raise ValueError(f"image {w}x{h}: sides must be in [1, 32768) (Pillow takes other code paths beyond)")
        plan = list(plan)
        for op, params in plan:                                          # validate before the first launch
            if op not in AUG_OPS:
                raise ValueError(f"unknown augmentation {op!r}")
            if op == "rotation" and not abs(float(params[0])) < 90:
                raise ValueError("rotation: degrees >= 90 are not supported (Pillow's transpose paths)")
            if op == "crop":
                x1, y1, cw, ch = (int(v) for v in params)
                if x1 < 0 or y1 < 0 or cw < 1 or ch < 1 or x1 + cw > w or y1 + ch > h:
                    raise ValueError(f"crop box {params} leaves the {w}x{h} image")
        cur_i = img.to(self.device, non_blocking=True).contiguous()
        cur_m = mask.to(self.device, non_blocking=True).contiguous()
        st = _stream()
        ni, nm = h * w * 3, h * w
        state = {"i": 0, "m": 0}

        def next_img():
            state["i"] ^= 1
            return self._scratch(self._img, state["i"], ni)[:ni].view(h, w, 3)

        def next_mask():
            state["m"] ^= 1
            return self._scratch(self._mask, state["m"], nm)[:nm].view(h, w)

        for op, params in plan:
            if op in ("fliplr", "flipud"):
                oi, om = next_img(), next_mask()
                L.call("ydl_aug_flip", _p(cur_i), _p(oi), h, w, 3, int(op == "fliplr"), st)
                L.call("ydl_aug_flip", _p(cur_m), _p(om), h, w, 1, int(op == "fliplr"), st)
                cur_i, cur_m = oi, om
            elif op == "rotation":
                angle = float(params[0]) % 360.0
                if angle == 0:                                           # Image.rotate: a copy
                    continue
                m = _rotate_matrix(w, h, angle)
                if m[1] == 0.0 and m[3] == 0.0:
                    # an angle so small (or so close to 360) that sin rounds to 0 at 15 decimals: cos is 1 then, the matrix is the
                    # identity, and both of Pillow's paths (bilinear transform; ImagingScaleAffine for NEAREST) return the source bytes
                    continue
                oi, om = next_img(), next_mask()
                L.call("ydl_aug_rotate_image", _p(cur_i), _p(oi), h, w, *m, st)
                L.call("ydl_aug_rotate_mask", _p(cur_m), _p(om), h, w, *_rotate_fixed(m), st)
                cur_i, cur_m = oi, om
            elif op == "brightness":
                oi = next_img()
                L.call("ydl_aug_brightness", _p(cur_i), _p(oi), h, w, float(params[0]), st)
                cur_i = oi
            elif op == "contrast":
                oi = next_img()
                L.call("ydl_aug_contrast", _p(cur_i), _p(oi), h, w, float(params[0]), _p(self._sum), st)
                cur_i = oi
            elif op == "blur":
                R, ww, fw = _box_weights(float(params[0]))
                for vertical in (0, 0, 0, 1, 1, 1):
                    oi = next_img()
                    L.call("ydl_aug_box_blur", _p(cur_i), _p(oi), h, w, vertical, R, ww, fw, st)
                    cur_i = oi
            else:                                                        # crop
                x1, y1, cw, ch = (int(v) for v in params)
                if (cw, ch) == (w, h):                                   # the whole image resized to its own size: a copy
                    continue
                xb = xk = yb = yk = tmp = None
                xks = yks = 0
                if cw != w:
                    xb, xk, xks = self._tables.get("bil", cw, w)
                    tmp = self._scratch(self._img, 2, ch * w * 3)
                if ch != h:
                    yb, yk, yks = self._tables.get("bil", ch, h)
                xt, yt = self._tables.get("near", cw, w), self._tables.get("near", ch, h)
                # all six tables stay referenced by these locals until both launches are enqueued, whatever the cache evicts
                oi, om = next_img(), next_mask()
                L.call("ydl_aug_crop_image", _p(cur_i), h, w, x1, y1, cw, ch, _p(tmp) if tmp is not None else None, _p(oi),
                       _p(xb) if xb is not None else None, _p(xk) if xk is not None else None, xks,
                       _p(yb) if yb is not None else None, _p(yk) if yk is not None else None, yks, st)
                L.call("ydl_aug_crop_mask", _p(cur_m), h, w, x1, y1, cw, ch, _p(om), _p(xt), _p(yt), st)
                cur_i, cur_m = oi, om
        return cur_i, cur_m
