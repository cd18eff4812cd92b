"""numpy / torch-CPU restatement of the prediction path: what the kernels of csrc/predict.hip and yolo_dual_amd.predict must equal,
bit for bit.  tests/test_predict_ref_cpu.py pins it against recordings of the reference's own code (tests/golden/predict_*.npz) and
against F.interpolate; the GPU tests compare the kernels with it."""
import warnings

import numpy as np
import torch


# the resize cases of the GPU tests, shared with the CPU test that pins nearest_index against F.interpolate for the same size pairs:
# (box (y0, x0, hc, wc) on a 16 x 16 canvas, (Ho, Wo)), and the (w, h) sources un-letterboxed from a 64 x 64 canvas
RESIZE_CASES = [((3, 0, 10, 16), (7, 23)), ((3, 0, 10, 16), (10, 16)), ((0, 0, 1, 1), (4, 4)), ((2, 5, 9, 6), (1, 1))]
UNLETTERBOX_CASES = [(100, 37), (37, 100)]
UNLETTERBOX_S = 64


# ---------------------------------------------------------------------------------------------------- label maps
def argmax_labels(scores: torch.Tensor, rep=(1, 1)) -> torch.Tensor:
    """(N, C, H, W) scores -> uint8 (N, H*rep_h, W*rep_w): torch.argmax on the f32 copy (first maximum, a NaN is the maximum),
    each stored pixel filling its rep_h x rep_w block"""
    lab = torch.argmax(scores.detach().float().cpu(), dim=1).to(torch.uint8)
    return lab.repeat_interleave(rep[0], dim=1).repeat_interleave(rep[1], dim=2)


def nearest_index(n_in: int, n_out: int) -> np.ndarray:
    """ATen's nearest source index: min(floor(i * (float)n_in / n_out), n_in - 1), scale and product in float32"""
    scale = np.float32(n_in) / np.float32(n_out)
    idx = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, n_in - 1)


def labels_resize(src: np.ndarray, box, Ho: int, Wo: int) -> np.ndarray:
    """the crop box (y0, x0, hc, wc) of a (..., H, W) label map resized to (Ho, Wo) by the nearest rule"""
    y0, x0, hc, wc = box
    return src[..., y0 + nearest_index(hc, Ho)[:, None], x0 + nearest_index(wc, Wo)[None, :]]


def letterbox_box(w: int, h: int, S: int):
    """the interior of the S x S letterbox canvas for a w x h source, as (y0, x0, hc, wc)"""
    scale = min(S / w, S / h)
    new_w, new_h = int(w * scale), int(h * scale)
    return (S - new_h) // 2, (S - new_w) // 2, new_h, new_w


def unletterbox(labels: np.ndarray, w: int, h: int, S: int) -> np.ndarray:
    return labels_resize(labels, letterbox_box(w, h, S), h, w)


# ---------------------------------------------------------------------------------------------------- counting
def confusion(pred: np.ndarray, target: np.ndarray, C: int, ignore: int = -1) -> np.ndarray:
    """int64 [C][C], rows = target; pixels with t < 0, t >= C, t == ignore or p >= C are dropped"""
    p, t = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(target).reshape(-1).astype(np.int64)
    keep = (t >= 0) & (t < C) & (t != ignore) & (p < C)
    return np.bincount(C * t[keep] + p[keep], minlength=C * C).reshape(C, C).astype(np.int64)


def bincount(labels: np.ndarray, nbins: int) -> np.ndarray:
    """int64 [nbins + 1]; the last entry counts the labels outside [0, nbins)"""
    v = np.asarray(labels).reshape(-1).astype(np.int64)
    v = np.where((v < 0) | (v >= nbins), nbins, v)
    return np.bincount(v, minlength=nbins + 1).astype(np.int64)


def metrics(matrix: np.ndarray) -> dict:
    """test.py's four keys from a confusion matrix (rows = target)"""
    m = np.asarray(matrix)
    tp = np.diag(m)
    rows, cols = m.sum(axis=1), m.sum(axis=0)
    iou = tp / (rows + cols - tp + 1e-10)
    return {"mIoU": np.nanmean(iou), "IoU": iou, "Accuracy": tp.sum() / (m.sum() + 1e-10), "Class_Accuracy": tp / (rows + 1e-10)}


class SegmentationMetrics:
    def __init__(self, num_classes: int):
        self.num_classes = num_classes
        self.confusion_matrix = np.zeros((num_classes, num_classes), np.int64)

    def update(self, pred, target):
        self.confusion_matrix += confusion(pred, target, self.num_classes)

    def get_metrics(self):
        return metrics(self.confusion_matrix)


def class_weights(masks, nc: int) -> torch.Tensor:
    """total / (nc * (counts + 1e-8)) over the masks whose labels all lie in [0, nc); the others are skipped whole, with a warning"""
    counts, total = np.zeros(nc, np.int64), 0
    for i, m in enumerate(masks):
        b = bincount(m, nc)
        if b[nc]:
            warnings.warn(f"mask {i}: {int(b[nc])} labels outside [0, {nc})")
            continue
        counts += b[:nc]
        total += int(np.asarray(m).size)
    return torch.from_numpy(total / (nc * (counts + 1e-8))).float()


# ---------------------------------------------------------------------------------------------------- pictures
def _lookup(labels: np.ndarray, palette: np.ndarray) -> np.ndarray:
    table = np.zeros((256, 3), np.uint8)
    table[:len(palette)] = palette
    return table[np.asarray(labels, np.uint8)]


def colorize(labels: np.ndarray, palette: np.ndarray) -> np.ndarray:
    """palette[label], black for a label the palette lacks"""
    return _lookup(labels, palette)


def difference(gt: np.ndarray, pred: np.ndarray, palette: np.ndarray) -> np.ndarray:
    """magenta where the maps differ, the palette colour (or black) where they agree"""
    out = _lookup(pred, palette)
    out[np.asarray(gt) != np.asarray(pred)] = (255, 0, 255)
    return out


def overlay(img: np.ndarray, labels: np.ndarray, palette: np.ndarray, bgr: bool = False) -> np.ndarray:
    """img: float32 (3, H, W) in [0, 1].  base = uint8(img * 255) by truncation (the product in float32), channel-swapped with
    ``bgr``; out = rint(0.5 * base + 0.5 * colour), half to even (OpenCV's saturate_cast of addWeighted's float sum)"""
    base = np.clip(np.asarray(img, np.float32).transpose(1, 2, 0) * np.float32(255), 0, 255).astype(np.uint8)
    if bgr:
        base = base[..., ::-1]
    s = np.float32(0.5) * base.astype(np.float32) + np.float32(0.5) * _lookup(labels, palette).astype(np.float32)
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)
