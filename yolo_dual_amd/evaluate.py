"""Validation metric of the seg scripts: argmax + confusion matrix + mIoU (unet-lite/yolo5-seg/val_diceloss.py:37-75).
The reference walks every pixel in a python loop (:56-58); here one HIP kernel does argmax over the class axis and a
block-local LDS histogram, then adds it to a device-resident int64 matrix."""
from __future__ import annotations

from typing import List, Tuple

import torch

from . import _lib as L
from .tape import _p, _stream


def _label_rows(t: torch.Tensor, what: str, dtypes) -> torch.Tensor:
    """a (N,H,W) or (H,W) label map on the GPU whose rows are dense (image and row strides are free)"""
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: label maps live on the GPU (yolo_dual_amd has no CPU fallback)")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError(f"{what} must be (N, H, W) or (H, W), got {tuple(t.shape)}")
    if t.dtype not in dtypes:
        raise TypeError(f"{what} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if t.stride(2) != 1 or t.stride(1) < t.size(2) or t.stride(0) < 0:
        t = t.contiguous()
    return t


def confusion_labels(matrix: torch.Tensor, num_classes: int, ignore_index: int, pred: torch.Tensor, target: torch.Tensor) -> None:
    """matrix[t][p] += 1 over two label maps (ydl_confusion_labels)"""
    pred = _label_rows(pred, "pred", (torch.uint8,))
    target = _label_rows(target, "target", (torch.uint8, torch.int64))
    if pred.shape != target.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    N, H, W = pred.shape
    L.call("ydl_confusion_labels", _p(pred), pred.stride(0), pred.stride(1), _p(target), int(target.dtype == torch.int64),
           target.stride(0), target.stride(1), N, H, W, num_classes, ignore_index, _p(matrix), _stream())


class ConfusionMatrix:
    def __init__(self, num_classes: int, ignore_index: int = 11, device="cuda"):
        self.num_classes = num_classes
        self.ignore_index = -1 if ignore_index is None else ignore_index
        self.matrix = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=device)

    def process_batch(self, preds: torch.Tensor, targets: torch.Tensor) -> None:
        """preds: (N,C,H,W) scores/probabilities (argmax taken on the GPU); targets: (N,H,W) int64."""
        if preds.dim() != 4 or preds.size(1) != self.num_classes:
            raise ValueError("preds must be (N, num_classes, H, W)")
        preds = preds.float()
        targets = targets.contiguous().long()
        N, C, H, W = preds.shape
        sn, sc, sh, sw = preds.stride()
        L.call("ydl_confusion_matrix", _p(preds), sn, sc, sh, sw, _p(targets), N, C, H, W, self.ignore_index,
               _p(self.matrix), _stream())

    def process_labels(self, pred_u8: torch.Tensor, targets: torch.Tensor) -> None:
        """pred_u8: (N,H,W) uint8 label map (yolo_dual_amd.predict); targets: (N,H,W) uint8 or int64.  The same matrix as
        ``process_batch`` on the scores the labels came from; a predicted label >= num_classes is dropped."""
        confusion_labels(self.matrix, self.num_classes, self.ignore_index, pred_u8, targets)

    def compute_iou(self) -> Tuple[float, List[float]]:
        m = self.matrix.cpu().double()
        ious = []
        for c in range(self.num_classes):
            if c == self.ignore_index:
                continue
            tp = m[c, c]
            union = m[:, c].sum() + m[c, :].sum() - tp
            ious.append(float(tp / union) if union != 0 else 0.0)
        return float(sum(ious) / len(ious)), ious
