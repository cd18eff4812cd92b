"""The test / predict path: what the reference does with a trained model besides mIoU, on the HIP kernels of csrc/predict.hip.

  label maps      argmax_labels, predict_labels, unletterbox_labels          (unet-lite/Resnet50/test.py:536-547)
  test metrics    SegmentationMetrics, ConfusionMatrix.process_labels       (test.py:410-464)
  class weights   label_class_weights                                       (seg_diceloss_yolov5.py:753-771)
  pictures        colorize, difference, overlay                             (seg_diceloss_yolov5.py:810-830, val_diceloss.py:103-119)

A label map is a uint8 tensor on the GPU.  ``model(x)`` is not changed by anything here: ``predict_labels`` runs the same taped forward
with one flag set, so that the argmax is taken of the scores where they are stored (NHWC, compute dtype, before the lazy nearest
up-sampling) instead of the f32 NCHW probabilities at full resolution."""
from __future__ import annotations

import colorsys
import logging
from typing import Dict, Iterable, Sequence

import numpy as np
import torch

from . import _lib as L
from . import config
from .data import letterbox_geometry
from .evaluate import _label_rows, confusion_labels
from .tape import Tape, _p, _stream

LOGGER = logging.getLogger("yolo_dual_amd")


def argmax_labels(scores: torch.Tensor) -> torch.Tensor:
    """(N, C, H, W) f32 or bf16 scores with any strides -> uint8 (N, H, W), by torch.argmax's rule (first maximum; a NaN is the maximum)"""
    if scores.device.type != "cuda":
        raise RuntimeError("argmax_labels runs on the GPU only (yolo_dual_amd has no CPU fallback)")
    if scores.dim() != 4:
        raise ValueError(f"scores must be (N, C, H, W), got {tuple(scores.shape)}")
    if scores.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"scores must be float32 or bfloat16, got {scores.dtype}")
    if any(s < 0 for s in scores.stride()):
        scores = scores.contiguous()
    N, C, H, W = scores.shape
    out = torch.empty((N, H, W), dtype=torch.uint8, device=scores.device)
    sn, sc, sh, sw = scores.stride()
    L.call("ydl_argmax_labels", L.YDL_F32 if scores.dtype == torch.float32 else L.YDL_BF16, _p(scores), sn, sc, sh, sw, N, C, H, W, 1, 1,
           _p(out), H * W, W, _stream())
    return out


def predict_labels(model: torch.nn.Module, imgs: torch.Tensor) -> torch.Tensor:
    """The label map of ``model``'s prediction for ``imgs`` (N, 3, H, W): uint8 (N, Ho, Wo) at the model's output size, equal to
    ``model.eval()(imgs).argmax(1)`` except where two classes tie after the softmax but not before it.

    The model's own taped forward runs in eval mode under no_grad with ``Tape.labels_out`` set; the output leaves through
    ``Tape.export_labels``.  A model that ends in ``nn.Softmax`` at its output size (every shipped yaml) launches neither
    ydl_softmax_fwd nor ydl_nhwc_to_nchw: the argmax is taken of the scores that layer reads, with the lazy replication folded into
    the store.  Serves the yaml models (YOLOv5Seg / YOLOv8Seg / YOLOv9Seg / ResNet50SegYaml), ResNet18Seg / ResNet50Seg and
    SegYoloModel: anything whose ``_fwd(tape, x)`` returns one Var (or, with the flag set, the label map itself)."""
    from .modules import refresh_weights
    if not hasattr(model, "_fwd") or getattr(model, "takes_list", False):
        raise TypeError(f"predict_labels needs a yolo_dual_amd model with a taped forward, got {type(model).__name__}")
    if imgs.device.type != "cuda":
        raise RuntimeError("yolo_dual_amd runs on the GPU only: there is no CPU fallback for the HIP kernels "
                           "(move the module and its inputs to cuda)")
    if imgs.dim() != 4:
        raise ValueError(f"imgs must be (N, 3, H, W), got {tuple(imgs.shape)}")
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            tape = Tape(config.compute_dtype(), imgs.device, False, False)
            tape.labels_out = True
            tape._slab_hint = getattr(model, "_ydl_slab_need", 0)
            refresh_weights(model, tape)
            x = tape.input_nchw(imgs, lazy=True)
            x.need = False
            res = model._fwd(tape, x)
            return res if isinstance(res, torch.Tensor) else tape.export_labels(res)
    finally:
        model.train(was_training)


def unletterbox_labels(labels: torch.Tensor, w: int, h: int, img_size: int) -> torch.Tensor:
    """Undo ``LetterboxGPU(img_size)`` on a label map: the interior ``letterbox_geometry(w, h, img_size)`` gives, resized to the
    source's (h, w) by ATen's nearest rule (F.interpolate(mode='nearest') of the box).  labels: uint8 (S, S) -> uint8 (h, w);
    (N, S, S) -> (N, h, w) for sources of one size.

    test.py:419-424 is not reproduced: its ``unsqueeze(0)`` turns the call into a 1-D resize along the width only, and it raises for
    the int64 predictions it is given."""
    squeeze = labels.dim() == 2
    src = _label_rows(labels, "labels", (torch.uint8,))
    N, S1, S2 = src.shape
    if (S1, S2) != (img_size, img_size):
        raise ValueError(f"labels are {S1}x{S2}, not the letterbox canvas {img_size}x{img_size}")
    new_w, new_h, pl, pt = letterbox_geometry(w, h, img_size)
    out = torch.empty((N, h, w), dtype=torch.uint8, device=src.device)
    L.call("ydl_labels_resize", _p(src), src.stride(0), src.stride(1), N, pt, pl, new_h, new_w, _p(out), h * w, w, h, w, _stream())
    return out[0] if squeeze else out


class SegmentationMetrics:
    """test.py:410-464 on a device-resident int64 confusion matrix (rows = target).  ``update`` takes label maps; a target outside
    [0, num_classes) is dropped as the reference's mask does, and so is a predicted label >= num_classes (the reference would file
    it under another cell)."""

    def __init__(self, num_classes: int, device="cuda"):
        self.num_classes = int(num_classes)
        self.confusion_matrix = torch.zeros((self.num_classes, self.num_classes), dtype=torch.int64, device=device)

    def update(self, pred_labels: torch.Tensor, target_labels: torch.Tensor) -> None:
        confusion_labels(self.confusion_matrix, self.num_classes, -1, pred_labels, target_labels)

    def get_metrics(self) -> Dict[str, object]:
        m = self.confusion_matrix.cpu().numpy()
        diag = np.diag(m)
        iou = diag / (np.sum(m, axis=1) + np.sum(m, axis=0) - diag + 1e-10)
        return {"mIoU": np.nanmean(iou), "IoU": iou, "Accuracy": diag.sum() / (m.sum() + 1e-10),
                "Class_Accuracy": diag / (np.sum(m, axis=1) + 1e-10)}


def label_class_weights(masks: Iterable, num_classes: int, device="cuda") -> torch.Tensor:
    """seg_labels_to_class_weights on label maps instead of JSON files: ``total / (nc * (counts + 1e-8))`` in float64, returned as
    float32 [num_classes] on the host.  masks: uint8 or int64 tensors / arrays of any shape.  A mask holding a label >= num_classes
    (or a negative one) is skipped whole with a warning, counts and total alike, as the reference's try/except around np.bincount
    does.  One histogram launch per mask, one read-back for all of them."""
    nc = int(num_classes)
    masks = list(masks)
    rows = torch.zeros((max(len(masks), 1), nc + 1), dtype=torch.int64, device=device)
    for i, m in enumerate(masks):
        t = torch.as_tensor(m)
        if t.dtype not in (torch.uint8, torch.int64):
            t = t.long()
        t = t.to(rows.device).contiguous()
        L.call("ydl_label_bincount", _p(t), int(t.dtype == torch.int64), t.numel(), nc, _p(rows[i]), _stream())
    rows = rows.cpu().numpy()
    counts, total = np.zeros(nc, dtype=np.int64), 0
    for i in range(len(masks)):
        if rows[i, nc]:
            LOGGER.warning("label_class_weights: mask %d holds %d labels outside [0, %d): skipped", i, int(rows[i, nc]), nc)
            continue
        counts += rows[i, :nc]
        total += int(rows[i, :nc].sum())
    return torch.from_numpy(total / (nc * (counts + 1e-8))).float()


def default_palette(n: int) -> torch.Tensor:
    """``n`` evenly spaced hues at full saturation as a uint8 [n][3] host tensor (what test_seg.py draws with when no palette is given)"""
    rgb = [colorsys.hsv_to_rgb(k / max(n, 1), 1.0, 1.0) for k in range(n)]
    return torch.tensor([[int(round(255 * c)) for c in t] for t in rgb], dtype=torch.uint8).reshape(n, 3)


def _render(mode: int, pred, target, img, palette: torch.Tensor, bgr: bool) -> torch.Tensor:
    squeeze = pred.dim() == 2
    pred = _label_rows(pred, "labels", (torch.uint8,)).contiguous()
    N, H, W = pred.shape
    palette = torch.as_tensor(palette)
    if palette.dtype != torch.uint8 or palette.dim() != 2 or palette.size(1) != 3 or not 1 <= palette.size(0) <= 256:
        raise ValueError("palette must be a uint8 [K][3] tensor with 1 <= K <= 256")
    palette = palette.to(pred.device).contiguous()
    if target is not None:
        target = _label_rows(target, "target", (torch.uint8,)).contiguous()
        if target.shape != pred.shape:
            raise ValueError("target and pred differ in shape")
    if img is not None:
        img = img.unsqueeze(0) if img.dim() == 3 else img
        if tuple(img.shape) != (N, 3, H, W) or img.dtype != torch.float32 or img.device != pred.device:
            raise ValueError(f"img must be float32 {(N, 3, H, W)} on the labels' device")
        img = img.contiguous()
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=pred.device)
    L.call("ydl_labels_render", mode, _p(pred), _p(target), _p(img), _p(palette), palette.size(0), _p(out), N, H, W, int(bool(bgr)),
           _stream())
    return out[0] if squeeze else out


def colorize(labels: torch.Tensor, palette: torch.Tensor) -> torch.Tensor:
    """mask_to_rgb: uint8 (N, H, W) or (H, W) labels -> uint8 (..., H, W, 3), ``palette[label]`` or black for a label the palette lacks"""
    return _render(0, labels, None, None, palette, False)


def difference(target: torch.Tensor, pred: torch.Tensor, palette: torch.Tensor) -> torch.Tensor:
    """visualize_prediction_difference: magenta (255, 0, 255) where the two label maps differ, the palette colour where they agree"""
    return _render(1, pred, target, None, palette, False)


def overlay(img: torch.Tensor, labels: torch.Tensor, palette: torch.Tensor, bgr: bool = False) -> torch.Tensor:
    """val_diceloss.py:103-119: ``rint(0.5 * uint8(img * 255) + 0.5 * palette[label])``.  img: float32 (N, 3, H, W) or (3, H, W) in
    [0, 1].  ``bgr``: swap the image's channels (cv2.cvtColor(RGB2BGR)) and write the palette triple unswapped, as the reference
    does before cv2.imwrite.  The rounding (half to even, saturated) is OpenCV's documented saturate_cast of cv2.addWeighted; no cv2
    build was at hand to pin it against."""
    return _render(2, labels, None, img, palette, bgr)
