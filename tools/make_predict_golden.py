#!/usr/bin/env python3
"""Dev-time generator of tests/golden/predict_*.npz: the reference's OWN picture, class-weight and test-metric code, run on small inputs.

    python tools/make_predict_golden.py --reference <checkout of the reference project>

Nothing of the reference is copied: line ranges of its files are exec'd in a scratch namespace and only inputs and recorded outputs
are written (plus the CamVid colour table and class names, as arrays: data the pictures are drawn with).

  predict_render.npz    unet-lite/yolo5-seg/seg_diceloss_yolov5.py:810-830 (mask_to_rgb, visualize_prediction_difference) with its
                        colour table (:61-71): c<k>/gt, c<k>/pred (labels beyond the table included), c<k>/colour, c<k>/difference,
                        palette [12][3], names
  predict_weights.npz   :753-771 (seg_labels_to_class_weights) fed temporary JSON files: mask_<i>, nc, weights; mask_2 holds a label
                        == nc and mask_4 a negative one (both are skipped by the reference's try/except)
  predict_metrics.npz   unet-lite/Resnet50/test.py:410-464 (SegmentationMetrics): pred [B][H][W], target [B][H][W] int64 with -1, nc
                        and 255 among the targets and one class that never occurs; matrix, mIoU, IoU, Accuracy, Class_Accuracy"""
import argparse
import json
import logging
import os
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
NC = 12


def _lines(path):
    return open(path, encoding="utf-8").read().split("\n")


def load_train_script(ref):
    path = os.path.join(ref, "unet-lite", "yolo5-seg", "seg_diceloss_yolov5.py")
    lines = _lines(path)
    ns = dict(np=np, torch=torch, json=json, LOGGER=logging.getLogger("make_predict_golden"))
    for a, b in ((61, 71), (753, 771), (810, 830)):
        exec(compile("\n" * (a - 1) + "\n".join(lines[a - 1:b]), path, "exec"), ns)
    return ns


def load_test_script(ref):
    path = os.path.join(ref, "unet-lite", "Resnet50", "test.py")
    ns = dict(np=np, torch=torch, F=F)
    exec(compile("\n" * 409 + "\n".join(_lines(path)[410 - 1:464]), path, "exec"), ns)
    return ns


def gen_render(ns):
    arrs = {"palette": np.array(ns["CAMVID_COLORS"], np.uint8), "names": np.array(ns["CLASS_NAMES"])}
    for c, (h, w) in enumerate([(9, 13), (16, 5)]):
        rs = np.random.RandomState(7100 + c)
        gt = rs.randint(0, NC + 2, size=(h, w)).astype(np.uint8)
        pred = np.where(rs.rand(h, w) < 0.6, gt, rs.randint(0, NC + 2, size=(h, w))).astype(np.uint8)
        arrs.update({f"c{c}/gt": gt, f"c{c}/pred": pred, f"c{c}/colour": ns["mask_to_rgb"](pred),
                     f"c{c}/difference": ns["visualize_prediction_difference"](gt, pred)})
    np.savez_compressed(os.path.join(OUT, "predict_render.npz"), **arrs)
    print("predict_render", {k: v.shape for k, v in arrs.items()})


def gen_weights(ns):
    rs = np.random.RandomState(7200)
    masks = [rs.randint(0, NC, size=n).astype(np.int64) for n in (40, 77, 30, 64, 25, 51)]
    masks[0][masks[0] == 5] = 3                 # a class that is rare, and one (7) that never occurs anywhere
    for m in masks:
        m[m == 7] = 0
    masks[2][4] = NC                            # np.bincount grows past minlength: the += raises, the file is skipped
    masks[4][9] = -1                            # np.bincount refuses negatives: skipped
    with tempfile.TemporaryDirectory() as d:
        files = []
        for i, m in enumerate(masks):
            files.append(os.path.join(d, f"m{i}.json"))
            with open(files[-1], "w") as f:
                json.dump({"mask_data": m.tolist()}, f)
        w = ns["seg_labels_to_class_weights"](files, NC)
    arrs = {f"mask_{i}": m for i, m in enumerate(masks)}
    arrs.update(nc=np.array(NC), weights=w.numpy())
    np.savez_compressed(os.path.join(OUT, "predict_weights.npz"), **arrs)
    print("predict_weights", w.tolist())


def gen_metrics(ns):
    rs = np.random.RandomState(7300)
    B, H, W = 3, 11, 14
    target = rs.randint(0, NC, size=(B, H, W)).astype(np.int64)
    target[target == 9] = 2                     # class 9 never occurs as a target
    pred = np.where(rs.rand(B, H, W) < 0.7, target, rs.randint(0, NC, size=(B, H, W))).astype(np.int64)
    target[0, 0, :5] = -1
    target[1, 3, 2:6] = 255
    target[2, 10, 7:] = NC
    m = ns["SegmentationMetrics"](NC)
    for p, t in zip(pred, target):
        m.update(torch.from_numpy(p), torch.from_numpy(t))
    r = m.get_metrics()
    np.savez_compressed(os.path.join(OUT, "predict_metrics.npz"), pred=pred.astype(np.uint8), target=target, nc=np.array(NC),
                        matrix=m.confusion_matrix, mIoU=np.array(r["mIoU"]), IoU=r["IoU"], Accuracy=np.array(r["Accuracy"]),
                        Class_Accuracy=r["Class_Accuracy"])
    print("predict_metrics", float(r["mIoU"]), float(r["Accuracy"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference project")
    a = ap.parse_args()
    train = load_train_script(a.reference)
    gen_render(train)
    gen_weights(train)
    gen_metrics(load_test_script(a.reference))
