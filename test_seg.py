#!/usr/bin/env python3
"""Test entry point after unet-lite/Resnet50/test.py (:468-621) on the MI355X path: load a checkpoint, predict label maps, print the
test metrics (mIoU, accuracy, per-class IoU and accuracy; test.py:410-464, :592-602) and write pictures of the first samples.

Predictions leave the model as uint8 label maps (yolo_dual_amd.predict_labels: no softmax, no NCHW export); metrics come from a
device-resident confusion matrix; pictures are drawn on the GPU and un-letterboxed to the source size: ``<name>_colour.png``
(mask_to_rgb), ``<name>_difference.png`` (visualize_prediction_difference, when there are labels) and ``<name>_overlay.png``
(val_diceloss.py:103-119, in RGB).  The figure layout and legend of test.py:50-131 are not reproduced.

Inputs: synthetic "blobby" batches by default (train_seg.blobby_batch, as no dataset ships with the reference), or
``--source DIR [--labels DIR]``: images decoded with Pillow on the host and letterboxed on the GPU (LetterboxGPU); a label map is the
8-bit PNG of the same stem.

    python test_seg.py --weights runs/train-seg/best.pt --arch yolov5 --imgsz 640 --batch-size 16 --save-dir runs/test-seg
    python test_seg.py --weights best.pt --source data/test/images --labels data/test/labels --palette camvid.yaml
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import train_seg  # noqa: E402  (ARCH, build_model, blobby_batch)

IMG_EXT = (".png", ".jpg", ".jpeg", ".bmp")


def parse_opt(argv=None):
    p = argparse.ArgumentParser(description="segmentation test script on the HIP path")
    p.add_argument("--weights", type=str, default="", help="checkpoint (.pt with a state_dict under 'model'); '' = random init")
    p.add_argument("--cfg", type=str, default="", help="model yaml (default: the architecture's yaml under yolo_dual_amd/cfg)")
    p.add_argument("--arch", default="yolov5", choices=sorted(train_seg.ARCH))
    p.add_argument("--imgsz", "--img", "--img-size", type=int, default=640)
    p.add_argument("--batch-size", type=int, default=16)
    p.add_argument("--visualize-num", type=int, default=5, help="how many samples get pictures")
    p.add_argument("--save-dir", type=str, default="runs/test-seg")
    p.add_argument("--palette", type=str, default="", help="yaml (a list of [r, g, b], or a mapping with 'palette' and optionally 'names') "
                                                           "or npz ('palette', optionally 'names'); evenly spaced hues when absent")
    p.add_argument("--source", type=str, default="", help="directory of images; '' = synthetic batches")
    p.add_argument("--labels", type=str, default="", help="directory of 8-bit label PNGs with the images' stems (with --source)")
    p.add_argument("--batches", type=int, default=2, help="synthetic batches to test on")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f32"], help="compute dtype of the HIP kernels")
    p.add_argument("--dcn", default="substitute", choices=["substitute", "native"])
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", default="", help="cuda device index")
    opt = p.parse_args(argv)
    if opt.labels and not opt.source:
        p.error("--labels needs --source")
    return opt


def load_palette(path: str, nc: int):
    """-> (uint8 [K][3] host tensor, class names)"""
    import numpy as np
    import torch
    import yaml
    import yolo_dual_amd as ydl
    names = None
    if not path:
        pal = ydl.default_palette(nc)
    elif path.endswith(".npz"):
        z = np.load(path)
        pal = torch.from_numpy(np.asarray(z["palette"], dtype=np.uint8))
        names = [str(n) for n in z["names"]] if "names" in z.files else None
    else:
        d = yaml.safe_load(open(path))
        if isinstance(d, dict):
            names = d.get("names")
            d = d["palette"]
        pal = torch.tensor(d, dtype=torch.uint8)
    if pal.dim() != 2 or pal.size(1) != 3:
        raise ValueError(f"{path}: a palette is a list of [r, g, b] triples")
    return pal.contiguous(), list(names) if names else [str(i) for i in range(nc)]


def _source_batches(opt, lb, device):
    """batches of (imgs, targets or None, [(name, w, h, img_u8 on the device, mask_u8 on the device or None)])"""
    import numpy as np
    import torch
    from PIL import Image
    files = sorted(f for f in os.listdir(opt.source) if f.lower().endswith(IMG_EXT))
    if not files:
        raise FileNotFoundError(f"no images under {opt.source}")
    for b0 in range(0, len(files), opt.batch_size):
        imgs, masks, meta = [], [], []
        for f in files[b0:b0 + opt.batch_size]:
            stem = os.path.splitext(f)[0]
            img = torch.from_numpy(np.array(Image.open(os.path.join(opt.source, f)).convert("RGB"))).to(device)
            mask = None
            if opt.labels:
                mask = torch.from_numpy(np.array(Image.open(os.path.join(opt.labels, stem + ".png")).convert("L"))).to(device)
            imgs.append(img)
            masks.append(mask)
            meta.append((stem, int(img.shape[1]), int(img.shape[0]), img, mask))
        x, t = lb.batch(imgs, masks if opt.labels else None)
        yield x, t, meta


def _synthetic_batches(opt, nc, device):
    import torch
    gen = torch.Generator(device=device).manual_seed(99 + opt.seed)
    colours = torch.rand(nc, 3, device=device, generator=torch.Generator(device=device).manual_seed(7))
    S = opt.imgsz
    for b in range(opt.batches):
        x, t = train_seg.blobby_batch(gen, opt.batch_size, S, nc, device, colours)
        yield x, t, [(f"synthetic_{b}_{i}", S, S, None, None) for i in range(opt.batch_size)]


def main(argv=None) -> dict:
    import numpy as np
    import torch
    from PIL import Image
    import yolo_dual_amd as ydl

    opt = argv if isinstance(argv, argparse.Namespace) else parse_opt(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("test_seg.py runs on the GPU only (yolo_dual_amd has no CPU fallback)")
    device = torch.device("cuda", int(opt.device) if str(opt.device).isdigit() else 0)
    torch.cuda.set_device(device)
    torch.manual_seed(opt.seed)
    ydl.set_compute_dtype(opt.dtype)
    os.makedirs(opt.save_dir, exist_ok=True)

    model, _ = train_seg.build_model(opt)
    nc = model.num_classes
    if opt.weights:
        n, tot = ydl.load_weights(model, ydl.load_checkpoint(opt.weights))
        print(f"[test_seg] loaded weights: {n}/{tot} entries match")
    else:
        print("[test_seg] no --weights: testing a randomly initialised model")
    model = model.to(device).eval()
    print(f"[test_seg] classes: {nc}  input: {opt.imgsz}x{opt.imgsz}  parameters: {sum(p.numel() for p in model.parameters()):,}")
    palette, names = load_palette(opt.palette, nc)
    palette = palette.to(device)

    S = opt.imgsz
    lb = ydl.LetterboxGPU(S, num_classes=nc, device=device) if opt.source else None
    batches = _source_batches(opt, lb, device) if opt.source else _synthetic_batches(opt, nc, device)
    metrics = ydl.SegmentationMetrics(nc, device=device)
    seen, scored, written = 0, 0, []
    for x, t, meta in batches:
        labels = ydl.predict_labels(model, x)
        if tuple(labels.shape[1:]) != (S, S):
            raise RuntimeError(f"the model predicts {tuple(labels.shape[1:])}, not the {S}x{S} input (set --imgsz to its output size)")
        if t is not None:
            metrics.update(labels, t)
            scored += len(meta)
        for i, (name, w, h, img_u8, mask_u8) in enumerate(meta):
            if seen + i >= opt.visualize_num:
                break
            pred = ydl.unletterbox_labels(labels[i], w, h, S)                   # back to the source's size
            if img_u8 is not None:
                img = img_u8.permute(2, 0, 1).float().div(255.0).contiguous()      # k / 255 * 255 truncates back to k for every byte
                gt = mask_u8
            else:
                img, gt = x[i], (t[i].to(torch.uint8) if t is not None else None)
            pics = {"colour": ydl.colorize(pred, palette), "overlay": ydl.overlay(img, pred, palette)}
            if gt is not None:
                pics["difference"] = ydl.difference(gt.contiguous(), pred, palette)
            for kind, pic in pics.items():
                path = os.path.join(opt.save_dir, f"{name}_{kind}.png")
                Image.fromarray(np.ascontiguousarray(pic.cpu().numpy())).save(path)
                written.append(path)
        seen += len(meta)

    res = metrics.get_metrics() if scored else {}
    print(f"\n[test_seg] samples: {seen}  pictures: {len(written)} under {opt.save_dir}")
    if scored:
        print("\n===== test set results =====")
        print(f"mIoU: {res['mIoU']:.4f}")
        print(f"Accuracy: {res['Accuracy']:.4f}")
        print("\nIoU per class:")
        for i, (n_, v) in enumerate(zip(names, res["IoU"])):
            print(f"  class {i} ({n_}): {v:.4f}")
        print("\nAccuracy per class:")
        for i, (n_, v) in enumerate(zip(names, res["Class_Accuracy"])):
            print(f"  class {i} ({n_}): {v:.4f}")
    res = dict(res)
    res["files"] = written
    res["samples"] = seen
    return res


if __name__ == "__main__":
    main()
