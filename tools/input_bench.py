#!/usr/bin/env python3
"""What the per-sample input path costs: plan + augment + letterbox on the GPU (AugmentGPU + LetterboxGPU) against the same chain
in Pillow on the host, and a training step with and without the GPU stage in front of it.

    python tools/input_bench.py [--raw 960x720] [--imgsz 640] [--batch 16] [--batches 20] [--threads 16] [--no-train]

Prints one line per measurement; every figure is a wall-clock mean over the stated number of batches after warm-up, GPU legs
bracketed by torch.cuda.synchronize().  The plans are drawn ONCE (``--batches`` x ``--batch`` of them, seed 0) and every leg, GPU or
host, walks the same list, so all legs do the same work; drawing a plan is timed on its own.  The host leg runs the reference's
ops (ImageOps / Image.rotate / ImageEnhance / ImageFilter / crop + resize, then resize + paste + /255) in a thread pool (Pillow
releases the GIL inside its C loops)."""
import argparse
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pil_sample(img, mask, plan, S):
    from PIL import Image, ImageEnhance, ImageFilter, ImageOps
    im, mk = Image.fromarray(img), Image.fromarray(mask)
    for op, p in plan:
        if op == "fliplr":
            im, mk = ImageOps.mirror(im), ImageOps.mirror(mk)
        elif op == "flipud":
            im, mk = ImageOps.flip(im), ImageOps.flip(mk)
        elif op == "rotation":
            im, mk = im.rotate(p[0], resample=Image.BILINEAR), mk.rotate(p[0], resample=Image.NEAREST)
        elif op == "brightness":
            im = ImageEnhance.Brightness(im).enhance(p[0])
        elif op == "contrast":
            im = ImageEnhance.Contrast(im).enhance(p[0])
        elif op == "blur":
            im = im.filter(ImageFilter.GaussianBlur(radius=p[0]))
        else:
            w, h = im.size
            box = (p[0], p[1], p[0] + p[2], p[1] + p[3])
            im, mk = im.crop(box).resize((w, h), Image.BILINEAR), mk.crop(box).resize((w, h), Image.NEAREST)
    w, h = im.size
    scale = min(S / w, S / h)
    nw, nh = int(w * scale), int(h * scale)
    ci, cm = Image.new("RGB", (S, S), (128, 128, 128)), Image.new("L", (S, S), 0)
    ci.paste(im.resize((nw, nh), Image.BILINEAR), ((S - nw) // 2, (S - nh) // 2))
    cm.paste(mk.resize((nw, nh), Image.NEAREST), ((S - nw) // 2, (S - nh) // 2))
    return torch.from_numpy(np.array(ci)).permute(2, 0, 1).float() / 255.0, torch.from_numpy(np.array(cm)).long()


def timed(fn, n, warm=2, sync=False):
    for _ in range(warm):
        fn()
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--raw", default="960x720")
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    import yolo_dual_amd as ydl
    w, h = (int(v) for v in a.raw.lower().split("x"))
    S, B = a.imgsz, a.batch
    rs = np.random.RandomState(0)
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(B)]
    masks = [rs.randint(0, 12, (h, w)).astype(np.uint8) for _ in range(B)]
    dev_i, dev_m = [torch.from_numpy(x).cuda() for x in imgs], [torch.from_numpy(x).cuda() for x in masks]
    aug, lb = ydl.AugmentGPU(), ydl.LetterboxGPU(S, num_classes=12)
    out_i = torch.empty((B, 3, S, S), dtype=torch.float32, device="cuda")
    out_m = torch.empty((B, S, S), dtype=torch.int64, device="cuda")
    rng = random.Random(0)
    print(f"input_bench: raw {w}x{h} -> {S}, batch {B}, {a.batches} batches, host threads {a.threads}, "
          f"device {torch.cuda.get_device_name(0)}", flush=True)

    # ---- single ops, image + mask where the op has one: GPU (wall clock around 20 calls, synchronised) and Pillow (one thread) ----
    one = {"fliplr": (), "flipud": (), "rotation": (7.3,), "brightness": (1.2,), "contrast": (1.2,), "blur": (1.3,),
           "crop": (50, 40, int(w * 0.8), int(h * 0.8))}
    for op, p in one.items():
        g = timed(lambda: aug(dev_i[0], dev_m[0], [(op, p)]), 20, sync=True)
        c = timed(lambda: pil_sample(imgs[0], masks[0], [(op, p)], S), 3, warm=1) - timed(lambda: pil_sample(imgs[0], masks[0], [], S), 3, warm=1)
        print(f"op {op:10s}  gpu {g * 1e3:8.3f} ms   pillow (1 thread, net of letterbox) {c * 1e3:8.2f} ms", flush=True)
    c = timed(lambda: pil_sample(imgs[0], masks[0], [], S), 5, warm=1)
    g = timed(lambda: lb(dev_i[0], dev_m[0], out_i[0], out_m[0]), 20, sync=True)
    print(f"op {'letterbox':10s}  gpu {g * 1e3:8.3f} ms   pillow (1 thread) {c * 1e3:8.2f} ms", flush=True)

    # ---- whole batches: the same list of plans for every leg ----
    plans = [[aug.plan(w, h, rng) for _ in range(B)] for _ in range(a.batches)]
    nops = sum(len(p) for b in plans for p in b)
    t = timed(lambda: [aug.plan(w, h, rng) for _ in range(B)], 50)
    print(f"plans: {a.batches} batches x {B}, {nops / (a.batches * B):.2f} ops per sample; drawing one batch of plans {t * 1e3:.3f} ms", flush=True)
    turn = [0]

    def next_plans():
        turn[0] += 1
        return plans[turn[0] % len(plans)]

    def leg(fn, n, **kw):
        turn[0] = -1 - kw.get("warm", 2)              # warm-up consumes the tail of the list, the timed part starts at plans[0]
        return timed(fn, n, **kw)

    def gpu_batch(upload):
        ps = next_plans()
        for i in range(B):
            src_i, src_m = (imgs[i], masks[i]) if upload else (dev_i[i], dev_m[i])
            lb(*aug(src_i, src_m, ps[i]), out_i[i], out_m[i])

    for upload in (False, True):
        t = leg(lambda: gpu_batch(upload), a.batches, sync=True)
        print(f"gpu  augment+letterbox ({'host arrays, upload included' if upload else 'device-resident arrays'}): "
              f"{t * 1e3:8.2f} ms/batch  {B / t:9.1f} samples/s", flush=True)

    def gpu_lb_only():
        for i in range(B):
            lb(dev_i[i], dev_m[i], out_i[i], out_m[i])
    t = timed(gpu_lb_only, a.batches, sync=True)
    print(f"gpu  letterbox only (device-resident arrays): {t * 1e3:8.2f} ms/batch  {B / t:9.1f} samples/s", flush=True)

    for threads in sorted({1, a.threads}):
        with ThreadPoolExecutor(threads) as ex:
            def host_batch():
                ps = next_plans()
                return list(ex.map(lambda k: pil_sample(imgs[k], masks[k], ps[k], S), range(B)))
            t = leg(host_batch, a.batches, warm=1)
        print(f"host augment+letterbox in Pillow, {threads:2d} thread(s), all {a.batches} batches: {t * 1e3:8.2f} ms/batch  {B / t:9.1f} samples/s",
              flush=True)

    if a.no_train:
        return
    # ---- a train_seg.py-style step (yolov5, bf16, eager) fed by: a fixed batch / letterbox / augment + letterbox ----
    import train_seg
    opt = train_seg.parse_opt(["--batch-size", str(B), "--imgsz", str(S)])
    ydl.set_compute_dtype("bf16")
    model, loss_kind = train_seg.build_model(opt)
    model = model.cuda().train()
    crit = ydl.SegmentationLoss(12, 0.0, train_seg.class_weights("", 12).cuda())
    optim = ydl.smart_optimizer(model, "SGD", 0.01, 0.937, 5e-4, ema=True)
    gpu_batch(False)
    fixed_i, fixed_m = out_i.clone(), out_m.clone()

    def step(feed):
        if feed == "augment":
            gpu_batch(False)
            x, t_ = out_i, out_m
        elif feed == "letterbox":
            gpu_lb_only()
            x, t_ = out_i, out_m
        else:
            x, t_ = fixed_i, fixed_m
        optim.zero_grad()
        loss, _ = crit(model(x), t_)
        loss.backward()
        optim.step()

    for feed in ("fixed batch", "letterbox", "augment"):
        t = leg(lambda: step(feed), a.batches, warm=3, sync=True)
        print(f"train step (yolov5, bf16, eager, batch {B}) fed by {feed:12s}: {t * 1e3:8.2f} ms/step  {B / t:9.1f} images/s", flush=True)


if __name__ == "__main__":
    main()
