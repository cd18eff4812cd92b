#!/usr/bin/env python3
"""Micro-benchmark of the one-launch optimizer steps (SGD / Adam / AdamW / RMSProp + EMA) on the arenas of the BASELINE config 2
model (dev tool).  One real forward/backward at a small batch leaves the touched flags of a training step (the dead head layers stay
untouched), so every rule runs the run table a training step runs.  Each rule is timed per launch with HIP events: warm-up, then
REPS single launches, median.  Effective rate = words per parameter x 4 B x parameters / time (SGD 7 words, the others 9; RMSProp
without momentum would be 7).

    python tools/optim_bench.py [--reps 40] [--warmup 10]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import yaml
import yolo_dual_amd as ydl

CW = [1, 2, 25, 2, 10, 3, 25, 10, 5, 15, 25, 1]
WORDS = {"SGD": 7, "Adam": 9, "AdamW": 9, "RMSProp": 9}


def build(name: str):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "yolo_dual_amd", "cfg", "yolov5_seg.yaml")))
    for sec in ("backbone", "head"):
        for l in cfg[sec]:
            l[2] = {"C3_DCN": "C3"}.get(l[2], l[2])
    torch.manual_seed(0)
    m = ydl.YOLOv5Seg(cfg).cuda().train()
    m.img_size = [128, 128]
    opt = ydl.smart_optimizer(m, name, 0.01, 0.937, 5e-4)
    crit = ydl.SegmentationLoss(12, 0.0, torch.tensor(CW, dtype=torch.float32), "dice", sync=False)
    x = torch.rand(2, 3, 128, 128, device="cuda")
    t = torch.randint(0, 12, (2, 128, 128), device="cuda")
    for _ in range(2):                      # the second step has every momentum buffer (SGD: no first-step runs any more)
        opt.zero_grad()
        loss, _items = crit(m(x), t)
        loss.backward()
        opt.step()
    return m, opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    assert args.reps >= 20
    res = {}
    for name in ("SGD", "Adam", "AdamW", "RMSProp"):
        m, opt = build(name)
        opt.ensure_hyper()
        live = sum(n for p, _o, n, _g in opt._slots if getattr(p, "_ydl_touched", False))
        rows = opt._run_rows(opt._runs(commit=False))
        for _ in range(args.warmup):
            opt.prepare_step(1.0)
            opt.step_device_hyper()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            opt.prepare_step(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt.step_device_hyper()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        assert bool(torch.isfinite(opt.params_arena).all())
        us = statistics.median(ts)
        nbytes = 4.0 * WORDS[name] * opt.n_params      # nominal: the few dead parameters and the float buffers stream 3 words (EMA only)
        res[name] = (us, nbytes / us / 1e3)
        q1, _q2, q3 = statistics.quantiles(ts, n=4)
        print(f"{name:8s} runs {len(rows):3d}  params {opt.n_params}  live {live}  total {opt.n_total} | median {us:7.1f} us "
              f"(min {min(ts):.1f}, IQR {q3 - q1:.1f}, max {max(ts):.1f}) | {WORDS[name]} words/param | {res[name][1]:7.1f} GB/s", flush=True)
        del m, opt
        torch.cuda.empty_cache()
    for name in ("Adam", "AdamW", "RMSProp"):
        r = res[name][1] / res["SGD"][1]
        print(f"{name:8s} {r:.3f} x the SGD kernel's GB/s  ({'meets' if r >= 0.85 else 'MISSES'} the 0.85 expectation)")


if __name__ == "__main__":
    main()
