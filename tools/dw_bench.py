#!/usr/bin/env python3
"""Micro-benchmark of the strided depth-wise entry points (ydl_dwconv2_fwd / _dgrad / _wgrad) at the depth-wise layers of the
width-0.5 Ghost backbone (models/hub/yolov5s-ghost.yaml) at 640 x 640, bs = 16, both dtypes:

  5x5 s1 (GhostConv.cv2) at C = 32, 8 and 16 on the 160^2 map and the corresponding layers at 80^2, 40^2 and 20^2; one 3x3 s2 layer
  (GhostBottleneck's DWConv) per scale.

Per shape: the HBM byte floor of the forward (input read once, output written once, at the 6.3 TB/s streaming rate of DESIGN.md
section 8), the forward with fused statistics, the forward alone, at s = 1 the pair it replaces (ydl_dwconv_fwd + ydl_bn_stats),
``torch.nn.functional.conv2d(groups=C)`` in channels_last, and the two gradients.  Device events after warm-up; the variants are
alternated round by round within one process and the median round is reported.

    python tools/dw_bench.py [--iters 20] [--rounds 5]          (dev tool; one line per shape and dtype)"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from yolo_dual_amd import _lib as L

STREAM_RATE = 6.3e12
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
# (C, H, k, s)
SHAPES = [(32, 160, 5, 1), (8, 160, 5, 1), (16, 160, 5, 1), (64, 80, 5, 1), (16, 80, 5, 1), (32, 80, 5, 1),
          (128, 40, 5, 1), (32, 40, 5, 1), (64, 40, 5, 1), (256, 20, 5, 1), (64, 20, 5, 1), (128, 20, 5, 1),
          (32, 160, 3, 2), (64, 80, 3, 2), (128, 40, 3, 2), (256, 20, 3, 2)]


def block(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    opt = ap.parse_args()
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = L.lib()
    N = 16
    for C, H, k, s in SHAPES:
        for name, dt, tdt, es in (("bf16", L.YDL_BF16, torch.bfloat16, 2), ("f32 ", L.YDL_F32, torch.float32, 4)):
            p = k // 2
            Ho = (H + 2 * p - k) // s + 1
            ld = (C + 7) // 8 * 8
            nin, nout = N * H * H, N * Ho * Ho
            x = torch.randn(nin, ld, device=dev).to(tdt)
            y = torch.empty(nout, ld, device=dev, dtype=tdt)
            dy = torch.randn(nout, ld, device=dev).to(tdt)
            dx = torch.empty(nin, ld, device=dev, dtype=tdt)
            w = torch.randn(C, k * k, device=dev) / k
            dw = torch.zeros(C, k * k, device=dev)
            ws = torch.empty(lib.ydl_bn_stats_ws_bytes(nout, C) // 4, device=dev)
            wsg = torch.empty(lib.ydl_dwconv2_wgrad_ws_bytes(C, k) // 4, device=dev)
            tx = x.view(N, H, H, ld)[..., :C].permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
            tw = w.view(C, 1, k, k).to(tdt)
            variants = {
                "fused": lambda: L.call("ydl_dwconv2_fwd", dt, P(x), ld, P(w), P(y), ld, P(ws), N, H, H, C, k, s, st),
                "fwd": lambda: L.call("ydl_dwconv2_fwd", dt, P(x), ld, P(w), P(y), ld, None, N, H, H, C, k, s, st),
                "torch": lambda: F.conv2d(tx, tw, stride=s, padding=p, groups=C),
                "dgrad": lambda: L.call("ydl_dwconv2_dgrad", dt, P(dy), ld, P(w), P(dx), ld, 0, N, H, H, C, k, s, st),
                "wgrad": lambda: L.call("ydl_dwconv2_wgrad", dt, P(x), ld, P(dy), ld, P(dw), P(wsg), N, H, H, C, k, s, st),
            }
            if s == 1:
                def pair():
                    L.call("ydl_dwconv_fwd", dt, P(x), ld, P(w), P(y), ld, N, H, H, C, k, p, st)
                    L.call("ydl_bn_stats", dt, P(y), ld, P(ws), nout, C, st)
                variants["pair"] = pair
                variants["old_fwd"] = lambda: L.call("ydl_dwconv_fwd", dt, P(x), ld, P(w), P(y), ld, N, H, H, C, k, p, st)
            for fn in variants.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {n: [] for n in variants}
            for _ in range(opt.rounds):
                for n, fn in variants.items():
                    t[n].append(block(fn, opt.iters))
            m = {n: statistics.median(v) for n, v in t.items()}
            floor = (nin + nout) * C * es / STREAM_RATE * 1e6
            line = (f"{C:3d} ch @ {H:3d}^2 k{k} s{s} {name} | floor {floor:5.1f} us | fwd+stats {m['fused']:6.1f} us  fwd {m['fwd']:6.1f} us")
            if s == 1:
                line += f" | dwconv_fwd {m['old_fwd']:6.1f} us  +bn_stats {m['pair']:6.1f} us = {m['pair'] / m['fused']:4.2f}x fused"
            line += f" | torch conv2d {m['torch']:6.1f} us = {m['torch'] / m['fwd']:4.2f}x fwd | dgrad {m['dgrad']:6.1f} us  wgrad {m['wgrad']:6.1f} us"
            print(line, flush=True)


if __name__ == "__main__":
    main()
