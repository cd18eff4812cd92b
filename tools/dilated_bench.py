#!/usr/bin/env python3
"""Micro-benchmark of the dilated column kernels (ydl_dilated_cols / ydl_dilated_cols_bwd) at the stride-32 map of a 640 x 640
input: 256 and 512 channels @ 20^2, bs = 16, k = 3, d in {2, 6, 18}, both dtypes.

Per point and direction: the HBM byte floor (x read + col written, or d col read + d x written, at the 6.3 TB/s streaming rate of
DESIGN.md section 8), the new kernel, and the same convolution through ydl_deform_gather / ydl_deform_bwd with zero offsets (what
the library could do before; the backward includes clearing its f32 accumulator, as Tape.deform_conv does, but not the cast back
to the compute dtype).  Then, for the record, forward + backward of ASPP(256, 256) and RFB(256, 256) beside SPPF(256, 256, 5) on
the same map in both compute dtypes.

Device events; 10 warm-up runs and 40 timed runs per variant, each run ``--inner`` launches between two events, variants
alternated run by run; the median run is reported.

    python tools/dilated_bench.py [--inner 10]          (dev tool; one line per point)"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from yolo_dual_amd import _lib as L

STREAM_RATE = 6.3e12
WARMUP, RUNS = 10, 40
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3          # us


def medians(variants, inner):
    for fn in variants.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    t = {n: [] for n in variants}
    for _ in range(RUNS):
        for n, fn in variants.items():
            t[n].append(timed(fn, inner))
    return {n: statistics.median(v) for n, v in t.items()}


def kernels(inner):
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N, H, K = 16, 20, 3
    npix = N * H * H
    for C in (256, 512):
        for d in (2, 6, 18):
            for name, dt, tdt, es in (("bf16", L.YDL_BF16, torch.bfloat16, 2), ("f32 ", L.YDL_F32, torch.float32, 4)):
                ldc = K * K * C
                x = torch.randn(npix, C, device=dev).to(tdt)
                col = torch.empty(npix, ldc, device=dev, dtype=tdt)
                dcol = torch.randn(npix, ldc, device=dev).to(tdt)
                dx = torch.empty(npix, C, device=dev, dtype=tdt)
                off = torch.zeros(npix, 2 * K * K, device=dev, dtype=tdt)
                gin = torch.empty(npix, C, device=dev, dtype=torch.float32)
                goff = torch.empty(npix, 2 * K * K, device=dev, dtype=torch.float32)
                geo = (N, H, H, C, H, H, K, K, 1, 1, d, d, d, d, 1)

                def deform_bwd():
                    L.call("ydl_fill_zero", P(gin), gin.numel() * 4, st)
                    L.call("ydl_deform_bwd", dt, P(x), C, P(off), 2 * K * K, None, 0, 0, P(dcol), ldc, P(gin), P(goff), None, *geo, st)
                variants = {
                    "cols": lambda: L.call("ydl_dilated_cols", dt, P(x), C, P(col), ldc, 0, N, H, H, C, K, d, st),
                    "gather": lambda: L.call("ydl_deform_gather", dt, P(x), C, P(off), 2 * K * K, None, 0, 0, P(col), ldc, 0, *geo, st),
                    "cols_bwd": lambda: L.call("ydl_dilated_cols_bwd", dt, P(dcol), ldc, P(dx), C, 0, N, H, H, C, K, d, st),
                    "deform_bwd": deform_bwd,
                }
                m = medians(variants, inner)
                floor = npix * (C + ldc) * es / STREAM_RATE * 1e6        # the same bytes in both directions
                print(f"{C:3d} ch @ {H}^2 bs{N} d{d:<2d} {name} | floor {floor:5.1f} us | cols {m['cols']:6.1f} us  deform_gather "
                      f"{m['gather']:6.1f} us = {m['gather'] / m['cols']:5.2f}x | cols_bwd {m['cols_bwd']:6.1f} us  deform_bwd "
                      f"{m['deform_bwd']:7.1f} us = {m['deform_bwd'] / m['cols_bwd']:5.2f}x", flush=True)


def blocks():
    import yolo_dual_amd as ydl
    for mode in ("bf16", "f32"):
        ydl.set_compute_dtype(mode)
        torch.manual_seed(0)
        x = torch.randn(16, 256, 20, 20, device="cuda", requires_grad=True)
        g = torch.randn(16, 256, 20, 20, device="cuda")
        mods = {"ASPP(256,256)": ydl.ASPP(256, 256), "RFB(256,256)": ydl.RFB(256, 256), "SPPF(256,256,5)": ydl.SPPF(256, 256, 5)}
        variants = {}
        for n, mod in mods.items():
            mod = mod.cuda().train()

            def step(mod=mod):
                x.grad = None
                for p in mod.parameters():
                    p.grad = None
                mod(x).backward(g)
            variants[n] = step
        m = medians(variants, 1)
        print(f"blocks @ 20^2 bs16 {mode}: forward + backward (stand-alone region, host launch time included) | "
              + "  ".join(f"{n} {v:7.1f} us" for n, v in m.items()), flush=True)
    ydl.set_compute_dtype("bf16")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dilated_bench: needs a GPU (a CPU run cannot give a time)")
    kernels(opt.inner)
    blocks()
