#!/usr/bin/env python3
"""Micro-benchmark of the one-launch parallel pooling pyramid (ydl_spp_pool_fwd / ydl_spp_pool_bwd) against the route it replaces,
three ydl_maxpool_fwd / ydl_maxpool_bwd calls, at the stride-32 and stride-20 maps of a 640 x 640 input: bs = 16, k = (5, 9, 13),
256 and 512 channels, 20^2 and 32^2, both dtypes.  The buffers are laid out as SPP lays them out: x is slice 0 of the 4 C-channel
concat buffer and the pools write slices 1..3; backward, the three slice gradients are read and d x is accumulated into slice 0.

Per point and direction: the HBM byte floor (x read + three slices written, or three slice gradients read + d x written; the index
planes, a quarter to a half of that again, are not counted) at the 6.3 TB/s streaming rate of DESIGN.md section 8, the one launch,
and the three launches.  Before a point is timed, both routes run once on the same data and their outputs are compared bit for bit.

Device events; 10 warm-up runs and 40 timed runs per variant, each run ``--inner`` launches (or triples of launches) between two
events, variants alternated run by run; the median run is reported.

    python tools/spp_bench.py [--inner 10]          (dev tool; one line per point)"""
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
KS = (5, 9, 13)


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


def main(inner):
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N = 16
    for H in (20, 32):
        for C in (256, 512):
            for name, dt, tdt, es in (("bf16", L.YDL_BF16, torch.bfloat16, 2), ("f32 ", L.YDL_F32, torch.float32, 4)):
                npix, ld = N * H * H, 4 * C
                cat = torch.randn(npix, ld, device=dev).to(tdt)
                dcat = torch.randn(npix, ld, device=dev).to(tdt)
                idx = [torch.empty(npix * C, dtype=torch.uint8, device=dev) for _ in KS]
                P = lambda t, c=0: ctypes.c_void_p(t.data_ptr() + c * es)

                def fused_fwd(cat=cat, idx=idx):
                    L.call("ydl_spp_pool_fwd", dt, P(cat), ld, P(cat, C), P(cat, 2 * C), P(cat, 3 * C), ld, P(idx[0]), P(idx[1]), P(idx[2]),
                           N, H, H, C, *KS, st)

                def three_fwd(cat=cat, idx=idx):
                    for i, k in enumerate(KS):
                        L.call("ydl_maxpool_fwd", dt, P(cat), ld, P(cat, (i + 1) * C), ld, P(idx[i]), N, H, H, H, H, C, k, 1, k // 2, st)

                def fused_bwd(dcat=dcat, idx=idx):
                    L.call("ydl_spp_pool_bwd", dt, P(dcat, C), P(dcat, 2 * C), P(dcat, 3 * C), ld, P(idx[0]), P(idx[1]), P(idx[2]),
                           P(dcat), ld, 1, N, H, H, C, *KS, st)

                def three_bwd(dcat=dcat, idx=idx):
                    for i, k in enumerate(KS):
                        L.call("ydl_maxpool_bwd", dt, P(dcat, (i + 1) * C), ld, P(idx[i]), P(dcat), ld, 1, N, H, H, H, H, C, k, 1, k // 2, st)

                if not L.lib().ydl_spp_pool_supported(dt, H, H, C, *KS):
                    print(f"{C:3d} ch @ {H}^2 bs{N} {name} | not served by the one-launch form", flush=True)
                    continue
                # the same bits first (x is slice 0 and is not written by either forward)
                cat2, dcat2, idx2 = cat.clone(), dcat.clone(), [torch.empty_like(i) for i in idx]
                fused_fwd()
                three_fwd(cat2, idx2)
                fused_bwd()
                three_bwd(dcat2, idx2)
                torch.cuda.synchronize()
                bits = lambda t: t.view(torch.int16 if es == 2 else torch.int32)
                same = (torch.equal(bits(cat), bits(cat2)) and torch.equal(bits(dcat), bits(dcat2))
                        and all(torch.equal(a, b) for a, b in zip(idx, idx2)))
                dcat.copy_(dcat2)                       # d x accumulates run after run: both variants then work on the same values
                m = medians({"fused_fwd": fused_fwd, "three_fwd": three_fwd, "fused_bwd": fused_bwd, "three_bwd": three_bwd}, inner)
                floor = npix * 4 * C * es / STREAM_RATE * 1e6          # the same bytes in both directions
                print(f"{C:3d} ch @ {H}^2 bs{N} {name} | same bits {same} | floor {floor:5.1f} us | fwd one launch {m['fused_fwd']:6.1f} us  "
                      f"three {m['three_fwd']:6.1f} us = {m['three_fwd'] / m['fused_fwd']:5.2f}x | bwd one launch {m['fused_bwd']:6.1f} us  "
                      f"three {m['three_bwd']:6.1f} us = {m['three_bwd'] / m['fused_bwd']:5.2f}x", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spp_bench: needs a GPU (a CPU run cannot give a time)")
    main(opt.inner)
