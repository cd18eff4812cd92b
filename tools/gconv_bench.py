#!/usr/bin/env python3
"""Micro-benchmark of the grouped-convolution kernels (ydl_gconv_fwd / _dgrad / _wgrad) at the shapes where the reference uses
groups: the seven layers of SPPCSPC_group (models/common.py:1451-1468, all g = 4) on the stride-32 map of a 640 x 640 input, 20^2,
bs = 16, at yolov5n width (256 / 1024 / 512 -> 256 channels) and at half of it (128 / 512 / 256 -> 128), both dtypes.  The seven
layers are four distinct shapes: cv1 = cv2 = cv4 (1x1, c -> c), cv3 = cv6 (3x3, c -> c), cv5 (1x1, 4c -> c), cv7 (1x1, 2c -> c).

Per shape and direction three variants:
  one     the single launch for all groups (the weight gradient: its partial-tile launch + the fixed-order merge)
  loop    g calls of ydl_conv_fwd / ydl_conv_dgrad / ydl_conv_wgrad_det on channel slices (ldx, ldy and a contiguous weight block
          per group): what the library could do before
  torch   F.conv2d(groups=g) / aten.convolution_backward on channels_last tensors (the vendor library; "n/a" if it refuses)
and the largest difference between ``one`` and ``loop`` results (they sum in different orders; in bf16 the stores round).

Device events; 10 warm-up runs and 40 timed runs per variant, each run ``--inner`` launches between two events, variants alternated
run by run; the median run is reported.

    python tools/gconv_bench.py [--inner 10]          (dev tool; one line per point)"""
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


def point(label, N, H, Cin, Cout, G, k, dname, inner):
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dt, tdt, es = (L.YDL_BF16, torch.bfloat16, 2) if dname == "bf16" else (L.YDL_F32, torch.float32, 4)
    lib = L.lib()
    npix, kk, Cig, Cog, p = N * H * H, k * k, Cin // G, Cout // G, k // 2
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(npix, Cin, device=dev, generator=gen).to(tdt)
    dy = torch.randn(npix, Cout, device=dev, generator=gen).to(tdt)
    master = torch.randn(Cout, kk, Cig, device=dev, generator=gen) / (kk * Cig) ** 0.5
    w = torch.empty(Cout, kk, Cig, device=dev, dtype=tdt)
    wt = torch.empty(Cin, kk, Cog, device=dev, dtype=tdt)
    L.call("ydl_gconv_weight_prep", dt, P(master), P(w), P(wt), Cout, kk, Cin, G, st)
    y1, y2 = torch.empty(npix, Cout, device=dev, dtype=tdt), torch.empty(npix, Cout, device=dev, dtype=tdt)
    dx1, dx2 = torch.empty(npix, Cin, device=dev, dtype=tdt), torch.empty(npix, Cin, device=dev, dtype=tdt)
    dw1, dw2 = torch.zeros(Cout, kk, Cig, device=dev), torch.zeros(Cout, kk, Cig, device=dev)
    geom = L.ConvGeom(N, H, H, Cin, H, H, Cout, k, 1, p, Cin, Cout, 0)
    gp = ctypes.byref(geom)
    assert lib.ydl_gconv_supported(gp, G, dt)
    ws1 = torch.empty(max(lib.ydl_gconv_wgrad_ws_bytes(gp, G, dt) // 4, 4), device=dev)
    stats = torch.empty(lib.ydl_gconv_fwd_stats_ws_bytes(gp, G, dt) // 4, device=dev)
    # the per-group loop on the groups = 1 entry points
    sub = L.ConvGeom(N, H, H, Cig, H, H, Cog, k, 1, p, Cin, Cout, 0)
    sp = ctypes.byref(sub)
    ws2 = torch.empty(max(lib.ydl_conv_wgrad_ws_bytes(sp, dt) // 4, 4), device=dev)
    stats2 = torch.empty(max(lib.ydl_conv_fwd_stats_ws_bytes(sp, dt) // 4, 4), device=dev)

    def off(t, elems, size):
        return ctypes.c_void_p(t.data_ptr() + elems * size)

    def loop_fwd():
        for g in range(G):
            L.call("ydl_conv_fwd", sp, dt, off(x, g * Cig, es), off(w, g * Cog * kk * Cig, es), off(y2, g * Cog, es), P(stats2), 0, st)

    def loop_dgrad():
        for g in range(G):
            L.call("ydl_conv_dgrad", sp, dt, off(dy, g * Cog, es), off(wt, g * Cig * kk * Cog, es), off(dx2, g * Cig, es), 0, st)

    def loop_wgrad():
        for g in range(G):
            L.call("ydl_conv_wgrad_det", sp, dt, off(x, g * Cig, es), off(dy, g * Cog, es), off(dw2, g * Cog * kk * Cig, 4), P(ws2), st)

    one = {"fwd": lambda: L.call("ydl_gconv_fwd", gp, G, dt, P(x), P(w), P(y1), P(stats), st),
           "dgrad": lambda: L.call("ydl_gconv_dgrad", gp, G, dt, P(dy), P(wt), P(dx1), 0, st),
           "wgrad": lambda: L.call("ydl_gconv_wgrad", gp, G, dt, P(x), P(dy), P(dw1), P(ws1), st)}
    loop = {"fwd": loop_fwd, "dgrad": loop_dgrad, "wgrad": loop_wgrad}
    # torch, channels_last
    xt = x.view(N, H, H, Cin).permute(0, 3, 1, 2)
    dyt = dy.view(N, H, H, Cout).permute(0, 3, 1, 2)
    wtorch = w.view(Cout, k, k, Cig).permute(0, 3, 1, 2)
    conv_bwd = torch.ops.aten.convolution_backward

    def t_bwd(mask):
        return lambda: conv_bwd(dyt, xt, wtorch, None, (1, 1), (p, p), (1, 1), False, (0, 0), G, mask)
    tor = {"fwd": lambda: F.conv2d(xt, wtorch, None, 1, p, 1, G), "dgrad": t_bwd((True, False, False)), "wgrad": t_bwd((False, True, False))}
    # agreement of the two own paths, once
    for d in ("fwd", "dgrad", "wgrad"):
        one[d]()
        loop[d]()
    torch.cuda.synchronize()
    diff = {"fwd": float((y1.float() - y2.float()).abs().max()), "dgrad": float((dx1.float() - dx2.float()).abs().max()),
            "wgrad": float((dw1 - dw2).abs().max() / dw2.abs().max())}
    out = []
    for d in ("fwd", "dgrad", "wgrad"):
        variants = {"one": one[d], "loop": loop[d]}
        try:
            tor[d]()
            torch.cuda.synchronize()
            variants["torch"] = tor[d]
        except Exception:
            pass
        m = medians(variants, inner)
        tt = f"{m['torch']:6.1f}" if "torch" in m else "   n/a"
        out.append(f"{d} one {m['one']:6.1f} loop {m['loop']:6.1f} ({m['loop'] / m['one']:4.2f}x) torch {tt} us, diff {diff[d]:.1e}")
    gflop = 2.0 * npix * Cout * kk * Cig / 1e9
    print(f"{label:11s} {Cin:4d}->{Cout:3d} k{k} g{G} @ {H}^2 bs{N} {dname:4s} {gflop:5.2f} GFLOP | " + " | ".join(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gconv_bench: needs a GPU (a CPU run cannot give a time)")
    for c in (256, 128):
        for label, cin, k in (("cv1/cv2/cv4", c, 1), ("cv3/cv6", c, 3), ("cv5", 4 * c, 1), ("cv7", 2 * c, 1)):
            for dname in ("bf16", "f32"):
                point(label, 16, 20, cin, c, 4, k, dname, opt.inner)
