#!/usr/bin/env python3
"""Micro-benchmark of the cross-convolution kernels (ydl_xconv_fwd / _dgrad / _wgrad) at the C3 positions of the benchmarked model
(bs 16, 640 x 640): k = 3, s = 1, both axes, bf16 and f32, C -> C for C = 64 @ 160^2, 128 @ 80^2, 256 @ 40^2 and 512 @ 20^2, plus the
stride-2 pair of CrossConv(128, 128, 3, 2) on a 160^2 map ((1,3)/(1,2): 160x160 -> 160x80, then (3,1)/(2,1): 160x80 -> 80x80).

Per shape and direction three variants:
  x       the new launch (the weight gradient: its partial-tile launch + the fixed-order merge; the forward writes statistics rows)
  embed   the same layer as a 3x3 whose other six taps are zero, through ydl_conv_fwd (with statistics rows) / ydl_conv_dgrad /
          ydl_conv_wgrad_det: what the library could do before; stride 1 only (a stride of (1, s) is no square stride)
  vendor  F.conv2d / aten.convolution_backward on channels_last tensors ("n/a" if it refuses)
Before timing, ``x`` and ``embed`` are each compared with a float64 convolution of the same operands on the device at EVERY point,
within the bound of tests/test_gpu_xconv_kernels.py (2*K*2^-24*S + 2^-8 |ref| for a bf16 store; 2*n*2^-24*S for the weight gradient, S
the same convolution of absolute values; ``embed`` sums 3*K terms, two thirds of them zero).

Device events; 10 warm-up runs and 40 timed runs per variant, each run ``--inner`` launches between two events, variants alternated run
by run; the median run is reported.  ``x`` is timed twice in the same alternation: ``spread`` is the relative difference of its two
medians.  For ``x`` the algorithmic bytes (x once + y once at the storage dtype; the weight gradient reads x and dy once) over its time
are given as a share of the HBM peak (8.0 TB/s, MI355X_MICROARCH.md; about 6.3 TB/s is what a streaming copy reaches).

    python tools/xconv_bench.py [--inner 10]          (dev tool; one line per point and direction)"""
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
HBM_PEAK = 8.0e12
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


def ref64(x4, w3, dy4, axis, k, s, p):
    """float64 on the device, NHWC: a cross convolution is k shifted matrix products.  -> (y, dx, dw [Cout][k][Cin])"""
    N, H, W, Cin = x4.shape
    Ho, Wo, Cout = dy4.shape[1], dy4.shape[2], dy4.shape[3]
    dim = 2 if axis == L.AXIS_W else 1
    pad = (0, 0, p, p) if axis == L.AXIS_W else (0, 0, 0, 0, p, p)
    xp = F.pad(x4, pad)
    dxp = torch.zeros_like(xp)
    Lo = Wo if axis == L.AXIS_W else Ho
    y = torch.zeros_like(dy4)
    dw = torch.zeros(Cout, k, Cin, dtype=torch.float64, device=x4.device)
    for t in range(k):
        idx = [slice(None)] * 4
        idx[dim] = slice(t, t + (Lo - 1) * s + 1, s)
        xs = xp[tuple(idx)]
        y += xs @ w3[:, t, :].t()
        dxp[tuple(idx)] += dy4 @ w3[:, t, :]
        dw[:, t, :] = dy4.reshape(-1, Cout).t() @ xs.reshape(-1, Cin)
    idx = [slice(None)] * 4
    idx[dim] = slice(p, p + (W if axis == L.AXIS_W else H))
    return y, dxp[tuple(idx)], dw


def point(N, H, W, Cin, Cout, axis, k, s, dname, inner):
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dt, tdt, es = (L.YDL_BF16, torch.bfloat16, 2) if dname == "bf16" else (L.YDL_F32, torch.float32, 4)
    lib = L.lib()
    p = k // 2
    Ho = (H + 2 * p - k) // s + 1 if axis == L.AXIS_H else H
    Wo = (W + 2 * p - k) // s + 1 if axis == L.AXIS_W else W
    ks, ss, ps = ((1, k), (1, s), (0, p)) if axis == L.AXIS_W else ((k, 1), (s, 1), (p, 0))
    npi, npo = N * H * W, N * Ho * Wo
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(npi, Cin, device=dev, generator=gen).to(tdt)
    dy = torch.randn(npo, Cout, device=dev, generator=gen).to(tdt)
    master = torch.randn(Cout, k, Cin, device=dev, generator=gen) / (k * Cin) ** 0.5
    w = torch.empty(Cout, k, Cin, device=dev, dtype=tdt)
    wt = torch.empty(Cin, k, Cout, device=dev, dtype=tdt)
    L.call("ydl_weight_prep", dt, P(master), P(w), P(wt), Cout, k, Cin, st)
    y1 = torch.empty(npo, Cout, device=dev, dtype=tdt)
    dx1 = torch.empty(npi, Cin, device=dev, dtype=tdt)
    dw1 = torch.zeros(Cout, k, Cin, device=dev)
    geom = L.ConvGeom(N, H, W, Cin, Ho, Wo, Cout, k, s, p, Cin, Cout, 0)
    gp = ctypes.byref(geom)
    assert lib.ydl_xconv_supported(gp, axis, dt), lib.ydl_last_error()
    ws1 = torch.empty(max(lib.ydl_xconv_wgrad_ws_bytes(gp, axis, dt) // 4, 4), device=dev)
    stats = torch.empty(lib.ydl_xconv_fwd_stats_ws_bytes(gp, axis, dt) // 4, device=dev)
    xv = {"fwd": lambda: L.call("ydl_xconv_fwd", gp, axis, dt, P(x), P(w), P(y1), P(stats), st),
          "dgrad": lambda: L.call("ydl_xconv_dgrad", gp, axis, dt, P(dy), P(wt), P(dx1), 0, st),
          "wgrad": lambda: L.call("ydl_xconv_wgrad", gp, axis, dt, P(x), P(dy), P(dw1), P(ws1), st)}
    # the zero-embedded 3x3 on the square entry points (stride 1, k = 3)
    embed = None
    if s == 1 and k == 3:
        taps = [3, 4, 5] if axis == L.AXIS_W else [1, 4, 7]
        m9 = torch.zeros(Cout, 9, Cin, device=dev)
        m9[:, taps, :] = master
        w9 = torch.empty(Cout, 9, Cin, device=dev, dtype=tdt)
        wt9 = torch.empty(Cin, 9, Cout, device=dev, dtype=tdt)
        L.call("ydl_weight_prep", dt, P(m9), P(w9), P(wt9), Cout, 9, Cin, st)
        y2 = torch.empty(npo, Cout, device=dev, dtype=tdt)
        dx2 = torch.empty(npi, Cin, device=dev, dtype=tdt)
        dw2 = torch.zeros(Cout, 9, Cin, device=dev)
        sq = L.ConvGeom(N, H, W, Cin, H, W, Cout, 3, 1, 1, Cin, Cout, 0)
        sp = ctypes.byref(sq)
        ws2 = torch.empty(max(lib.ydl_conv_wgrad_ws_bytes(sp, dt) // 4, 4), device=dev)
        stats2 = torch.empty(max(lib.ydl_conv_fwd_stats_ws_bytes(sp, dt) // 4, 4), device=dev)
        embed = {"fwd": lambda: L.call("ydl_conv_fwd", sp, dt, P(x), P(w9), P(y2), P(stats2), 0, st),
                 "dgrad": lambda: L.call("ydl_conv_dgrad", sp, dt, P(dy), P(wt9), P(dx2), 0, st),
                 "wgrad": lambda: L.call("ydl_conv_wgrad_det", sp, dt, P(x), P(dy), P(dw2), P(ws2), st)}
    # vendor, channels_last
    xt = x.view(N, H, W, Cin).permute(0, 3, 1, 2)
    dyt = dy.view(N, Ho, Wo, Cout).permute(0, 3, 1, 2)
    wtorch = w.view(Cout, *ks, Cin).permute(0, 3, 1, 2)
    conv_bwd = torch.ops.aten.convolution_backward

    def t_bwd(mask):
        return lambda: conv_bwd(dyt, xt, wtorch, None, ss, ps, (1, 1), False, (0, 0), 1, mask)
    ven = {"fwd": lambda: F.conv2d(xt, wtorch, None, ss, ps), "dgrad": t_bwd((True, False, False)), "wgrad": t_bwd((False, True, False))}

    # agreement with float64 at every point, once
    for d in ("fwd", "dgrad", "wgrad"):
        xv[d]()
        if embed:
            embed[d]()
    torch.cuda.synchronize()
    seps = 2.0 ** -8 if dname == "bf16" else 0.0
    x4, dy4, w3 = x.view(N, H, W, Cin).double(), dy.view(N, Ho, Wo, Cout).double(), w.double()
    r, ra = ref64(x4, w3, dy4, axis, k, s, p), ref64(x4.abs(), w3.abs(), dy4.abs(), axis, k, s, p)
    ref = {"fwd": (r[0], ra[0], k * Cin, seps), "dgrad": (r[1], ra[1], k * Cout, seps), "wgrad": (r[2], ra[2], npo, 0.0)}
    got = {"fwd": y1.view(N, Ho, Wo, Cout), "dgrad": dx1.view(N, H, W, Cin), "wgrad": dw1}
    if embed:
        got2 = {"fwd": y2.view(N, H, W, Cout), "dgrad": dx2.view(N, H, W, Cin), "wgrad": dw2[:, taps, :]}
    worst = {}
    for d, (r, sabs, terms, se) in ref.items():
        bound = (2 * terms * 2.0 ** -24 * sabs + se * r.abs()).clamp_min(1e-30)
        worst[d] = float(((got[d].double() - r).abs() / bound).max())
        assert worst[d] <= 1.0, (d, "x", worst[d])
        if embed:
            bound2 = (2 * 3 * terms * 2.0 ** -24 * sabs + se * r.abs()).clamp_min(1e-30) if d != "wgrad" else bound
            e2 = float(((got2[d].double() - r).abs() / bound2).max())
            assert e2 <= 1.0, (d, "embed", e2)
    del x4, dy4, w3, r, ra, ref
    dw1.zero_()

    gflop = 2.0 * npo * Cout * k * Cin / 1e9
    head = f"{Cin:4d}->{Cout:3d} {'1x' + str(k) if axis == L.AXIS_W else str(k) + 'x1'} s{s} {H}x{W} bs{N} {dname:4s} {gflop:5.2f} GFLOP"
    for d in ("fwd", "dgrad", "wgrad"):
        variants = {"x": xv[d], "x2": xv[d]}
        if embed:
            variants["embed"] = embed[d]
        try:
            ven[d]()
            torch.cuda.synchronize()
            variants["vendor"] = ven[d]
        except Exception:
            pass
        m = medians(variants, inner)
        nbytes = (npi * Cin + npo * Cout) * es
        tx = min(m["x"], m["x2"])
        spread = abs(m["x"] - m["x2"]) / tx
        te = f"{m['embed']:7.1f} ({m['embed'] / m['x']:4.2f}x)" if embed else "    n/a        "
        tv = f"{m['vendor']:7.1f} ({m['vendor'] / m['x']:4.2f}x)" if "vendor" in m else "    n/a        "
        print(f"{head} | {d:5s} x {m['x']:7.1f} us (again {m['x2']:7.1f}, spread {100 * spread:4.1f} %) embed {te} vendor {tv} | "
              f"{nbytes / 1e6:6.1f} MB, {nbytes / (m['x'] * 1e-6) / 1e12:4.2f} TB/s = {100 * nbytes / (m['x'] * 1e-6) / HBM_PEAK:4.1f} % of HBM peak | "
              f"err/bound {worst[d]:.3f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", default="", help="comma list of dtypes (bf16,f32)")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xconv_bench: needs a GPU (a CPU run cannot give a time)")
    dts = [d for d in ("bf16", "f32") if not opt.only or d in opt.only.split(",")]
    for dname in dts:
        for C, S in ((64, 160), (128, 80), (256, 40), (512, 20)):
            for axis in (L.AXIS_W, L.AXIS_H):
                point(16, S, S, C, C, axis, 3, 1, dname, opt.inner)
        point(16, 160, 160, 128, 128, L.AXIS_W, 3, 2, dname, opt.inner)
        point(16, 160, 80, 128, 128, L.AXIS_H, 3, 2, dname, opt.inner)
