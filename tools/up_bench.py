#!/usr/bin/env python3
"""Micro-benchmark of the decoder up-samplers at the decoder shapes of BASELINE config 2 (bs 16): 256 ch 20^2 -> 40^2, 128 ch 40^2 -> 80^2,
64 ch 80^2 -> 160^2, bf16 and f32.  One line per shape, dtype and operation:

  bicubic   ydl_bicubic_fwd / ydl_bicubic_bwd (align_corners False) against the bilinear kernels (ydl_resize_* mode 1) at the same shape (the same bytes: the ratio is
            the VALU cost), against F.interpolate(mode='bicubic') and its autograd on the device (channels_last), and against the byte
            floor (input + output once over the streaming rate)
  tconv     nn.ConvTranspose2d(C, C, k, 2, p) for k = 2 and k = 4 on the mirrored entry points: forward (ydl_conv_dgrad) and the bias pass
            (ydl_bn_act_fwd in place) separately, input gradient (ydl_conv_fwd), weight gradient (ydl_conv_wgrad); against
            F.conv_transpose2d / aten.convolution_backward (channels_last, the same dtype) and against the launches it replaces: nearest
            Upsample (ydl_resize_fwd mode 0) + a 1x1 convolution C -> C on the up-sampled map
  dwtconv   ydl_dwtconv_fwd / _dgrad / _wgrad for k = 4 against F.conv_transpose2d(groups=C) and its backward, and the byte floor

Device events; 10 warm-up runs and 30 timed runs per variant, each run ``--inner`` launches between two events ended by a device
synchronise, variants alternated run by run; the median run is reported.  The first variant of a line is timed twice in the same
alternation: ``spread`` is the relative difference of its two medians.  Byte floors use 6.3 TB/s, the rate a streaming copy reaches
(DESIGN.md).

    python tools/up_bench.py [--inner 10] [--only bf16] [--ops bicubic,tconv,dwtconv]"""
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

WARMUP, RUNS = 10, 30
STREAM_RATE = 6.3e12
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
    first = next(iter(variants))
    variants = dict(variants, again=variants[first])
    for fn in variants.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    t = {n: [] for n in variants}
    for _ in range(RUNS):
        for n, fn in variants.items():
            t[n].append(timed(fn, inner))
    m = {n: statistics.median(v) for n, v in t.items()}
    m["spread"] = abs(m[first] - m.pop("again")) / m[first]
    return m


def line(head, op, m, floor_us=None):
    names = [n for n in m if n != "spread"]
    first = names[0]
    txt = f"{head} | {op:10s} " + "  ".join(f"{n} {m[n]:7.1f} us" + ("" if n == first else f" ({m[n] / m[first]:4.2f}x)") for n in names)
    txt += f"  spread {100 * m['spread']:4.1f} %"
    if floor_us is not None:
        txt += f"  byte floor {floor_us:6.1f} us ({m[first] / floor_us:4.2f}x)"
    print(txt, flush=True)


def bench(N, C, S, dname, inner, ops=("bicubic", "tconv", "dwtconv")):
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dt, tdt, es = (L.YDL_BF16, torch.bfloat16, 2) if dname == "bf16" else (L.YDL_F32, torch.float32, 4)
    lib = L.lib()
    H = W = S
    npi, npo = N * H * W, N * 4 * H * W
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(npi, C, device=dev, generator=gen).to(tdt)
    dy = torch.randn(npo, C, device=dev, generator=gen).to(tdt)
    y = torch.empty(npo, C, device=dev, dtype=tdt)
    dx = torch.empty(npi, C, device=dev, dtype=tdt)
    head = f"{C:3d} ch {S}^2->{2 * S}^2 bs{N} {dname:4s}"
    floor = (npi + npo) * C * es / STREAM_RATE * 1e6
    xt = x.view(N, H, W, C).permute(0, 3, 1, 2).requires_grad_(True)         # channels_last views for the vendor paths
    dyt = dy.view(N, 2 * H, 2 * W, C).permute(0, 3, 1, 2)

    # ---- bicubic against bilinear and F.interpolate
    def rs(name, mode):
        f, b, arg = ("ydl_bicubic_fwd", "ydl_bicubic_bwd", 0) if mode == L.RESIZE_BICUBIC else ("ydl_resize_fwd", "ydl_resize_bwd", mode)
        if name == "fwd":
            return lambda: L.call(f, dt, arg, P(x), C, P(y), C, N, H, W, 2 * H, 2 * W, C, 0.5, 0.5, st)
        return lambda: L.call(b, dt, arg, P(dy), C, P(dx), C, 0, N, H, W, 2 * H, 2 * W, C, 0.5, 0.5, st)
    yt = F.interpolate(xt, scale_factor=2, mode="bicubic", align_corners=False) if "bicubic" in ops else None
    if "bicubic" in ops:
        line(head, "bicubic fwd", medians({"bicubic": rs("fwd", 3), "bilinear": rs("fwd", 1),
                                           "torch": lambda: F.interpolate(xt.detach(), scale_factor=2, mode="bicubic", align_corners=False)}, inner), floor)
        line(head, "bicubic bwd", medians({"bicubic": rs("bwd", 3), "bilinear": rs("bwd", 1),
                                           "torch": lambda: torch.autograd.grad(yt, xt, dyt, retain_graph=True)}, inner), floor)
    del yt

    # ---- dense transposed convolution, k = 2 and k = 4
    conv_bwd = torch.ops.aten.convolution_backward
    for k, p in ((2, 0), (4, 1)) if "tconv" in ops else ():
        master = torch.randn(C, k * k, C, device=dev, generator=gen) / (((k + 1) // 2) ** 2 * C) ** 0.5
        w = torch.empty(C, k * k, C, device=dev, dtype=tdt)
        wt = torch.empty(C, k * k, C, device=dev, dtype=tdt)
        L.call("ydl_weight_prep", dt, P(master), P(w), P(wt), C, k * k, C, st)
        geom = L.ConvGeom(N, 2 * H, 2 * W, C, H, W, C, k, 2, p, C, C, 0)
        gp = ctypes.byref(geom)
        ones, bias = torch.ones(C, device=dev), torch.randn(C, device=dev, generator=gen)
        dw = torch.zeros(C, k * k, C, device=dev)
        wtorch = w.view(C, k, k, C).permute(0, 3, 1, 2)                      # [c1][c2][k][k], channels_last storage
        bt = bias.to(tdt)
        # what it replaces: nearest x2 + 1x1 convolution at the output size
        m1 = torch.randn(C, 1, C, device=dev, generator=gen) / C ** 0.5
        w1, w1t = torch.empty(C, 1, C, device=dev, dtype=tdt), torch.empty(C, 1, C, device=dev, dtype=tdt)
        L.call("ydl_weight_prep", dt, P(m1), P(w1), P(w1t), C, 1, C, st)
        g1 = L.ConvGeom(N, 2 * H, 2 * W, C, 2 * H, 2 * W, C, 1, 1, 0, C, C, 0)
        g1p = ctypes.byref(g1)
        up = torch.empty(npo, C, device=dev, dtype=tdt)

        def replaced():
            L.call("ydl_resize_fwd", dt, 0, P(x), C, P(up), C, N, H, W, 2 * H, 2 * W, C, 0.5, 0.5, st)
            L.call("ydl_conv_fwd", g1p, dt, P(up), P(w1), P(y), None, 0, st)

        def fwd_bias():
            L.call("ydl_conv_dgrad", gp, dt, P(x), P(wt), P(y), 0, st)
            L.call("ydl_bn_act_fwd", dt, P(y), C, P(ones), P(bias), None, 0, L.RES_NONE, L.ACT_NONE, P(y), C, npo, C, st)
        tk = dict(stride=2, padding=p)

        def t_bwd(mask):
            return lambda: conv_bwd(dyt, xt.detach(), wtorch, None, (2, 2), (p, p), (1, 1), True, (0, 0), 1, mask)
        tag = f"tconv k{k}"
        line(head, tag + " fwd", medians({"fwd+bias": fwd_bias, "fwd": lambda: L.call("ydl_conv_dgrad", gp, dt, P(x), P(wt), P(y), 0, st),
                                          "bias": lambda: L.call("ydl_bn_act_fwd", dt, P(y), C, P(ones), P(bias), None, 0, L.RES_NONE, L.ACT_NONE,
                                                                 P(y), C, npo, C, st),
                                          "torch": lambda: F.conv_transpose2d(xt.detach(), wtorch, bt, **tk), "nearest+1x1": replaced}, inner))
        line(head, tag + " dx", medians({"dx": lambda: L.call("ydl_conv_fwd", gp, dt, P(dy), P(w), P(dx), None, 0, st),
                                         "torch": t_bwd((True, False, False))}, inner))
        line(head, tag + " dW", medians({"dW": lambda: L.call("ydl_conv_wgrad", gp, dt, P(dy), P(x), P(dw), st),
                                         "torch": t_bwd((False, True, False))}, inner))

    # ---- depth-wise transposed convolution, k = 4
    if "dwtconv" not in ops:
        return
    k, p, op = 4, 1, 0
    wm = torch.randn(C, k * k, device=dev, generator=gen) / 2
    bias = torch.randn(C, device=dev, generator=gen)
    dwg = torch.zeros(C, k * k, device=dev)
    ws = torch.empty(lib.ydl_dwtconv_wgrad_ws_bytes(C, k) // 4, device=dev)
    wd = wm.view(C, 1, k, k).to(tdt)
    bt = bias.to(tdt)
    tk = dict(stride=2, padding=p, groups=C)

    def d_bwd(mask):
        return lambda: conv_bwd(dyt, xt.detach(), wd, None, (2, 2), (p, p), (1, 1), True, (0, 0), C, mask)
    line(head, "dwtconv fwd", medians({"fwd": lambda: L.call("ydl_dwtconv_fwd", dt, P(x), C, P(wm), P(bias), P(y), C, N, H, W, C, k, p, op, st),
                                       "torch": lambda: F.conv_transpose2d(xt.detach(), wd, bt, **tk)}, inner), floor)
    line(head, "dwtconv dx", medians({"dx": lambda: L.call("ydl_dwtconv_dgrad", dt, P(dy), C, P(wm), P(dx), C, 0, N, H, W, C, k, p, op, st),
                                      "torch": d_bwd((True, False, False))}, inner), floor)
    line(head, "dwtconv dW", medians({"dW": lambda: L.call("ydl_dwtconv_wgrad", dt, P(x), C, P(dy), C, P(dwg), P(ws), N, H, W, C, k, p, op, st),
                                      "torch": d_bwd((False, True, False))}, inner), floor)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", default="", help="comma list of dtypes (bf16,f32)")
    ap.add_argument("--ops", default="bicubic,tconv,dwtconv", help="comma list of operations")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("up_bench: needs a GPU (a CPU run cannot give a time)")
    for dname in [d for d in ("bf16", "f32") if not opt.only or d in opt.only.split(",")]:
        for C, S in ((256, 20), (128, 40), (64, 80)):
            bench(16, C, S, dname, opt.inner, tuple(opt.ops.split(",")))
