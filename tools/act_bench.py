#!/usr/bin/env python3
"""Micro-benchmark of the Conv activations at the C3 positions of the benchmarked model (bs 16, 640 x 640): C = 64 @ 160^2, 128 @ 80^2,
256 @ 40^2 and 512 @ 20^2, bf16 and f32.

Per shape and dtype:
  apply     ydl_bn_act_fwd under YDL_ACT_SILU (the comparison: same bytes, the floor already measured in this code base), and under
            LEAKY (slope 0.1, through ydl_bn_act_fwd_p), HSWISH and MISH
  backward  ydl_bn_act_bwd_sums (reduce + apply, replica sums) under the same four codes
  acon      ydl_acon_fwd and ydl_acon_bwd (dz + the three per-channel sums + the fold launch)
  max2      ydl_max2_fwd and ydl_max2_bwd (both gradients written): FReLU's merge
  eager     torch on the same tensors: act(y * scale + shift) for the four point-wise activations, AconC's formula, torch.maximum

Device events; 10 warm-up runs and 40 timed runs per variant, each run ``--inner`` launches between two events, variants alternated run
by run.  Reported per variant: the median run in us and the quartile spread (q3 - q1) / median; the SiLU launch is timed twice in the
same alternation (``silu`` / ``silu2``) so that the difference of two medians of the SAME code is visible beside the others.  The
algorithmic bytes (apply and the forward layers: one tensor read + one written, max2 two read; backward: y and dout read, dy written; acon
backward: z and dout read, dz written; max2 backward: a, b, dout read, da, db written) over the time give the share of the HBM peak
(8.0 TB/s, MI355X_MICROARCH.md; a streaming copy reaches about 6.3 TB/s).

    python tools/act_bench.py [--inner 10]          (dev tool; one line per shape, dtype and group)"""
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
SLOPE = 0.1
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
CODES = (("silu", L.ACT_SILU), ("leaky", L.ACT_LEAKY), ("hswish", L.ACT_HSWISH), ("mish", L.ACT_MISH))


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3          # us


def measure(variants, inner):
    """-> {name: (median us, (q3 - q1) / median)}"""
    for fn in variants.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    t = {n: [] for n in variants}
    for _ in range(RUNS):
        for n, fn in variants.items():
            t[n].append(timed(fn, inner))
    out = {}
    for n, v in t.items():
        q = statistics.quantiles(v, n=4)
        out[n] = (statistics.median(v), (q[2] - q[0]) / statistics.median(v))
    return out


def line(head, group, m, nbytes):
    cells = []
    for n, (us, sp) in m.items():
        bw = "" if nbytes.get(n) is None else f" {100 * nbytes[n] / (us * 1e-6) / HBM_PEAK:4.1f}%"
        cells.append(f"{n} {us:7.1f} us +-{100 * sp:4.1f}%{bw}")
    print(f"{head} | {group:8s} | " + " | ".join(cells), flush=True)


def act_call(name, code, k, *args):
    if code == L.ACT_LEAKY:
        return lambda: L.call(name + "_p", *args[:k + 1], SLOPE, *args[k + 1:])
    return lambda: L.call(name, *args)


def point(N, S, C, dname, inner):
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dt, tdt, es = (L.YDL_BF16, torch.bfloat16, 2) if dname == "bf16" else (L.YDL_F32, torch.float32, 4)
    npix = N * S * S
    gen = torch.Generator(device=dev).manual_seed(1)
    y = (torch.randn(npix, C, device=dev, generator=gen) * 1.5 + 0.5).to(tdt)
    dout = torch.randn(npix, C, device=dev, generator=gen).to(tdt)
    b = torch.randn(npix, C, device=dev, generator=gen).to(tdt)
    out, dy, da, db = (torch.empty(npix, C, device=dev, dtype=tdt) for _ in range(4))
    mean = y.float().mean(0)
    invstd = 1.0 / torch.sqrt(y.float().var(0, unbiased=False) + 1e-3)
    scale = (torch.rand(C, device=dev, generator=gen) + 0.5) * invstd
    shift = torch.rand(C, device=dev, generator=gen) * 0.6 - 0.3
    p1, p2 = torch.randn(C, device=dev, generator=gen), torch.randn(C, device=dev, generator=gen)
    beta = torch.rand(C, device=dev, generator=gen) + 0.5
    dg, dbt, g1, g2, g3 = (torch.zeros(C, device=dev) for _ in range(5))
    sums = torch.zeros(L.BN_REPLICAS * 2 * C, device=dev)
    ws = torch.empty(max(L.lib().ydl_acon_bwd_ws_bytes(npix, S * S, 0, C) // 4, 4), device=dev)
    T = float(npix) * C * es
    head = f"{C:4d} ch {S:3d}^2 bs{N} {dname:4s} {T / 1e6:6.1f} MB/tensor"

    apply_v, bwd_v, eager_v = {}, {}, {}
    for n, code in CODES + (("silu2", L.ACT_SILU),):
        apply_v[n] = act_call("ydl_bn_act_fwd", code, 8, dt, P(y), C, P(scale), P(shift), None, 0, L.RES_NONE, code, P(out), C, npix, C, st)
        bwd_v[n] = act_call("ydl_bn_act_bwd_sums", code, 12, dt, P(y), C, P(dout), C, None, 0, P(mean), P(invstd), P(scale), P(shift),
                            L.RES_NONE, code, P(dy), C, None, 0, P(dg), P(dbt), 0, P(sums), npix, C, C, st)
    line(head, "apply", measure(apply_v, inner), {n: 2 * T for n in apply_v})
    line(head, "backward", measure(bwd_v, inner), {n: 3 * T for n in bwd_v})
    layers = {"acon_fwd": lambda: L.call("ydl_acon_fwd", dt, P(y), C, P(p1), P(p2), P(beta), 0, P(out), C, npix, S * S, C, C, st),
              "acon_bwd": lambda: L.call("ydl_acon_bwd", dt, P(y), C, P(dout), C, P(p1), P(p2), P(beta), 0, P(dy), C, 0, P(g1), P(g2), P(g3), 0,
                                         P(ws), npix, S * S, C, C, st),
              "max2_fwd": lambda: L.call("ydl_max2_fwd", dt, P(y), C, P(b), C, P(out), C, npix, C, st),
              "max2_bwd": lambda: L.call("ydl_max2_bwd", dt, P(y), C, P(b), C, P(dout), C, P(da), C, 0, P(db), C, 0, npix, C, st)}
    line(head, "layers", measure(layers, inner), {"acon_fwd": 2 * T, "acon_bwd": 3 * T, "max2_fwd": 3 * T, "max2_bwd": 5 * T})
    sc, sf = scale.to(tdt), shift.to(tdt)
    q1, q2, bt = p1.to(tdt), p2.to(tdt), beta.to(tdt)

    def acon_eager():
        d = (q1 - q2) * y
        return d * torch.sigmoid(bt * d) + q2 * y
    eager_v = {"silu": lambda: F.silu(y * sc + sf), "leaky": lambda: F.leaky_relu(y * sc + sf, SLOPE), "hswish": lambda: F.hardswish(y * sc + sf),
               "mish": lambda: F.mish(y * sc + sf), "acon": acon_eager, "max2": lambda: torch.maximum(y, b)}
    line(head, "eager", measure(eager_v, inner), {})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", default="", help="comma list of dtypes (bf16,f32)")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("act_bench: needs a GPU (a CPU run cannot give a time)")
    dts = [d for d in ("bf16", "f32") if not opt.only or d in opt.only.split(",")]
    for dname in dts:
        for C, S in ((64, 160), (128, 80), (256, 40), (512, 20)):
            point(16, S, C, dname, opt.inner)
