#!/usr/bin/env python3
"""Micro-benchmark of the ConvNeXt kernels (csrc/convnext.hip) at the shapes of a 640^2 batch of 16, bf16 and f32:
96 ch @ 160^2, 192 @ 80^2, 384 @ 40^2, 768 @ 20^2 (bias + GELU at the hidden width 4 C).

One line per kernel, direction, shape and dtype with
  (a) the byte floor: the tensors the pass must read and write, each once, over 6.3 TB/s, the rate a streaming copy reaches:
      LayerNorm fwd x + y, bwd x + dy + dx; GELU fwd z + y, bwd z + dy + dz; residual fwd y + x + out, bwd dout + y + dy (dx aliased);
  (b) torch's own op on the same GPU and the same NHWC memory: F.layer_norm over the last dimension, F.gelu(z + b), torch.addcmul,
      their backward through torch.autograd.grad on a retained graph.
Then (c): one CNBlock training step (forward + backward) of this package against the plain-torch module of tests/convnext_ref.py on the
GPU, in f32 and bf16, at 96 ch @ 160^2 and 384 ch @ 40^2.

Device events; 10 warm-up runs and 30 timed runs per variant, each run ``--inner`` launches between two events ended by a device
synchronise, variants alternated run by run; the median run is reported.  The kernel is timed twice in the same alternation:
``spread`` is the relative difference of its two medians.  Results are compared with torch's before anything is timed.

    python tools/convnext_bench.py [--inner 10] [--only bf16] [--skip-block]"""
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
SHAPES = ((96, 160), (192, 80), (384, 40), (768, 20))
N = 16
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


def report(head, dname, m, passes, npix, C, es):
    floor = passes * npix * C * es / STREAM_RATE * 1e6
    print(f"{head:26s} bs{N} {dname:4s} | kernel {m['kernel']:7.1f} us  torch {m['torch']:7.1f} us ({m['torch'] / m['kernel']:4.2f}x)  "
          f"spread {100 * m['spread']:4.1f} %  byte floor {floor:6.1f} us ({m['kernel'] / floor:4.2f}x)", flush=True)


def close(a, b, dname, what):
    tol = 2e-2 if dname == "bf16" else 1e-4
    err = float((a.float() - b.float()).abs().max()) / max(float(b.float().abs().max()), 1e-30)
    assert err < tol, (what, dname, err)


def bench_kernels(C, hw, dname, inner):
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dt, tdt, es = (L.YDL_BF16, torch.bfloat16, 2) if dname == "bf16" else (L.YDL_F32, torch.float32, 4)
    npix = N * hw * hw
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)
    lib = L.lib()
    tag = f"{C} ch @ {hw}^2"
    # ---- LayerNorm
    x, dy = rnd(npix, C).to(tdt), rnd(npix, C).to(tdt)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    gamma, beta, pb = rnd(C) * 0.2 + 1, rnd(C) * 0.2, rnd(C) * 0.2
    stats = torch.empty(npix, 2, device=dev)
    dg, db, dp = (torch.zeros(C, device=dev) for _ in range(3))
    ws = torch.empty(max(lib.ydl_ln_bwd_ws_bytes(npix, C) // 4, 4), device=dev)
    k_fwd = lambda: L.call("ydl_ln_fwd", dt, P(x), C, P(pb), P(gamma), P(beta), 1e-6, P(y), C, P(stats), npix, C, st)
    k_bwd = lambda: L.call("ydl_ln_bwd", dt, P(x), C, P(pb), P(gamma), P(stats), P(dy), C, P(dx), C, 0, P(dg), P(db), P(dp), P(ws), npix, C, st)
    xr = x.clone().requires_grad_(True)
    gt, bt, pt = (v.to(tdt).requires_grad_(True) for v in (gamma, beta, pb))
    t_fwd = lambda: F.layer_norm(xr + pt, (C,), gt, bt, 1e-6)
    yt = t_fwd()
    t_bwd = lambda: torch.autograd.grad(yt, (xr, gt, bt, pt), dy, retain_graph=True)
    k_fwd(); k_bwd()
    close(y, yt.detach(), dname, "ln fwd"); close(dx, t_bwd()[0], dname, "ln bwd")
    report("layer_norm fwd " + tag, dname, medians({"kernel": k_fwd, "torch": t_fwd}, inner), 2, npix, C, es)
    report("layer_norm bwd " + tag, dname, medians({"kernel": k_bwd, "torch": t_bwd}, inner), 3, npix, C, es)
    del x, dy, y, dx, xr, yt, stats
    # ---- bias + GELU at the hidden width
    H = 4 * C
    z, dy = rnd(npix, H).to(tdt), rnd(npix, H).to(tdt)
    y, dz = torch.empty_like(z), torch.empty_like(z)
    b = rnd(H) * 0.2
    dbias = torch.zeros(H, device=dev)
    ws = torch.empty(max(lib.ydl_bias_gelu_bwd_ws_bytes(npix, H) // 4, 4), device=dev)
    k_fwd = lambda: L.call("ydl_bias_gelu_fwd", dt, P(z), H, P(b), P(y), H, npix, H, st)
    k_bwd = lambda: L.call("ydl_bias_gelu_bwd", dt, P(z), H, P(b), P(dy), H, P(dz), H, P(dbias), P(ws), npix, H, st)
    zr, bt = z.clone().requires_grad_(True), b.to(tdt).requires_grad_(True)
    t_fwd = lambda: F.gelu(zr + bt)
    yt = t_fwd()
    t_bwd = lambda: torch.autograd.grad(yt, (zr, bt), dy, retain_graph=True)
    k_fwd(); k_bwd()
    close(y, yt.detach(), dname, "gelu fwd"); close(dz, t_bwd()[0], dname, "gelu bwd")
    report(f"bias_gelu fwd {H} ch @ {hw}^2", dname, medians({"kernel": k_fwd, "torch": t_fwd}, inner), 2, npix, H, es)
    report(f"bias_gelu bwd {H} ch @ {hw}^2", dname, medians({"kernel": k_bwd, "torch": t_bwd}, inner), 3, npix, H, es)
    del z, dy, y, dz, zr, yt
    # ---- layer-scaled residual
    x, yb, dout = rnd(npix, C).to(tdt), rnd(npix, C).to(tdt), rnd(npix, C).to(tdt)
    out, dyb = torch.empty_like(x), torch.empty_like(x)
    g = rnd(C) * 0.2 + 1
    dgam = torch.zeros(C, device=dev)
    ws = torch.empty(max(lib.ydl_scale_res_bwd_ws_bytes(N, hw * hw, C) // 4, 4), device=dev)
    k_fwd = lambda: L.call("ydl_scale_res_fwd", dt, P(yb), C, P(g), None, P(x), C, P(out), C, N, hw * hw, C, st)
    k_bwd = lambda: L.call("ydl_scale_res_bwd", dt, P(dout), C, P(yb), C, P(g), None, P(dyb), C, None, 0, 0, P(dgam), P(ws), N, hw * hw, C, st)
    yr, gt = yb.clone().requires_grad_(True), g.to(tdt).requires_grad_(True)
    t_fwd = lambda: torch.addcmul(x, yr, gt)
    ot = t_fwd()
    t_bwd = lambda: torch.autograd.grad(ot, (yr, gt), dout, retain_graph=True)
    k_fwd(); k_bwd()
    close(out, ot.detach(), dname, "scale_res fwd"); close(dyb, t_bwd()[0], dname, "scale_res bwd")
    report("scale_res fwd " + tag, dname, medians({"kernel": k_fwd, "torch": t_fwd}, inner), 3, npix, C, es)
    report("scale_res bwd " + tag, dname, medians({"kernel": k_bwd, "torch": t_bwd}, inner), 3, npix, C, es)


def bench_block(C, hw, dname, inner):
    import yolo_dual_amd as ydl
    from tests import convnext_ref as R
    ydl.set_compute_dtype(dname)
    tdt = torch.bfloat16 if dname == "bf16" else torch.float32
    torch.manual_seed(0)
    ref = R.CNBlock(C, 1.0).cuda().train()
    mod = ydl.CNBlock(C, 1.0)
    mod.load_state_dict(ref.state_dict())
    mod = mod.cuda().train()
    ref = ref.to(tdt).to(memory_format=torch.channels_last)
    x = torch.randn(N, C, hw, hw, device="cuda")
    gout = torch.randn(N, C, hw, hw, device="cuda")
    xt, gt = x.to(tdt).contiguous(memory_format=torch.channels_last), gout.to(tdt).contiguous(memory_format=torch.channels_last)

    def ours():
        xi = x.requires_grad_(True)
        mod(xi).backward(gout)

    def theirs():
        xi = xt.requires_grad_(True)
        ref(xi).backward(gt)
    m = medians({"kernel": ours, "torch": theirs}, max(inner // 5, 1))
    print(f"CNBlock step {C} ch @ {hw}^2      bs{N} {dname:4s} | this {m['kernel'] / 1e3:7.2f} ms  plain torch {m['torch'] / 1e3:7.2f} ms "
          f"({m['torch'] / m['kernel']:4.2f}x)  spread {100 * m['spread']:4.1f} %  (ours includes the NCHW f32 edge conversions)", flush=True)
    ydl.set_compute_dtype("bf16")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", default="", help="comma list of dtypes (bf16,f32)")
    ap.add_argument("--skip-block", action="store_true")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convnext_bench: needs a GPU (a CPU run cannot give a time)")
    dnames = [d for d in ("bf16", "f32") if not opt.only or d in opt.only.split(",")]
    for dname in dnames:
        for C, hw in SHAPES:
            bench_kernels(C, hw, dname, opt.inner)
    if not opt.skip_block:
        for dname in dnames:
            for C, hw in ((96, 160), (384, 40)):
                bench_block(C, hw, dname, opt.inner)
