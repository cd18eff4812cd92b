#!/usr/bin/env python3
"""Micro-benchmark of the squeeze-excitation kernels (csrc/se.hip) at batch 16 and the SE shapes of a 640^2 batch, bf16 and f32:
MobileNetV3-small 16 ch @ 160^2, 96 @ 40^2, 576 @ 20^2 and EfficientNet-B0 32 ch @ 320^2, 240 @ 80^2, 1152 @ 20^2 (squeeze widths 8, 24,
144 and 8, 10, 48).

(a) One line per kernel, shape and dtype against its byte floor: the tensors the pass must read and write, each once, over 6.3 TB/s, the
    rate a streaming copy reaches.  pool: x; dgate (the pool's product form): dy + x; scale_bwd: dy + dx; the forward multiply
    (ydl_scale_channels): x + out.  ydl_channel_dot, the existing kernel the dgate pass replaces, is timed next to it.  The excitation
    launches move kilobytes: their time is reported as it is (launch-bound), with the bytes of the two weight matrices as the floor.
(b) The whole gate forward + backward (six entry points) against the composition of existing pieces that GAM uses today, WITHOUT its two
    1x1 convolutions each way (which only flatters the composition): ydl_global_pool_fwd, ydl_gate_fwd, ydl_scale_channels; then
    ydl_channel_dot, ydl_gate_bwd, ydl_scale_channels into a temporary, ydl_copy2d adding it, ydl_global_pool_bwd adding the pooled term.
(c) One InvertedResidual / MBConv training step (forward + backward) of this package against the plain-torch module of tests/se_ref.py
    on the GPU in channels_last, f32 and bf16.

Device events; 10 warm-up runs and 30 timed runs per variant, each run ``--inner`` launches between two events ended by a device
synchronise, variants alternated run by run; the median run is reported.  The first variant is timed twice in the same alternation:
``spread`` is the relative difference of its two medians.

    python tools/se_bench.py [--inner 10] [--only bf16] [--skip-block]"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from yolo_dual_amd import _lib as L

WARMUP, RUNS = 10, 30
STREAM_RATE = 6.3e12
# (C, Cs, map side, act, gate)
SHAPES = ((16, 8, 160, "relu", "hardsigmoid"), (96, 24, 40, "relu", "hardsigmoid"), (576, 144, 20, "relu", "hardsigmoid"),
          (32, 8, 320, "silu", "sigmoid"), (240, 10, 80, "silu", "sigmoid"), (1152, 48, 20, "silu", "sigmoid"))
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


def line(head, dname, us, spread, floor_us, extra=""):
    print(f"{head:34s} bs{N} {dname:4s} | {us:8.1f} us  spread {100 * spread:4.1f} %  byte floor {floor_us:7.1f} us ({us / floor_us:5.2f}x){extra}",
          flush=True)


def bench_kernels(C, Cs, side, act, gate, dname, inner):
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dt, tdt, es = (L.YDL_BF16, torch.bfloat16, 2) if dname == "bf16" else (L.YDL_F32, torch.float32, 4)
    hw = side * side
    npix = N * hw
    lib = L.lib()
    ac = L.ACT_RELU if act == "relu" else L.ACT_SILU
    gc = L.SE_GATE_HSIGMOID if gate == "hardsigmoid" else L.SE_GATE_SIGMOID
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)
    f32 = lambda *s: torch.empty(*s, device=dev)
    x, dout = rnd(npix, C).to(tdt), rnd(npix, C).to(tdt)
    out, dx, tmp = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    w1, b1, w2, b2 = rnd(Cs, C) * C ** -0.5, rnd(Cs) * 0.1, rnd(C, Cs) * Cs ** -0.5, rnd(C) * 0.1
    gw1, gb1, gw2, gb2 = (torch.zeros_like(t) for t in (w1, b1, w2, b2))
    S = lib.ydl_se_pool_splits(N, hw)
    part, dpart = f32(N * S * C), f32(N * S * C)
    pooled, z, g, dpool, dgate = (f32(N, C) for _ in range(5))
    h = f32(N, Cs)
    ws = f32(max(lib.ydl_se_excite_bwd_ws_bytes(N, C, Cs) // 4, 4))
    tag = f"{C} ch @ {side}^2"
    k_pool = lambda: L.call("ydl_se_pool_fwd", dt, P(x), C, None, 0, P(part), N, hw, C, st)
    k_exf = lambda: L.call("ydl_se_excite_fwd", P(part), S, P(w1), P(b1), P(w2), P(b2), ac, gc, P(pooled), P(h), P(z), P(g), N, hw, C, Cs, st)
    k_mul = lambda: L.call("ydl_scale_channels", dt, P(x), C, P(g), P(out), C, N, hw, C, st)
    k_dg = lambda: L.call("ydl_se_pool_fwd", dt, P(dout), C, P(x), C, P(dpart), N, hw, C, st)
    k_exb = lambda: L.call("ydl_se_excite_bwd", P(dpart), S, P(pooled), P(h), P(z), P(w1), P(w2), ac, gc, P(dpool), P(gw1), P(gb1), P(gw2),
                           P(gb2), P(ws), N, C, Cs, st)
    k_sb = lambda: L.call("ydl_se_scale_bwd", dt, P(dout), C, P(g), P(dpool), P(dx), C, 0, N, hw, C, st)
    k_dot = lambda: L.call("ydl_channel_dot", dt, P(dout), C, P(x), C, P(dgate), N, hw, C, st)
    for fn in (k_pool, k_exf, k_mul, k_dg, k_exb, k_sb, k_dot):
        fn()
    torch.cuda.synchronize()
    # the results agree with torch before anything is timed
    xr = x.float().view(N, hw, C)
    pr = xr.mean(1)
    hr = pr @ w1.T + b1
    zr = (torch.relu(hr) if act == "relu" else torch.nn.functional.silu(hr)) @ w2.T + b2
    gr = torch.nn.functional.hardsigmoid(zr) if gate == "hardsigmoid" else torch.sigmoid(zr)
    assert torch.allclose(pooled, pr, rtol=1e-4, atol=1e-5) and torch.allclose(g, gr, rtol=1e-4, atol=1e-5)
    assert torch.allclose(dpart.view(N, S, C).sum(1), dgate, rtol=1e-3, atol=1e-2 * float(dgate.abs().max()))
    fl = lambda passes: passes * npix * C * es / STREAM_RATE * 1e6
    wfl = 2 * C * Cs * 4 / STREAM_RATE * 1e6
    for head, fn, floor in (("se_pool_fwd", k_pool, fl(1)), ("se_pool_fwd dgate form", k_dg, fl(2)), ("se_scale_bwd", k_sb, fl(2)),
                            ("scale_channels (forward product)", k_mul, fl(2)), ("channel_dot (replaced dgate)", k_dot, fl(2))):
        m = medians({"kernel": fn}, inner)
        line(f"{head} {tag}", dname, m["kernel"], m["spread"], floor)
    for head, fn in (("se_excite_fwd", k_exf), ("se_excite_bwd (2 launches)", k_exb)):
        m = medians({"kernel": fn}, inner)
        line(f"{head} {C}->{Cs}", dname, m["kernel"], m["spread"], wfl, "  (launch-bound)")
    # (b) the whole gate against the composition of existing pieces
    avg, mx = torch.empty(N, C, device=dev, dtype=tdt), torch.empty(N, C, device=dev, dtype=tdt)
    amax = torch.empty(N, C, device=dev, dtype=torch.int32)
    da, db_ = torch.empty_like(avg), torch.empty_like(avg)
    g2 = f32(N, C)

    def new():
        k_pool(); k_exf(); k_mul(); k_dg(); k_exb(); k_sb()

    def old():
        L.call("ydl_global_pool_fwd", dt, P(x), C, P(avg), C, P(mx), C, P(amax), N, hw, C, st)
        L.call("ydl_gate_fwd", dt, P(avg), C, P(mx), C, P(g2), N, C, st)
        L.call("ydl_scale_channels", dt, P(x), C, P(g2), P(out), C, N, hw, C, st)
        L.call("ydl_channel_dot", dt, P(dout), C, P(x), C, P(dgate), N, hw, C, st)
        L.call("ydl_gate_bwd", dt, P(g2), P(dgate), P(da), C, 0, P(db_), C, 0, N, C, st)
        L.call("ydl_scale_channels", dt, P(dout), C, P(g2), P(tmp), C, N, hw, C, st)
        L.call("ydl_copy2d", dt, P(tmp), C, P(dx), C, npix, C, 1, st)
        L.call("ydl_global_pool_bwd", dt, P(da), C, None, C, P(amax), P(dx), C, 1, N, hw, C, st)
    m = medians({"kernel": new, "old": old}, inner)
    print(f"{'SE gate fwd+bwd ' + tag:34s} bs{N} {dname:4s} | new {m['kernel']:8.1f} us  existing pieces {m['old']:8.1f} us "
          f"({m['old'] / m['kernel']:4.2f}x)  spread {100 * m['spread']:4.1f} %  byte floor {fl(6):7.1f} us ({m['kernel'] / fl(6):5.2f}x)", flush=True)


def bench_block(cls, args, C, side, dname, inner):
    import yolo_dual_amd as ydl
    from tests import se_ref as R
    ydl.set_compute_dtype(dname)
    tdt = torch.bfloat16 if dname == "bf16" else torch.float32
    torch.manual_seed(0)
    ref = getattr(R, cls)(*args).cuda().train()
    mod = getattr(ydl, cls)(*args)
    mod.load_state_dict(ref.state_dict())
    mod = mod.cuda().train()
    ref = ref.to(tdt).to(memory_format=torch.channels_last)
    x = torch.randn(N, C, side, side, device="cuda")
    gout = torch.randn(N, C, side, side, device="cuda")
    xt, gt = x.to(tdt).contiguous(memory_format=torch.channels_last), gout.to(tdt).contiguous(memory_format=torch.channels_last)

    def ours():
        mod(x.requires_grad_(True)).backward(gout)

    def theirs():
        ref(xt.requires_grad_(True)).backward(gt)
    m = medians({"kernel": ours, "torch": theirs}, max(inner // 5, 1))
    print(f"{cls + ' step ' + str(C) + ' ch @ ' + str(side) + '^2':34s} bs{N} {dname:4s} | this {m['kernel'] / 1e3:7.2f} ms  plain torch "
          f"{m['torch'] / 1e3:7.2f} ms ({m['torch'] / m['kernel']:4.2f}x)  spread {100 * m['spread']:4.1f} %  (ours includes the NCHW f32 edge "
          "conversions)", flush=True)
    ydl.set_compute_dtype("bf16")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", default="", help="comma list of dtypes (bf16,f32)")
    ap.add_argument("--skip-block", action="store_true")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("se_bench: needs a GPU (a CPU run cannot give a time)")
    dnames = [d for d in ("bf16", "f32") if not opt.only or d in opt.only.split(",")]
    for dname in dnames:
        for shape in SHAPES:
            bench_kernels(*shape, dname, opt.inner)
    if not opt.skip_block:
        for dname in dnames:
            bench_block("InvertedResidual", (40, 5, 240, 40, True, "HS", 1), 40, 40, dname, opt.inner)
            bench_block("MBConv", (6, 5, 1, 40, 40), 40, 80, dname, opt.inner)
