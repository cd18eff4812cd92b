#!/usr/bin/env python3
"""Micro-benchmark of ydl_space_to_depth / ydl_depth_to_space (csrc/s2d.hip) at bs 16, bf16 and f32:

  focus     Focus's concat on the 640^2 image: 3 ch @ 640^2 (row stride 8, the tape's padded NHWC image) -> 12 ch @ 320^2 (row stride 16),
            order 1; C = 3 runs on the element-granular kernel
  contract  Contract(2): 64 ch @ 160^2 -> 256 ch @ 80^2 and 128 ch @ 80^2 -> 512 ch @ 40^2, order 0, 16-byte chunks
  expand    Expand(2), their inverses: 256 ch @ 80^2 -> 64 ch @ 160^2 and 512 ch @ 40^2 -> 128 ch @ 80^2

One line per shape and dtype: the kernel, the same permutation done by torch on the same NHWC memory (view / permute / contiguous:
one strided copy kernel), and the byte floor: the logical bytes read once plus written once over 6.3 TB/s, the rate a streaming copy
reaches.  The torch result is compared with the kernel's, bit for bit, before anything is timed.

Device events; 10 warm-up runs and 30 timed runs per variant, each run ``--inner`` launches between two events ended by a device
synchronise, variants alternated run by run; the median run is reported.  The kernel is timed twice in the same alternation:
``spread`` is the relative difference of its two medians.

    python tools/sd_bench.py [--inner 10] [--only bf16]"""
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
P = lambda t: ctypes.c_void_p(t.data_ptr())


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


def bench(op, N, C, Hc, Wc, s, order, dname, inner):
    """``C`` channels per block, a coarse map of Hc x Wc: space-to-depth reads (N, Hc*s, Wc*s, C), depth-to-space writes it"""
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dt, tdt, es = (L.YDL_BF16, torch.bfloat16, 2) if dname == "bf16" else (L.YDL_F32, torch.float32, 4)
    ldf, ldc = (C + 7) // 8 * 8, (s * s * C + 7) // 8 * 8
    gen = torch.Generator(device=dev).manual_seed(1)
    fine = torch.randn(N, Hc * s, Wc * s, ldf, device=dev, generator=gen).to(tdt)
    coarse = torch.randn(N, Hc, Wc, ldc, device=dev, generator=gen).to(tdt)
    down = op != "expand"
    perm = (0, 1, 3, 2, 4, 5) if order == 0 else (0, 1, 3, 4, 2, 5)                 # (n, hc, wc, blk-major, blk-minor, c)
    if down:
        def kernel():
            L.call("ydl_space_to_depth", dt, P(fine), ldf, P(coarse), ldc, N, Hc * s, Wc * s, C, s, order, 0, st)

        def torch_way():
            return fine.view(N, Hc, s, Wc, s, ldf)[..., :C].permute(*perm).contiguous()
        kernel()
        assert torch.equal(coarse[..., :s * s * C].reshape(N, Hc, Wc, s, s, C), torch_way())
        head = f"{op:8s} {C:3d} ch {Hc * s}^2->{s * s * C} ch {Hc}^2"
    else:
        def kernel():
            L.call("ydl_depth_to_space", dt, P(coarse), ldc, P(fine), ldf, N, Hc, Wc, C, s, order, 0, st)

        def torch_way():
            return coarse[..., :s * s * C].view(N, Hc, Wc, s, s, C).permute(0, 1, 3, 2, 4, 5).contiguous()
        kernel()
        assert order == 0 and torch.equal(fine[..., :C].reshape(N, Hc, s, Wc, s, C), torch_way())
        head = f"{op:8s} {s * s * C:3d} ch {Hc}^2->{C} ch {Hc * s}^2"
    m = medians({"kernel": kernel, "torch": torch_way}, inner)
    floor = 2.0 * N * Hc * Wc * s * s * C * es / STREAM_RATE * 1e6
    path = "16-byte" if C % (16 // es) == 0 else "element"
    print(f"{head} bs{N} {dname:4s} | {path:7s} kernel {m['kernel']:7.1f} us  torch {m['torch']:7.1f} us ({m['torch'] / m['kernel']:4.2f}x)  "
          f"spread {100 * m['spread']:4.1f} %  byte floor {floor:6.1f} us ({m['kernel'] / floor:4.2f}x)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", default="", help="comma list of dtypes (bf16,f32)")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sd_bench: needs a GPU (a CPU run cannot give a time)")
    for dname in [d for d in ("bf16", "f32") if not opt.only or d in opt.only.split(",")]:
        bench("focus", 16, 3, 320, 320, 2, 1, dname, opt.inner)
        bench("contract", 16, 64, 80, 80, 2, 0, dname, opt.inner)
        bench("contract", 16, 128, 40, 40, 2, 0, dname, opt.inner)
        bench("expand", 16, 64, 80, 80, 2, 0, dname, opt.inner)
        bench("expand", 16, 128, 40, 40, 2, 0, dname, opt.inner)
