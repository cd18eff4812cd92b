#!/usr/bin/env python3
"""Per-layer A/B of the BatchNorm backward behind a one-pass 1x1 backward (dev tool): 128 -> 128 channels at bs x 160 x 160,

    unfused: ydl_bn_act_bwd_sums (reduce + apply)  +  ydl_conv_bwd_pw
    fused:   ydl_bn_act_bwd_reduce_sums            +  ydl_conv_bwd_pw_bn

on rotating operand sets (a re-used set sits in the Infinity Cache and flatters both).  Every case is timed --rounds times, the two
forms alternating; the table gives the mean and the spread of each.
usage: python tools/pw_bn_bench.py [--bs 16] [--rotate 6] [--iters 20] [--rounds 3]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from yolo_dual_amd import _lib as L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--hw", type=int, default=160)
    ap.add_argument("--rotate", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    C, N, H = 128, a.bs, a.hw
    M = N * H * H
    bf, R = torch.bfloat16, a.rotate
    xs = [torch.randn(M, C, device=dev).to(bf) for _ in range(R)]
    ys = [(torch.randn(M, C, device=dev) * 1.5 + 0.5).to(bf) for _ in range(R)]
    dos = [torch.randn(M, C, device=dev).to(bf) for _ in range(R)]
    dxs = [torch.zeros(M, C, device=dev, dtype=bf) for _ in range(R)]
    dys = [torch.empty(M, C, device=dev, dtype=bf) for _ in range(R)]
    wt = (torch.randn(C, C, device=dev) / C ** 0.5).to(bf)
    dw = torch.zeros(C, C, device=dev)
    mean, invstd = torch.full((C,), 0.5, device=dev), torch.full((C,), 1 / 1.5, device=dev)
    scale, shift = torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) - 0.5
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    g = L.ConvGeom(N, H, H, C, H, H, C, 1, 1, 0, C, C, 0)
    gp = ctypes.byref(g)
    dt = L.YDL_BF16
    assert L.lib().ydl_conv_bwd_pw_bn_supported(gp, dt)
    sums = torch.zeros(8 * 2 * C, device=dev)           # (never cleared between iterations: the values do not matter to the timing)

    def unfused(i, act, nseg, acc):
        for c0 in range(0, C, C // nseg):
            cw = C // nseg
            L.call("ydl_bn_act_bwd_sums", dt, P(ys[i][:, c0:]), C, P(dos[i][:, c0:]), C, None, 0, P(mean[c0:]), P(invstd[c0:]), P(scale[c0:]),
                   P(shift[c0:]), 0, act, P(dys[i][:, c0:]), C, None, 0, P(dg[c0:]), P(db[c0:]), 0, P(sums), M, cw, cw, st)
        L.call("ydl_conv_bwd_pw", gp, dt, P(xs[i]), P(dys[i]), P(wt), P(dxs[i]), C, acc, P(dw), st)

    def fused(i, act, nseg, acc):
        for c0 in range(0, C, C // nseg):
            cw = C // nseg
            L.call("ydl_bn_act_bwd_reduce_sums", dt, P(ys[i][:, c0:]), C, P(dos[i][:, c0:]), C, None, 0, P(mean[c0:]), P(invstd[c0:]),
                   P(scale[c0:]), P(shift[c0:]), 0, act, None, 0, P(sums[c0 * 16:]), M, cw, cw, st)
        two = nseg == 2
        L.call("ydl_conv_bwd_pw_bn", gp, dt, P(xs[i]), P(ys[i]), C, P(dos[i]), C, P(dos[i][:, 64:]) if two else None, C if two else 0,
               P(mean), P(invstd), P(scale), P(shift), P(sums), P(sums[1024:]) if two else None, M, act, P(dg), P(db), 0, None, 0,
               P(wt), P(dxs[i]), C, acc, P(dw), st)

    def timed(fn, *args):
        it = 0
        for _ in range(3):
            fn(it % R, *args)
            it += 1
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn(it % R, *args)
            it += 1
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters * 1e3

    print(f"128 -> 128 @ {N} x {H} x {H}, {R} rotating sets, {a.iters} iterations x {a.rounds} rounds; us per layer backward (BN backward + conv backward)")
    for act, an in ((L.ACT_SILU, "silu"), (L.ACT_NONE, "none")):
        for nseg in (1, 2):
            for acc in (0, 1):
                tu, tf = [], []
                for _ in range(a.rounds):
                    tu.append(timed(unfused, act, nseg, acc))
                    tf.append(timed(fused, act, nseg, acc))
                mu, mf = sum(tu) / len(tu), sum(tf) / len(tf)
                print(f"act {an:4s} segments {nseg} accumulate {acc}: unfused {mu:7.1f} (spread {max(tu) - min(tu):5.1f})  "
                      f"fused {mf:7.1f} (spread {max(tf) - min(tf):5.1f})  fused - unfused {mf - mu:+7.1f}", flush=True)


if __name__ == "__main__":
    main()
