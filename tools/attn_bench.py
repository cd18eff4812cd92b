#!/usr/bin/env python3
"""Micro-benchmark of the local self-attention op (ydl_local_attn_fwd / _bwd) at the three shapes a width-0.25 Attention/Self yaml
produces at 640^2, bs = 16 (64 ch @ 80^2, 128 ch @ 40^2, 256 ch @ 20^2; k = 3, the AttentionConv form), both dtypes, beside

  * the byte floor: algorithmic bytes (Q, K, V and dout read once; out, dQ, dK, dV written once) at the 6.3 TB/s streaming rate of
    DESIGN.md section 8, and
  * the same math as the torch composition of tests/local_attn_ref.py, forward and autograd backward, same dtype, same GPU.

    python tools/attn_bench.py [--iters 20]                       (dev tool; prints one line per shape and dtype)"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from tests import local_attn_ref as R
from yolo_dual_amd import _lib as L

STREAM_RATE = 6.3e12
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


def timed(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    opt = ap.parse_args()
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N, ks = 16, 3
    for C, H in ((64, 80), (128, 40), (256, 20)):
        for name, dt, tdt, es in (("bf16", L.YDL_BF16, torch.bfloat16, 2), ("f32 ", L.YDL_F32, torch.float32, 4)):
            npix = N * H * H
            q, k, v, go = (torch.randn(npix, C, device=dev).mul(0.8).to(tdt) for _ in range(4))
            rh, rw = torch.randn(C // 2, ks, device=dev), torch.randn(C // 2, ks, device=dev)
            out = torch.empty(npix, C, device=dev, dtype=tdt)
            lse = torch.empty(npix, C, device=dev)
            dq, dk, dv = (torch.empty(npix, C, device=dev, dtype=tdt) for _ in range(3))
            drh, drw = torch.zeros_like(rh), torch.zeros_like(rw)
            ws = torch.empty(L.lib().ydl_local_attn_bwd_ws_bytes(C, ks, 1) // 4, device=dev)

            def fwd():
                L.call("ydl_local_attn_fwd", dt, P(q), C, P(k), C, P(v), C, 0, 1, P(rh), P(rw), None, P(out), C, P(lse), N, H, H, C, ks, st)

            def bwd():
                L.call("ydl_local_attn_bwd", dt, P(q), C, P(k), C, P(v), C, 0, 1, P(rh), P(rw), None, P(out), C, P(lse), P(go), C,
                       P(dq), P(dk), P(dv), C, 0, 0, P(drh), P(drw), None, P(ws), N, H, H, C, ks, st)
            tf, tb = timed(fwd, opt.iters), timed(bwd, opt.iters)
            # torch composition: NCHW tensors of the same dtype
            nchw = lambda t: t.view(N, H, H, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
            tq, tk, tv = nchw(q), nchw(k), nchw(v)
            trh, trw = rh.to(tdt).requires_grad_(True), rw.to(tdt).requires_grad_(True)
            tgo = go.view(N, H, H, C).permute(0, 3, 1, 2).contiguous()
            tfw = lambda: R.local_attention(tq, tk, [tv], ks, trh, trw)

            def tboth():
                for t in (tq, tk, tv, trh, trw):
                    t.grad = None
                tfw().backward(tgo)
            ttf, ttfb = timed(lambda: tfw().detach(), opt.iters), timed(tboth, opt.iters)
            # algorithmic bytes: Q, K, V and dout read once; out, dQ, dK, dV written once (four tensors each way; what the backward
            # re-reads of Q, K, V, out and the f32 lse rows is real traffic on top of the floor)
            floor = 8 * npix * C * es / STREAM_RATE * 1e6
            print(f"{C:3d} ch @ {H}^2 {name} | fwd {tf:6.1f} us  bwd {tb:6.1f} us  fwd+bwd {tf + tb:6.1f} us | byte floor fwd+bwd {floor:5.1f} us "
                  f"({floor / (tf + tb) * 100:4.1f} %) | torch composition fwd {ttf:7.1f} us  fwd+bwd {ttfb:7.1f} us = {ttfb / (tf + tb):5.2f}x",
                  flush=True)


if __name__ == "__main__":
    main()
