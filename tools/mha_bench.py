#!/usr/bin/env python3
"""Dev-time benchmark of the dense multi-head self-attention op alone (ydl_mha_fwd / ydl_mha_bwd), bf16 and f32, against
torch.nn.functional.scaled_dot_product_attention and nn.MultiheadAttention on the same GPU.

    python tools/mha_bench.py [--iters 50]

Prints, per shape (N, S, heads, d) and dtype: milliseconds forward and backward for the three, the FLOP floor (4*N*heads*S^2*d forward,
10* backward, at the dense bf16 MFMA rate DESIGN.md section 8 quotes; f32 at 1/16 of it) and the byte floor (q, k, v, out once forward;
q, k, v, out, dout, dq, dk, dv backward) at the HBM rate quoted there."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yolo_dual_amd import _lib as L  # noqa: E402

SHAPES = [(16, 400, 4, 64), (16, 400, 4, 32), (8, 1024, 4, 64), (16, 1600, 4, 32)]
MFMA_BF16_TFLOPS, HBM_TBPS = 2500.0, 8.0


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def timeit(fn, iters):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    opt = ap.parse_args()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    print(f"{'shape':>20} {'dtype':>5} | {'ours fwd':>9} {'bwd':>8} | {'sdpa fwd':>9} {'bwd':>8} | {'nn.MHA fwd':>10} {'bwd':>8} | "
          f"{'flop floor f/b':>15} {'byte floor f/b':>15}   (ms)")
    for N, S, H, d in SHAPES:
        C = H * d
        for name, dt, tdt in (("bf16", L.YDL_BF16, torch.bfloat16), ("f32", L.YDL_F32, torch.float32)):
            qkv = torch.randn(N * S, 3 * C, device="cuda").to(tdt)
            out, dout, dqkv = torch.empty(N * S, C, device="cuda", dtype=tdt), torch.randn(N * S, C, device="cuda").to(tdt), torch.empty_like(qkv)
            lse = torch.empty(N * H * S, device="cuda")
            ws = torch.empty(L.lib().ydl_mha_bwd_ws_bytes(N, S, H) // 4, device="cuda")
            es = qkv.element_size()
            blk = [ctypes.c_void_p(qkv.data_ptr() + i * C * es) for i in range(3)]
            dblk = [ctypes.c_void_p(dqkv.data_ptr() + i * C * es) for i in range(3)]
            sc = d ** -0.5
            fwd = lambda: L.call("ydl_mha_fwd", dt, blk[0], 3 * C, blk[1], 3 * C, blk[2], 3 * C, _p(out), C, _p(lse), N, S, H, d, sc, st)
            bwd = lambda: L.call("ydl_mha_bwd", dt, blk[0], 3 * C, blk[1], 3 * C, blk[2], 3 * C, _p(out), C, _p(lse), _p(dout), C,
                                 dblk[0], dblk[1], dblk[2], 3 * C, 0, _p(ws), N, S, H, d, sc, st)
            t_f, t_b = timeit(fwd, opt.iters), timeit(bwd, opt.iters)
            # torch: (N, H, S, d) operands
            q, k, v = (torch.randn(N, H, S, d, device="cuda").to(tdt).requires_grad_(True) for _ in range(3))
            go = torch.randn(N, H, S, d, device="cuda").to(tdt)
            sd = lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v)
            o = sd()
            s_f = timeit(lambda: sd(), opt.iters)
            s_b = timeit(lambda: torch.autograd.grad(o, (q, k, v), go, retain_graph=True), opt.iters)
            mha = torch.nn.MultiheadAttention(C, H).cuda().to(tdt)
            xq, xk, xv = (torch.randn(S, N, C, device="cuda").to(tdt).requires_grad_(True) for _ in range(3))
            mo = mha(xq, xk, xv, need_weights=False)[0]
            gm = torch.randn_like(mo)
            m_f = timeit(lambda: mha(xq, xk, xv, need_weights=False), opt.iters)
            m_b = timeit(lambda: torch.autograd.grad(mo, (xq, xk, xv), gm, retain_graph=True), opt.iters)
            rate = MFMA_BF16_TFLOPS * 1e12 / (1 if name == "bf16" else 16)
            ff = 4.0 * N * H * S * S * d / rate * 1e3
            bf = 4.0 * N * S * C * es / (HBM_TBPS * 1e12) * 1e3
            print(f"{str((N, S, H, d)):>20} {name:>5} | {t_f:9.4f} {t_b:8.4f} | {s_f:9.4f} {s_b:8.4f} | {m_f:10.4f} {m_b:8.4f} | "
                  f"{ff:7.4f}/{2.5 * ff:7.4f} {bf:7.4f}/{2 * bf:7.4f}", flush=True)


if __name__ == "__main__":
    main()
