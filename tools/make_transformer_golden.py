#!/usr/bin/env python3
"""Dev-time generator of tests/golden/tr_*.npz: the reference's OWN TransformerLayer / TransformerBlock / C3TR classes (and through
them torch's nn.MultiheadAttention), run on the CPU in float64, train mode.

    python tools/make_transformer_golden.py --reference <checkout of the reference project>

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad and Conv (:38-58), TransformerLayer and
TransformerBlock (:79-112), Bottleneck (:115-125), C3 (:161-172) and C3TR (:183-188) are exec'd in a namespace that provides math,
torch and nn.  Only arrays are written, per case:

  cls, args     class name and positional constructor arguments
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x     (N, C, H, W); a TransformerLayer sees x as the (H*W, N, C) sequence the block would hand it

Weights are drawn ~ N(0, 1/fan_in), every bias (in_proj_bias, out_proj.bias, linear.bias) ~ N(0, 0.5^2) so that a dropped bias or
bias gradient shows; BatchNorm weights are uniform in [0.5, 1.5] and biases in [-0.3, 0.3].  Everything drawn is rounded to float32
first (the f32 GPU path then starts from the same numbers); the reference itself runs in float64.  Parameters (exact in float32)
and their gradients (rounded to float32, 6e-8 relative) are stored as float32, and so are x and grad_out (drawn in float32: exact);
out and grad_x stay float64.  A file holds every parameter and its gradient, 8 bytes per parameter: 9 c^2 weights per layer make
the cases 127 to 384 KB, above the 100 000 bytes the smaller fixture families keep and under the repository's limit of 1 MiB per
committed file (tests/test_mha_ref_cpu.py checks the latter)."""
import argparse
import math
import os

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
RANGES = ((38, 58), (79, 112), (115, 125), (161, 172), (183, 188))

# name -> (class, positional arguments, input shape (N, C, H, W))
CASES = {
    "tr_layer_32_h4": ("TransformerLayer", (32, 4), (2, 32, 7, 5)),
    "tr_block_48_h2_l2": ("TransformerBlock", (48, 48, 2, 2), (2, 48, 5, 4)),
    "tr_block_16_32_h4_conv": ("TransformerBlock", (16, 32, 4, 1), (2, 16, 6, 6)),
    "tr_c3tr_32_64_n1": ("C3TR", (32, 64, 1), (2, 32, 6, 6)),          # c_ = 32: d = 8 (c2 = 32 would give d = 4)
}


def load_reference(ref):
    path = os.path.join(ref, "models", "common.py")
    lines = open(path, encoding="utf-8").read().split("\n")
    ns = dict(math=math, torch=torch, nn=nn)
    for a, b in RANGES:
        exec(compile("\n" * (a - 1) + "\n".join(lines[a - 1:b]), path, "exec"), ns)
    return ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    opt = ap.parse_args()
    ns = load_reference(opt.reference)
    os.makedirs(OUT, exist_ok=True)
    for seed, (name, (cls, args, shape)) in enumerate(CASES.items()):
        gen = torch.Generator().manual_seed(400 + seed)
        mod = ns[cls](*args).double().train()
        bn = {n for n, m in mod.named_modules() if isinstance(m, nn.BatchNorm2d)}
        with torch.no_grad():
            for key, p in mod.named_parameters():
                owner, _, leaf = key.rpartition(".")
                if owner in bn:
                    lo, hi = (0.5, 1.5) if leaf == "weight" else (-0.3, 0.3)
                    p.copy_((torch.rand(p.shape, generator=gen, dtype=torch.float64) * (hi - lo) + lo).float().double())
                elif p.dim() == 1:
                    p.copy_((torch.randn(p.shape, generator=gen, dtype=torch.float64) * 0.5).float().double())
                else:
                    p.copy_((torch.randn(p.shape, generator=gen, dtype=torch.float64) * (p[0].numel() ** -0.5)).float().double())
        before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
        x = torch.randn(*shape, generator=gen, dtype=torch.float64).float().double().requires_grad_(True)
        if cls == "TransformerLayer":
            N, C, H, W = shape
            out = mod(x.flatten(2).permute(2, 0, 1)).permute(1, 2, 0).reshape(N, C, H, W)
        else:
            out = mod(x)
        gout = torch.randn(out.shape, generator=gen, dtype=torch.float64).float().double()
        out.backward(gout)
        keys = list(before.keys())
        arrs = dict(cls=np.array(cls), args=np.array(args), keys=np.array(keys),
                    x=x.detach().float().numpy(), out=out.detach().numpy(), grad_out=gout.float().numpy(), grad_x=x.grad.numpy())
        for key in keys:
            v = before[key]
            arrs["p." + key] = v.float().numpy() if v.dtype.is_floating_point else v.numpy()
        for key, p in mod.named_parameters():
            arrs["g." + key] = p.grad.float().numpy()
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrs)
        print(f"{path}: {os.path.getsize(path)} bytes, out {tuple(out.shape)}, {len(keys)} keys")


if __name__ == "__main__":
    main()
