#!/usr/bin/env python3
"""Dev-time generator of tests/golden/ghost_*.npz: the reference's OWN DWConv / GhostConv / GhostBottleneck / C3Ghost classes, run
on the CPU in float64, train mode.

    python tools/make_ghost_golden.py --reference <checkout of the reference project>

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad, Conv and DWConv (:38-70), Bottleneck
(:115-125), C3 (:161-172), C3Ghost (:199-204) and GhostConv / GhostBottleneck (:253-279) are exec'd in a namespace that provides
math, torch and nn.  Only arrays are written, per case:

  cls, args     class name and positional constructor arguments
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x
  rm.<key>, rv.<key>   running_mean / running_var AFTER the one train-mode forward

Parameters are drawn as in tools/make_attn_golden.py (weights ~ N(0, 1/fan_in)); BatchNorm weights are uniform in [0.5, 1.5] and
biases in [-0.3, 0.3], so that no channel's batch variance is near zero.  Everything drawn is rounded to float32 first (the f32 GPU
path then starts from the same numbers, and the files compress to under 100 KB); the reference itself runs in float64."""
import argparse
import math
import os

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
RANGES = ((38, 70), (115, 125), (161, 172), (199, 204), (253, 279))

# name -> (class, positional arguments, keyword arguments, input shape)
CASES = {
    "ghost_dwconv_8_k3s2": ("DWConv", (8, 8, 3, 2), dict(act=False), (2, 8, 9, 7)),
    "ghost_conv_8_16": ("GhostConv", (8, 16, 1, 1), {}, (2, 8, 6, 6)),
    "ghost_conv_16_32_k3s2": ("GhostConv", (16, 32, 3, 2), {}, (2, 16, 8, 8)),
    "ghost_bneck_16_16_s1": ("GhostBottleneck", (16, 16, 3, 1), {}, (2, 16, 6, 6)),
    "ghost_bneck_16_32_s2": ("GhostBottleneck", (16, 32, 3, 2), {}, (2, 16, 8, 8)),
    "ghost_c3_16_16_n1": ("C3Ghost", (16, 16, 1), {}, (2, 16, 6, 6)),
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
    for seed, (name, (cls, args, kw, shape)) in enumerate(CASES.items()):
        gen = torch.Generator().manual_seed(300 + seed)
        mod = ns[cls](*args, **kw).double().train()
        bn = {n for n, m in mod.named_modules() if isinstance(m, nn.BatchNorm2d)}
        with torch.no_grad():
            for key, p in mod.named_parameters():
                owner, leaf = key.rsplit(".", 1)
                if owner in bn:
                    lo, hi = (0.5, 1.5) if leaf == "weight" else (-0.3, 0.3)
                    p.copy_((torch.rand(p.shape, generator=gen, dtype=torch.float64) * (hi - lo) + lo).float().double())
                else:
                    p.copy_((torch.randn(p.shape, generator=gen, dtype=torch.float64) * (p[0].numel() ** -0.5)).float().double())
        before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
        x = torch.randn(*shape, generator=gen, dtype=torch.float64).float().double().requires_grad_(True)
        out = mod(x)
        gout = torch.randn(out.shape, generator=gen, dtype=torch.float64).float().double()
        out.backward(gout)
        keys = list(before.keys())
        arrs = dict(cls=np.array(cls), args=np.array(args), act=np.array(int(kw.get("act", True))), keys=np.array(keys),
                    x=x.detach().numpy(), out=out.detach().numpy(), grad_out=gout.numpy(), grad_x=x.grad.numpy())
        for key in keys:
            arrs["p." + key] = before[key].numpy()
        for key, p in mod.named_parameters():
            arrs["g." + key] = p.grad.numpy()
        after = mod.state_dict()
        for key in keys:
            if key.endswith("running_mean"):
                arrs["rm." + key] = after[key].numpy()
            elif key.endswith("running_var"):
                arrs["rv." + key] = after[key].numpy()
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrs)
        print(f"{path}: {os.path.getsize(path)} bytes, out {tuple(out.shape)}, {len(keys)} keys")


if __name__ == "__main__":
    main()
