#!/usr/bin/env python3
"""Dev-time generator of tests/golden/gconv_*.npz: the reference's OWN Conv (with groups) and SPPCSPC_group classes, run on the CPU in
float64, train mode.

    python tools/make_gconv_golden.py --reference <checkout of the reference project>

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad and Conv (:38-64) and SPPCSPC_group
(:1451-1468) are exec'd in a namespace that provides math, warnings, torch and nn.  Only arrays are written, per case, in the layout
of tools/make_spp_golden.py:

  cls, args     class name and the positional constructor arguments as a JSON list
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x
  rm.<key>, rv.<key>   running_mean / running_var AFTER the one train-mode forward

Parameters are drawn as there (weights ~ N(0, 1/fan_in) with the fan-in of ONE group; BatchNorm weights uniform in [0.5, 1.5], biases
in [-0.3, 0.3]) and rounded to float32 first; the reference itself runs in float64; arrays are stored as float32."""
import argparse
import json
import math
import os
import warnings

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
RANGES = ((38, 64), (1451, 1468))

# name -> (class, positional arguments, input shape)
CASES = {
    "gconv_sppcspc_group_64_64": ("SPPCSPC_group", (64, 64), (2, 64, 9, 7)),        # seven Conv(g=4): 16 -> 16 and 64 -> 16 per group
    "gconv_conv_32_96_g2_k3": ("Conv", (32, 96, 3, 1, None, 2), (2, 32, 7, 5)),     # 16 -> 48 per group
}


def load_reference(ref):
    path = os.path.join(ref, "models", "common.py")
    lines = open(path, encoding="utf-8").read().split("\n")
    ns = dict(math=math, warnings=warnings, torch=torch, nn=nn)
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
        gen = torch.Generator().manual_seed(1300 + seed)
        mod = ns[cls](*args).double().train()
        bn = {n for n, m in mod.named_modules() if isinstance(m, nn.BatchNorm2d)}
        with torch.no_grad():
            for key, p in mod.named_parameters():
                owner, leaf = key.rsplit(".", 1)
                if owner in bn:
                    lo, hi = (0.5, 1.5) if leaf == "weight" else (-0.3, 0.3)
                    p.copy_((torch.rand(p.shape, generator=gen, dtype=torch.float64) * (hi - lo) + lo).float().double())
                else:
                    fan_in = p[0].numel()
                    p.copy_((torch.randn(p.shape, generator=gen, dtype=torch.float64) * (fan_in ** -0.5)).float().double())
        before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
        x = torch.randn(*shape, generator=gen, dtype=torch.float64).float().double().requires_grad_(True)
        out = mod(x)
        gout = torch.randn(out.shape, generator=gen, dtype=torch.float64).float().double()
        out.backward(gout)
        keys = list(before.keys())
        arrs = dict(cls=np.array(cls), args=np.array(json.dumps(list(args))), keys=np.array(keys),
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
        arrs = {k: v.astype(np.float32) if v.dtype == np.float64 else v for k, v in arrs.items()}
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrs)
        nparam = sum(p.numel() for p in mod.parameters())
        print(f"{path}: {os.path.getsize(path)} bytes, out {tuple(out.shape)}, {len(keys)} keys, {nparam} parameters")


if __name__ == "__main__":
    main()
