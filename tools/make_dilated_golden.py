#!/usr/bin/env python3
"""Dev-time generator of tests/golden/dil_*.npz: the reference's OWN Conv (dilated), BasicConv, RFB and ASPP classes, run on the CPU
in float64, train mode.

    python tools/make_dilated_golden.py --reference <checkout of the reference project>

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad and Conv (:38-64), ASPP (:1336-1361),
BasicConv (:1366-1384) and RFB (:1386-1425) are exec'd in a namespace that provides math, torch, nn and F.  Only arrays are written,
per case:

  cls, args     class name and the positional constructor arguments as a JSON list (Conv's padding is None)
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x
  rm.<key>, rv.<key>   running_mean / running_var AFTER the one train-mode forward (the cases that hold a BatchNorm)

Parameters are drawn as in tools/make_ghost_golden.py (weights and convolution biases ~ N(0, 1/fan_in)); BatchNorm weights are
uniform in [0.5, 1.5] and biases in [-0.3, 0.3].  Everything drawn is rounded to float32 first (the f32 GPU path then starts from
the same numbers); the reference itself runs in float64.  Arrays are stored as float32: exact for what was drawn, a rounding of 6e-8
for the results, far below the 1e-4 the fixtures are compared at, and half the bytes (the RFB case has 17k parameters)."""
import argparse
import json
import math
import os
import warnings

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
RANGES = ((38, 64), (1336, 1361), (1366, 1384), (1386, 1425))

# name -> (class, positional arguments, input shape)
CASES = {
    "dil_conv_16_24_d2": ("Conv", (16, 24, 3, 1, None, 1, 2), (2, 16, 9, 7)),
    # BasicConv(12, 16, 3, padding=3, dilation=3, relu=False): (in, out, kernel_size, stride, padding, dilation, groups, relu)
    "dil_basic_12_16_d3": ("BasicConv", (12, 16, 3, 1, 3, 3, 1, False), (2, 12, 8, 8)),
    "dil_aspp_16_8": ("ASPP", (16, 8), (2, 16, 20, 13)),
    "dil_rfb_64_32": ("RFB", (64, 32), (2, 64, 8, 8)),            # scale = 0.1, map_reduce = 8, vision = 1: the defaults
}


def load_reference(ref):
    path = os.path.join(ref, "models", "common.py")
    lines = open(path, encoding="utf-8").read().split("\n")
    ns = dict(math=math, torch=torch, nn=nn, F=F)
    for a, b in RANGES:
        exec(compile("\n" * (a - 1) + "\n".join(lines[a - 1:b]), path, "exec"), ns)
    return ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    opt = ap.parse_args()
    ns = load_reference(opt.reference)
    warnings.filterwarnings("ignore", category=UserWarning)        # F.upsample is deprecated spelling of F.interpolate
    os.makedirs(OUT, exist_ok=True)
    for seed, (name, (cls, args, shape)) in enumerate(CASES.items()):
        gen = torch.Generator().manual_seed(700 + seed)
        mod = ns[cls](*args).double().train()
        bn = {n for n, m in mod.named_modules() if isinstance(m, nn.BatchNorm2d)}
        with torch.no_grad():
            for key, p in mod.named_parameters():
                owner, leaf = key.rsplit(".", 1)
                if owner in bn:
                    lo, hi = (0.5, 1.5) if leaf == "weight" else (-0.3, 0.3)
                    p.copy_((torch.rand(p.shape, generator=gen, dtype=torch.float64) * (hi - lo) + lo).float().double())
                else:
                    fan_in = dict(mod.named_parameters())[owner + ".weight"][0].numel()
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
        print(f"{path}: {os.path.getsize(path)} bytes, out {tuple(out.shape)}, {len(keys)} keys")


if __name__ == "__main__":
    main()
