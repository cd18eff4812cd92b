#!/usr/bin/env python3
"""Dev-time generator of tests/golden/spp_*.npz: the reference's OWN SPP, C3SPP, SimSPPF, SPPCSPC and SimCSPSPPF classes, run on the
CPU in float64, train mode.

    python tools/make_spp_golden.py --reference <checkout of the reference project>

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad and Conv (:38-64), Bottleneck (:115-125),
C3 (:161-172), C3SPP (:191-197), SPP (:1275-1286), SimConv and SimSPPF (:1292-1330), SPPCSPC (:1430-1448) and SimCSPSPPF
(:1473-1492) are exec'd in a namespace that provides math, warnings, torch and nn.  Only arrays are written, per case:

  cls, args     class name and the positional constructor arguments as a JSON list
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x
  rm.<key>, rv.<key>   running_mean / running_var AFTER the one train-mode forward

Parameters are drawn as in tools/make_dilated_golden.py (weights ~ N(0, 1/fan_in); BatchNorm weights uniform in [0.5, 1.5], biases in
[-0.3, 0.3]).  Everything drawn is rounded to float32 first (the f32 GPU path then starts from the same numbers); the reference itself
runs in float64.  Arrays are stored as float32: exact for what was drawn, a rounding of 6e-8 for the results, far below the 1e-4 the
fixtures are compared at."""
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
RANGES = ((38, 64), (115, 125), (161, 172), (191, 197), (1275, 1286), (1292, 1330), (1430, 1448), (1473, 1492))

# name -> (class, positional arguments, input shape)
CASES = {
    "spp_16_16": ("SPP", (16, 16), (2, 16, 9, 7)),                      # k = (5, 9, 13): every window overhangs the plane
    "spp_c3_16_16_k35": ("C3SPP", (16, 16, (3, 5)), (2, 16, 8, 8)),     # two pools: one max-pool launch per window size
    "spp_cspc_16_16": ("SPPCSPC", (16, 16), (2, 16, 20, 13)),
    "spp_sim_16_16": ("SimSPPF", (16, 16, 5), (2, 16, 9, 7)),
    "spp_simcsp_16_16": ("SimCSPSPPF", (16, 16), (2, 16, 9, 7)),
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
        gen = torch.Generator().manual_seed(900 + seed)
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
