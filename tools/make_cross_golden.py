#!/usr/bin/env python3
"""Dev-time generator of tests/golden/cross_*.npz: the reference's OWN Conv (with a (1, k) / (k, 1) kernel), CrossConv and C3x classes,
run on the CPU in float64, train mode.

    python tools/make_cross_golden.py --reference <checkout of the reference project>

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad and Conv (:38-64), Bottleneck (:115-125, C3's
constructor needs it) and CrossConv, C3 and C3x (:147-180) are exec'd in a namespace that provides math, warnings, torch and nn.  Only
arrays are written, per case, in the layout of tools/make_gconv_golden.py:

  cls, args     class name and the positional constructor arguments as a JSON list
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x
  rm.<key>, rv.<key>   running_mean / running_var AFTER the one train-mode forward
  floor.out, floor.grad, floor.run     the bf16 floor, see below

Parameters are drawn as there (weights ~ N(0, 1/fan_in); BatchNorm weights uniform in [0.5, 1.5], biases in [-0.3, 0.3]) and rounded to
float32 first; the reference itself runs in float64; arrays are stored as float32.

The bf16 floor is the reference's own error when its tensors pass through bf16 where a bf16 implementation stores them: the same module
with the same parameters is run a second time, everything in float64 except that the input, every nn.Conv2d weight, every nn.Conv2d
output and its incoming gradient, and every Conv module output and its incoming gradient are rounded to bf16 (a rounding
autograd.Function applied in forward hooks).  floor.out / floor.grad / floor.run are the worst error of that run against the float64
run, relative to each tensor's max, over the output / the gradients of x and of every parameter / the running statistics."""
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
RANGES = ((38, 64), (115, 125), (147, 180))

# name -> (class, positional arguments, input shape)
CASES = {
    "cross_conv_1x3_16_24": ("Conv", (16, 24, (1, 3), (1, 1)), (2, 16, 7, 5)),
    "cross_conv_5x1_s2_16_16": ("Conv", (16, 16, (5, 1), (2, 1)), (2, 16, 9, 6)),
    "cross_crossconv_16_16_add": ("CrossConv", (16, 16, 3, 1, 1, 1.0, True), (2, 16, 9, 7)),
    "cross_crossconv_16_32_s2": ("CrossConv", (16, 32, 3, 2), (2, 16, 9, 7)),
    "cross_c3x_32_32_n2": ("C3x", (32, 32, 2), (2, 32, 8, 6)),
}


def load_reference(ref):
    path = os.path.join(ref, "models", "common.py")
    lines = open(path, encoding="utf-8").read().split("\n")
    ns = dict(math=math, warnings=warnings, torch=torch, nn=nn)
    for a, b in RANGES:
        exec(compile("\n" * (a - 1) + "\n".join(lines[a - 1:b]), path, "exec"), ns)
    return ns


def bf16(t):
    return t.to(torch.bfloat16).to(torch.float64)


class RoundBoth(torch.autograd.Function):
    """the value on the way forward and its gradient on the way back, both through bf16"""

    @staticmethod
    def forward(ctx, t):
        return bf16(t)

    @staticmethod
    def backward(ctx, g):
        return bf16(g)


def run(mod, x, gout):
    """one train-mode forward + backward -> tensors by the fixture's names"""
    x = x.clone().requires_grad_(True)
    out = mod(x)
    out.backward(gout)
    res = {"out": out.detach(), "grad_x": x.grad}
    for key, p in mod.named_parameters():
        res["g." + key] = p.grad
    for key, v in mod.state_dict().items():
        if key.endswith("running_mean"):
            res["rm." + key] = v.detach().clone()
        elif key.endswith("running_var"):
            res["rv." + key] = v.detach().clone()
    return res


def bf16_floor(ns, cls, args, before, x, gout, exact):
    mod = ns[cls](*args).double().train()
    mod.load_state_dict(before)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(bf16(m.weight))
    for m in mod.modules():
        if isinstance(m, (nn.Conv2d, ns["Conv"])):
            m.register_forward_hook(lambda _m, _i, o: RoundBoth.apply(o))
    got = run(mod, bf16(x), gout)
    floor = {"out": 0.0, "grad": 0.0, "run": 0.0}
    for k, want in exact.items():
        kind = "out" if k == "out" else "run" if k[:3] in ("rm.", "rv.") else "grad"
        scale = float(want.abs().max())
        floor[kind] = max(floor[kind], float((got[k] - want).abs().max()) / (scale if scale > 0 else 1.0))
    return floor


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    opt = ap.parse_args()
    ns = load_reference(opt.reference)
    os.makedirs(OUT, exist_ok=True)
    for seed, (name, (cls, args, shape)) in enumerate(CASES.items()):
        gen = torch.Generator().manual_seed(1400 + seed)
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
        x = torch.randn(*shape, generator=gen, dtype=torch.float64).float().double()
        out_shape = mod.eval()(x).shape
        mod.train()
        gout = torch.randn(out_shape, generator=gen, dtype=torch.float64).float().double()
        exact = run(mod, x, gout)
        floor = bf16_floor(ns, cls, args, before, x, gout, exact)
        keys = list(before.keys())
        arrs = dict(cls=np.array(cls), args=np.array(json.dumps(list(args))), keys=np.array(keys), x=x.numpy(), grad_out=gout.numpy())
        for key in keys:
            arrs["p." + key] = before[key].numpy()
        for k, v in exact.items():
            arrs[k] = v.numpy()
        for k, v in floor.items():
            arrs["floor." + k] = np.array(v, dtype=np.float64)
        arrs = {k: v.astype(np.float32) if v.dtype == np.float64 and not k.startswith("floor.") else v for k, v in arrs.items()}
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrs)
        nparam = sum(p.numel() for p in mod.parameters())
        print(f"{path}: {os.path.getsize(path)} bytes, out {tuple(out_shape)}, {len(keys)} keys, {nparam} parameters, floor "
              + ", ".join(f"{k} {v:.2e}" for k, v in floor.items()))


if __name__ == "__main__":
    main()
