#!/usr/bin/env python3
"""Dev-time generator of tests/golden/act_*.npz: the reference's OWN Conv, DWConv and C3 classes under other activations than SiLU, and
its own AconC and FReLU layers, run on the CPU in float64, train mode.

    python tools/make_act_golden.py --reference <checkout of the reference project>

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad, Conv and DWConv (:38-70), Bottleneck
(:115-125) and C3 (:161-172), and those of utils/activations.py that hold FReLU and AconC (:53-78), are exec'd in a namespace that
provides math, warnings, torch, nn and F.  Only arrays are written, per case, in the layout of tools/make_cross_golden.py:

  cls, args     class name and the positional constructor arguments as a JSON list
  act, how      the activation as a string and how the module gets it: "arg" as the constructor's ``act=`` argument, "default" as
                ``Conv.default_act`` while the module is built.  The point-wise strings are what a yaml's ``activation:`` key holds
                (yolo_dual_amd.resolve_activation reads them); "AconC(c)" / "FReLU(c)" name the class and its channel count
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x
  rm.<key>, rv.<key>   running_mean / running_var AFTER the one train-mode forward
  floor.out, floor.grad, floor.run     the bf16 floor, see below

Parameters are drawn as there (weights ~ N(0, 1/fan_in); BatchNorm weights uniform in [0.5, 1.5], biases in [-0.3, 0.3]; AconC's p1, p2
~ N(0, 1) and beta uniform in [0.5, 1.5]) and rounded to float32 first; the reference itself runs in float64; arrays are stored as
float32.

The bf16 floor is the reference's own error when its tensors pass through bf16 where a bf16 implementation stores them: the same module
with the same parameters is run a second time, everything in float64 except that the input, every nn.Conv2d weight, every nn.Conv2d
output and its incoming gradient (FReLU's depth-wise output is one), every Conv module output and its incoming gradient, and the
BatchNorm output that feeds an AconC or FReLU layer with its incoming gradient are rounded to bf16 (a rounding autograd.Function applied
in forward hooks).  floor.out / floor.grad / floor.run are the worst error of that run against the float64 run, relative to each
tensor's max, over the output / the gradients of x and of every parameter / the running statistics."""
import argparse
import json
import math
import os
import re
import warnings

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
COMMON_RANGES = ((38, 70), (115, 125), (161, 172))
ACT_RANGES = ((53, 78),)

# name -> (class, positional arguments, activation, how, input shape)
CASES = {
    "act_conv_leaky_16_24_k3": ("Conv", (16, 24, 3, 1), "nn.LeakyReLU(0.1)", "arg", (2, 16, 7, 5)),
    "act_conv_hswish_16_24_k1": ("Conv", (16, 24, 1, 1), "nn.Hardswish()", "arg", (2, 16, 7, 5)),
    "act_conv_mish_16_16_k3_s2": ("Conv", (16, 16, 3, 2), "nn.Mish()", "arg", (2, 16, 7, 5)),
    "act_dwconv_hswish_16_16_k3_s2": ("DWConv", (16, 16, 3, 2), "nn.Hardswish()", "default", (2, 16, 7, 5)),
    "act_c3_leaky_32_32_n1": ("C3", (32, 32, 1), "nn.LeakyReLU(0.1)", "default", (2, 32, 8, 6)),
    "act_conv_acon_16_24_k3": ("Conv", (16, 24, 3, 1), "AconC(24)", "arg", (2, 16, 7, 5)),
    "act_conv_frelu_16_24_k3": ("Conv", (16, 24, 3, 1), "FReLU(24)", "arg", (2, 16, 7, 5)),
    "act_conv_acon_16_20_k1": ("Conv", (16, 20, 1, 1), "AconC(20)", "arg", (2, 16, 7, 5)),
}


def load_reference(ref):
    ns = dict(math=math, warnings=warnings, torch=torch, nn=nn, F=F)
    for rel, ranges in ((os.path.join("models", "common.py"), COMMON_RANGES), (os.path.join("utils", "activations.py"), ACT_RANGES)):
        path = os.path.join(ref, rel)
        lines = open(path, encoding="utf-8").read().split("\n")
        for a, b in ranges:
            exec(compile("\n" * (a - 1) + "\n".join(lines[a - 1:b]), path, "exec"), ns)
    return ns


def make_act(ns, spec):
    """the activation module a case's string names, from torch or from the reference's own classes"""
    m = re.match(r"^(nn\.)?(\w+)\((.*)\)$", spec)
    name, args = m.group(2), [json.loads(a) for a in m.group(3).split(",") if a.strip()]
    return (getattr(nn, name) if m.group(1) else ns[name])(*args)


def build(ns, cls, args, act, how):
    if how == "arg":
        return ns[cls](*args, act=make_act(ns, act))
    old = ns["Conv"].default_act
    ns["Conv"].default_act = make_act(ns, act)
    try:
        return ns[cls](*args)
    finally:
        ns["Conv"].default_act = old


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


def bf16_floor(ns, case, before, x, gout, exact):
    mod = build(ns, *case).double().train()
    mod.load_state_dict(before)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(bf16(m.weight))
    for m in mod.modules():
        if isinstance(m, (nn.Conv2d, ns["Conv"])):
            m.register_forward_hook(lambda _m, _i, o: RoundBoth.apply(o))
        if isinstance(m, ns["Conv"]) and isinstance(m.act, (ns["AconC"], ns["FReLU"])):     # the stored BatchNorm output behind it
            m.bn.register_forward_hook(lambda _m, _i, o: RoundBoth.apply(o))
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
    for seed, (name, case) in enumerate(CASES.items()):
        cls, args, act, how, shape = case
        case = case[:4]
        gen = torch.Generator().manual_seed(1500 + seed)
        mod = build(ns, *case).double().train()
        bn = {n for n, m in mod.named_modules() if isinstance(m, nn.BatchNorm2d)}
        with torch.no_grad():
            for key, p in mod.named_parameters():
                owner, leaf = key.rsplit(".", 1)
                if owner in bn:
                    lo, hi = (0.5, 1.5) if leaf == "weight" else (-0.3, 0.3)
                    p.copy_((torch.rand(p.shape, generator=gen, dtype=torch.float64) * (hi - lo) + lo).float().double())
                elif leaf == "beta":
                    p.copy_((torch.rand(p.shape, generator=gen, dtype=torch.float64) + 0.5).float().double())
                elif leaf in ("p1", "p2"):
                    p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64).float().double())
                else:
                    fan_in = p[0].numel()
                    p.copy_((torch.randn(p.shape, generator=gen, dtype=torch.float64) * (fan_in ** -0.5)).float().double())
        before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
        x = torch.randn(*shape, generator=gen, dtype=torch.float64).float().double()
        out_shape = mod.eval()(x).shape
        mod.train()
        gout = torch.randn(out_shape, generator=gen, dtype=torch.float64).float().double()
        exact = run(mod, x, gout)
        floor = bf16_floor(ns, case, before, x, gout, exact)
        keys = list(before.keys())
        arrs = dict(cls=np.array(cls), args=np.array(json.dumps(list(args))), act=np.array(act), how=np.array(how), keys=np.array(keys),
                    x=x.numpy(), grad_out=gout.numpy())
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
