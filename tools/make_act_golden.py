#!/usr/bin/env python3
"""Dev-time generator of tests/golden/act_*.npz: the reference's OWN Conv, DWConv and C3 classes under other activations than SiLU, and
its own AconC and FReLU layers, run on the CPU in float64, train mode.

    python tools/make_act_golden.py --reference <checkout of the reference project> [--out DIR]

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad, Conv and DWConv (:38-70), Bottleneck
(:115-125) and C3 (:161-172), and those of utils/activations.py that hold FReLU and AconC (:53-78), are exec'd in a namespace that
provides math, warnings, torch, nn and F.  Only arrays are written, per case, in the layout of tools/golden_blocks.py (write_fixture):

  cls, args     class name and the positional constructor arguments as a JSON list
  act, how      the activation as a string and how the module gets it: "arg" as the constructor's ``act=`` argument, "default" as
                ``Conv.default_act`` while the module is built.  The point-wise strings are what a yaml's ``activation:`` key holds
                (yolo_dual_amd.resolve_activation reads them); "AconC(c)" / "FReLU(c)" name the class and its channel count
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x
  rm.<key>, rv.<key>   running_mean / running_var AFTER the one train-mode forward
  floor.out, floor.grad, floor.run     the bf16 floor, see below

Parameters are drawn by tools/golden_blocks.py (weights ~ N(0, 1/fan_in); BatchNorm weights uniform in [0.5, 1.5], biases in [-0.3, 0.3]; AconC's p1, p2
~ N(0, 1) and beta uniform in [0.5, 1.5]) and rounded to float32 first; the reference itself runs in float64; arrays are stored as
float32.

The bf16 floor is the reference's own error when its tensors pass through bf16 where a bf16 implementation stores them: the same module
with the same parameters is run a second time, everything in float64 except that the input, every nn.Conv2d weight, every nn.Conv2d
output and its incoming gradient (FReLU's depth-wise output is one), every Conv module output and its incoming gradient, and the
BatchNorm output that feeds an AconC or FReLU layer with its incoming gradient are rounded to bf16 (a rounding autograd.Function applied
in forward hooks).  floor.out / floor.grad / floor.run are the worst error of that run against the float64 run, relative to each
tensor's max, over the output / the gradients of x and of every parameter / the running statistics."""
import json
import math
import os
import re
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

import golden_blocks as G

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
    G.load_ranges(os.path.join(ref, "models", "common.py"), COMMON_RANGES, ns)
    return G.load_ranges(os.path.join(ref, "utils", "activations.py"), ACT_RANGES, ns)


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


def acon_draw(leaf, p, gen):
    """AconC's beta uniform in [0.5, 1.5], p1 and p2 ~ N(0, 1)"""
    if leaf == "beta":
        return torch.rand(p.shape, generator=gen, dtype=torch.float64) + 0.5
    if leaf in ("p1", "p2"):
        return torch.randn(p.shape, generator=gen, dtype=torch.float64)


def record(ns, seed, case, path):
    cls, args, act, how, shape = case

    def make():
        return build(ns, cls, args, act, how).double().train()

    def rounded(before):
        mod = make()
        mod.load_state_dict(before)
        for m in mod.modules():
            if isinstance(m, ns["Conv"]) and isinstance(m.act, (ns["AconC"], ns["FReLU"])):     # the stored BatchNorm output behind it
                G.round_output(m.bn)
        return G.round_convs(mod, ns["Conv"])
    G.record_module(path, torch.Generator().manual_seed(1500 + seed), make, shape, dict(cls=cls, args=json.dumps(list(args)), act=act, how=how),
                    draw=lambda mod, gen: G.draw_parameters(mod, gen, acon_draw), rounded=rounded)


if __name__ == "__main__":
    G.main(CASES, load_reference, record)
