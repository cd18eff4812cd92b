#!/usr/bin/env python3
"""Dev-time generator of tests/golden/cross_*.npz: the reference's OWN Conv (with a (1, k) / (k, 1) kernel), CrossConv and C3x classes,
run on the CPU in float64, train mode.

    python tools/make_cross_golden.py --reference <checkout of the reference project> [--out DIR]

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad and Conv (:38-64), Bottleneck (:115-125, C3's
constructor needs it) and CrossConv, C3 and C3x (:147-180) are exec'd in a namespace that provides math, warnings, torch and nn.  Only
arrays are written, per case, in the layout of tools/golden_blocks.py (write_fixture):

  cls, args     class name and the positional constructor arguments as a JSON list
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x
  rm.<key>, rv.<key>   running_mean / running_var AFTER the one train-mode forward
  floor.out, floor.grad, floor.run     the bf16 floor, see below

Parameters are drawn by tools/golden_blocks.py (weights ~ N(0, 1/fan_in); BatchNorm weights uniform in [0.5, 1.5], biases in [-0.3, 0.3]) and rounded to
float32 first; the reference itself runs in float64; arrays are stored as float32.

The bf16 floor is the reference's own error when its tensors pass through bf16 where a bf16 implementation stores them: the same module
with the same parameters is run a second time, everything in float64 except that the input, every nn.Conv2d weight, every nn.Conv2d
output and its incoming gradient, and every Conv module output and its incoming gradient are rounded to bf16 (a rounding
autograd.Function applied in forward hooks).  floor.out / floor.grad / floor.run are the worst error of that run against the float64
run, relative to each tensor's max, over the output / the gradients of x and of every parameter / the running statistics."""
import json
import math
import os
import warnings

import torch
import torch.nn as nn

import golden_blocks as G

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
    return G.load_ranges(os.path.join(ref, "models", "common.py"), RANGES, dict(math=math, warnings=warnings, torch=torch, nn=nn))


def record(ns, seed, case, path):
    cls, args, shape = case

    def make():
        return ns[cls](*args).double().train()

    def rounded(before):
        mod = make()
        mod.load_state_dict(before)
        return G.round_convs(mod, ns["Conv"])
    G.record_module(path, torch.Generator().manual_seed(1400 + seed), make, shape, dict(cls=cls, args=json.dumps(list(args))), rounded=rounded)


if __name__ == "__main__":
    G.main(CASES, load_reference, record)
