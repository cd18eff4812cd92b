#!/usr/bin/env python3
"""Dev-time generator of tests/golden/ghost_*.npz: the reference's OWN DWConv / GhostConv / GhostBottleneck / C3Ghost classes, run
on the CPU in float64, train mode.

    python tools/make_ghost_golden.py --reference <checkout of the reference project> [--out DIR]

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad, Conv and DWConv (:38-70), Bottleneck
(:115-125), C3 (:161-172), C3Ghost (:199-204) and GhostConv / GhostBottleneck (:253-279) are exec'd in a namespace that provides
math, torch and nn.  Only arrays are written, per case:

  cls, args     class name and positional constructor arguments
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x
  rm.<key>, rv.<key>   running_mean / running_var AFTER the one train-mode forward

Parameters are drawn by tools/golden_blocks.py (weights ~ N(0, 1/fan_in)); BatchNorm weights are uniform in [0.5, 1.5] and
biases in [-0.3, 0.3], so that no channel's batch variance is near zero.  Everything drawn is rounded to float32 first (the f32 GPU
path then starts from the same numbers, and the files compress to under 100 KB); the reference itself runs in float64."""
import math
import os

import numpy as np
import torch
import torch.nn as nn

import golden_blocks as G

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
    return G.load_ranges(os.path.join(ref, "models", "common.py"), RANGES, dict(math=math, torch=torch, nn=nn))


def record(ns, seed, case, path):
    cls, args, kw, shape = case
    G.record_module(path, torch.Generator().manual_seed(300 + seed), lambda: ns[cls](*args, **kw).double().train(), shape,
                    dict(cls=cls, args=np.array(args), act=int(kw.get("act", True))), as_f32=lambda k: False)      # stored as float64


if __name__ == "__main__":
    G.main(CASES, load_reference, record)
