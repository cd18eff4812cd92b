#!/usr/bin/env python3
"""Dev-time generator of tests/golden/gconv_*.npz: the reference's OWN Conv (with groups) and SPPCSPC_group classes, run on the CPU in
float64, train mode.

    python tools/make_gconv_golden.py --reference <checkout of the reference project> [--out DIR]

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad and Conv (:38-64) and SPPCSPC_group
(:1451-1468) are exec'd in a namespace that provides math, warnings, torch and nn.  Only arrays are written, per case, in the layout
of tools/golden_blocks.py (write_fixture):

  cls, args     class name and the positional constructor arguments as a JSON list
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x
  rm.<key>, rv.<key>   running_mean / running_var AFTER the one train-mode forward

Parameters are drawn as there (weights ~ N(0, 1/fan_in) with the fan-in of ONE group; BatchNorm weights uniform in [0.5, 1.5], biases
in [-0.3, 0.3]) and rounded to float32 first; the reference itself runs in float64; arrays are stored as float32."""
import json
import math
import os
import warnings

import torch
import torch.nn as nn

import golden_blocks as G

RANGES = ((38, 64), (1451, 1468))

# name -> (class, positional arguments, input shape)
CASES = {
    "gconv_sppcspc_group_64_64": ("SPPCSPC_group", (64, 64), (2, 64, 9, 7)),        # seven Conv(g=4): 16 -> 16 and 64 -> 16 per group
    "gconv_conv_32_96_g2_k3": ("Conv", (32, 96, 3, 1, None, 2), (2, 32, 7, 5)),     # 16 -> 48 per group
}


def load_reference(ref):
    return G.load_ranges(os.path.join(ref, "models", "common.py"), RANGES, dict(math=math, warnings=warnings, torch=torch, nn=nn))


def record(ns, seed, case, path):
    cls, args, shape = case
    G.record_module(path, torch.Generator().manual_seed(1300 + seed), lambda: ns[cls](*args).double().train(), shape,
                    dict(cls=cls, args=json.dumps(list(args))))


if __name__ == "__main__":
    G.main(CASES, load_reference, record)
