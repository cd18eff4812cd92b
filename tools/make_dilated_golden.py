#!/usr/bin/env python3
"""Dev-time generator of tests/golden/dil_*.npz: the reference's OWN Conv (dilated), BasicConv, RFB and ASPP classes, run on the CPU
in float64, train mode.

    python tools/make_dilated_golden.py --reference <checkout of the reference project> [--out DIR]

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad and Conv (:38-64), ASPP (:1336-1361),
BasicConv (:1366-1384) and RFB (:1386-1425) are exec'd in a namespace that provides math, torch, nn and F.  Only arrays are written,
per case:

  cls, args     class name and the positional constructor arguments as a JSON list (Conv's padding is None)
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x
  rm.<key>, rv.<key>   running_mean / running_var AFTER the one train-mode forward (the cases that hold a BatchNorm)

Parameters are drawn by tools/golden_blocks.py (weights and convolution biases ~ N(0, 1/fan_in)); BatchNorm weights are
uniform in [0.5, 1.5] and biases in [-0.3, 0.3].  Everything drawn is rounded to float32 first (the f32 GPU path then starts from
the same numbers); the reference itself runs in float64.  Arrays are stored as float32: exact for what was drawn, a rounding of 6e-8
for the results, far below the 1e-4 the fixtures are compared at, and half the bytes (the RFB case has 17k parameters)."""
import json
import math
import os
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

import golden_blocks as G

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
    warnings.filterwarnings("ignore", category=UserWarning)        # F.upsample is deprecated spelling of F.interpolate
    return G.load_ranges(os.path.join(ref, "models", "common.py"), RANGES, dict(math=math, torch=torch, nn=nn, F=F))


def record(ns, seed, case, path):
    cls, args, shape = case
    G.record_module(path, torch.Generator().manual_seed(700 + seed), lambda: ns[cls](*args).double().train(), shape,
                    dict(cls=cls, args=json.dumps(list(args))))


if __name__ == "__main__":
    G.main(CASES, load_reference, record)
