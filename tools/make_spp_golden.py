#!/usr/bin/env python3
"""Dev-time generator of tests/golden/spp_*.npz: the reference's OWN SPP, C3SPP, SimSPPF, SPPCSPC and SimCSPSPPF classes, run on the
CPU in float64, train mode.

    python tools/make_spp_golden.py --reference <checkout of the reference project> [--out DIR]

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad and Conv (:38-64), Bottleneck (:115-125),
C3 (:161-172), C3SPP (:191-197), SPP (:1275-1286), SimConv and SimSPPF (:1292-1330), SPPCSPC (:1430-1448) and SimCSPSPPF
(:1473-1492) are exec'd in a namespace that provides math, warnings, torch and nn.  Only arrays are written, per case:

  cls, args     class name and the positional constructor arguments as a JSON list
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x
  rm.<key>, rv.<key>   running_mean / running_var AFTER the one train-mode forward

Parameters are drawn by tools/golden_blocks.py (weights ~ N(0, 1/fan_in); BatchNorm weights uniform in [0.5, 1.5], biases in
[-0.3, 0.3]).  Everything drawn is rounded to float32 first (the f32 GPU path then starts from the same numbers); the reference itself
runs in float64.  Arrays are stored as float32: exact for what was drawn, a rounding of 6e-8 for the results, far below the 1e-4 the
fixtures are compared at."""
import json
import math
import os
import warnings

import torch
import torch.nn as nn

import golden_blocks as G

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
    return G.load_ranges(os.path.join(ref, "models", "common.py"), RANGES, dict(math=math, warnings=warnings, torch=torch, nn=nn))


def record(ns, seed, case, path):
    cls, args, shape = case
    G.record_module(path, torch.Generator().manual_seed(900 + seed), lambda: ns[cls](*args).double().train(), shape,
                    dict(cls=cls, args=json.dumps(list(args))))


if __name__ == "__main__":
    G.main(CASES, load_reference, record)
