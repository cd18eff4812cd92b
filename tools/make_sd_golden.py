#!/usr/bin/env python3
"""Dev-time generator of tests/golden/sd_*.npz: the reference's OWN Focus, Contract, Expand and BottleneckCSP classes and torch's
nn.BatchNorm2d, run on the CPU in float64, train mode.

    python tools/make_sd_golden.py --reference <checkout of the reference project> [--out DIR]

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad and Conv (:38-64), Bottleneck (:115-125),
BottleneckCSP (:128-144), Focus (:241-250) and Contract and Expand (:282-307) are exec'd in a namespace that provides math, warnings,
torch and nn.  Only arrays are written, per case, in the layout of tools/golden_blocks.py (write_fixture):

  cls, args     class name and the positional constructor arguments as a JSON list
  keys          the state_dict keys, in order (none for Contract / Expand);  p.<key> the parameter or buffer BEFORE the step,
                g.<key> a parameter's gradient
  x, out, grad_out, grad_x
  rm.<key>, rv.<key>   running_mean / running_var AFTER the one train-mode forward
  floor.out, floor.grad, floor.run     the bf16 floor, see below (floor.run where there are running statistics)

Parameters are drawn by tools/golden_blocks.py (weights ~ N(0, 1/fan_in); BatchNorm weights uniform in [0.5, 1.5], biases in
[-0.3, 0.3]) and rounded to float32 first; the modules run in float64; arrays are stored as float32.

The bf16 floor is the module's own error when its tensors pass through bf16 where a bf16 implementation stores them: the same module
with the same parameters is run a second time, everything in float64 except that the input, every nn.Conv2d weight, every nn.Conv2d
output and its incoming gradient, every Conv module output and its incoming gradient, BottleneckCSP's activated concat (the output of
its ``act``) and the output of a module that has no convolution (Contract, Expand, BatchNorm2d) are rounded to bf16."""
import json
import math
import os
import warnings

import torch
import torch.nn as nn

import golden_blocks as G

RANGES = ((38, 64), (115, 125), (128, 144), (241, 250), (282, 307))

# name -> (class, positional arguments, input shape)
CASES = {
    "sd_focus_3_16_k3": ("Focus", (3, 16, 3), (2, 3, 12, 20)),
    "sd_focus_8_24_k1": ("Focus", (8, 24, 1), (2, 8, 8, 12)),
    "sd_contract_g2_c12": ("Contract", (2,), (2, 12, 8, 12)),
    "sd_contract_g4_c8": ("Contract", (4,), (2, 8, 8, 12)),
    "sd_expand_g2_c32": ("Expand", (2,), (2, 32, 5, 7)),
    "sd_expand_g2_c48": ("Expand", (2,), (2, 48, 5, 7)),
    "sd_csp_32_32_n1": ("BottleneckCSP", (32, 32, 1), (2, 32, 8, 8)),
    "sd_csp_16_32_n2_noadd": ("BottleneckCSP", (16, 32, 2, False), (2, 16, 8, 8)),
    "sd_bn_24": ("BatchNorm2d", (24,), (2, 24, 5, 7)),
}


def load_reference(ref):
    ns = G.load_ranges(os.path.join(ref, "models", "common.py"), RANGES, dict(math=math, warnings=warnings, torch=torch, nn=nn))
    ns["BatchNorm2d"] = nn.BatchNorm2d
    return ns


def record(ns, seed, case, path):
    cls, args, shape = case

    def make():
        return ns[cls](*args).double().train()

    def rounded(before):
        mod = make()
        mod.load_state_dict(before)
        G.round_convs(mod, ns["Conv"])
        if cls == "BottleneckCSP":
            G.round_output(mod.act)
        elif cls in ("Contract", "Expand", "BatchNorm2d"):
            G.round_output(mod)
        return mod
    G.record_module(path, torch.Generator().manual_seed(1600 + seed), make, shape, dict(cls=cls, args=json.dumps(list(args))), rounded=rounded)


if __name__ == "__main__":
    G.main(CASES, load_reference, record)
