#!/usr/bin/env python3
"""Dev-time generator of tests/golden/tr_*.npz: the reference's OWN TransformerLayer / TransformerBlock / C3TR classes (and through
them torch's nn.MultiheadAttention), run on the CPU in float64, train mode.

    python tools/make_transformer_golden.py --reference <checkout of the reference project> [--out DIR]

Nothing of the reference is copied: the line ranges of models/common.py that hold autopad and Conv (:38-58), TransformerLayer and
TransformerBlock (:79-112), Bottleneck (:115-125), C3 (:161-172) and C3TR (:183-188) are exec'd in a namespace that provides math,
torch and nn.  Only arrays are written, per case:

  cls, args     class name and positional constructor arguments
  keys          the state_dict keys, in order;  p.<key> the parameter or buffer BEFORE the step,  g.<key> a parameter's gradient
  x, out, grad_out, grad_x     (N, C, H, W); a TransformerLayer sees x as the (H*W, N, C) sequence the block would hand it

Weights are drawn ~ N(0, 1/fan_in), every bias (in_proj_bias, out_proj.bias, linear.bias) ~ N(0, 0.5^2) so that a dropped bias or
bias gradient shows; BatchNorm weights are uniform in [0.5, 1.5] and biases in [-0.3, 0.3].  Everything drawn is rounded to float32
first (the f32 GPU path then starts from the same numbers); the reference itself runs in float64.  Parameters (exact in float32)
and their gradients (rounded to float32, 6e-8 relative) are stored as float32, and so are x and grad_out (drawn in float32: exact);
out and grad_x stay float64.  A file holds every parameter and its gradient, 8 bytes per parameter: 9 c^2 weights per layer make
the cases 127 to 384 KB, above the 100 000 bytes the smaller fixture families keep and under the repository's limit of 1 MiB per
committed file (tests/test_mha_ref_cpu.py checks the latter)."""
import math
import os

import numpy as np
import torch
import torch.nn as nn

import golden_blocks as G

RANGES = ((38, 58), (79, 112), (115, 125), (161, 172), (183, 188))

# name -> (class, positional arguments, input shape (N, C, H, W))
CASES = {
    "tr_layer_32_h4": ("TransformerLayer", (32, 4), (2, 32, 7, 5)),
    "tr_block_48_h2_l2": ("TransformerBlock", (48, 48, 2, 2), (2, 48, 5, 4)),
    "tr_block_16_32_h4_conv": ("TransformerBlock", (16, 32, 4, 1), (2, 16, 6, 6)),
    "tr_c3tr_32_64_n1": ("C3TR", (32, 64, 1), (2, 32, 6, 6)),          # c_ = 32: d = 8 (c2 = 32 would give d = 4)
}


def load_reference(ref):
    return G.load_ranges(os.path.join(ref, "models", "common.py"), RANGES, dict(math=math, torch=torch, nn=nn))


def bias_draw(leaf, p, gen):
    if p.dim() == 1:
        return torch.randn(p.shape, generator=gen, dtype=torch.float64) * 0.5


def as_sequence(mod, x):
    """a TransformerLayer sees x as the (H*W, N, C) sequence the block would hand it"""
    return mod(x.flatten(2).permute(2, 0, 1)).permute(1, 2, 0).reshape(x.shape)


def record(ns, seed, case, path):
    cls, args, shape = case
    gen = torch.Generator().manual_seed(400 + seed)
    mod = ns[cls](*args).double().train()
    G.draw_parameters(mod, gen, bias_draw)
    before = G.snapshot(mod)
    call = as_sequence if cls == "TransformerLayer" else None
    x, gout = G.draw_io(mod, shape, gen, call)
    exact = {k: v for k, v in G.run(mod, x, gout, call).items() if G.kind(k) != "run"}          # no running statistics in these files
    G.write_fixture(path, dict(cls=cls, args=np.array(args)), before, x, gout, exact, as_f32=lambda k: k not in ("out", "grad_x"))


if __name__ == "__main__":
    G.main(CASES, load_reference, record)
