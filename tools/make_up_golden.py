#!/usr/bin/env python3
"""Dev-time generator of tests/golden/up_*.npz: the decoder up-samplers run on the CPU in float64 — ``nn.ConvTranspose2d`` and
``nn.Upsample(mode='bicubic')`` from torch, ``DWConvTranspose2d`` from the reference's OWN class.

    python tools/make_up_golden.py --reference <checkout of the reference project> [--out DIR]

Nothing of the reference is copied: the lines of models/common.py that hold DWConvTranspose2d (:73-76) are exec'd in a namespace that
provides math, torch and nn.  Only arrays are written, per case, in the layout of tools/golden_blocks.py (write_fixture):

  cls, args, kwargs   class name, the positional constructor arguments and the keyword arguments as JSON
  keys                the state_dict keys, in order;  p.<key> the parameter BEFORE the step,  g.<key> its gradient
  x, out, grad_out, grad_x
  floor.out, floor.grad     the bf16 floor, see below (there are no running statistics)

Weights are drawn ~ N(0, 1 / (ceil(k/2)^2 * channels summed per output)), biases uniform in [-0.3, 0.3], rounded to float32 first; the
modules run in float64; arrays are stored as float32.

The bf16 floor is the module's own error when its tensors pass through bf16 where a bf16 implementation stores them: the same module
with the same parameters run a second time in float64, with the input, the weight, the output and its incoming gradient rounded to
bf16.  floor.out / floor.grad are the worst error of that run against the float64 run, relative to each tensor's max, over the output /
the gradients of x and of every parameter."""
import json
import math
import os

import torch
import torch.nn as nn

import golden_blocks as G

RANGES = ((73, 76),)

# name -> (class, positional arguments, keyword arguments, input shape)
CASES = {
    "up_tconv_16_24_k2": ("ConvTranspose2d", (16, 24, 2, 2), {}, (2, 16, 5, 7)),
    "up_tconv_16_16_k4_nobias": ("ConvTranspose2d", (16, 16, 4, 2, 1), {"bias": False}, (2, 16, 5, 7)),
    "up_tconv_24_8_k3": ("ConvTranspose2d", (24, 8, 3, 2, 1, 1), {}, (2, 24, 5, 7)),
    "up_dwtconv_16_k4": ("DWConvTranspose2d", (16, 16, 4, 2, 1, 0), {}, (2, 16, 5, 7)),
    "up_dwtconv_24_k2": ("DWConvTranspose2d", (24, 24, 2, 2, 0, 0), {}, (2, 24, 5, 7)),
    "up_bicubic_x2": ("Upsample", (None, 2.0, "bicubic"), {}, (2, 16, 5, 7)),
    "up_bicubic_7x10_ac": ("Upsample", ((7, 10), None, "bicubic", True), {}, (2, 16, 5, 7)),
}


def load_reference(ref):
    ns = G.load_ranges(os.path.join(ref, "models", "common.py"), RANGES, dict(math=math, torch=torch, nn=nn))
    ns["ConvTranspose2d"], ns["Upsample"] = nn.ConvTranspose2d, nn.Upsample
    return ns


def draw(mod, gen):
    with torch.no_grad():
        for key, p in mod.named_parameters():
            if key == "weight":
                k = p.shape[-1]
                terms = ((k + 1) // 2) ** 2 * (p.shape[0] if mod.groups == 1 else 1)
                p.copy_(G.f32(torch.randn(p.shape, generator=gen, dtype=torch.float64) * terms ** -0.5))
            else:
                p.copy_(G.f32(torch.rand(p.shape, generator=gen, dtype=torch.float64) * 0.6 - 0.3))


def record(ns, seed, case, path):
    cls, args, kwargs, shape = case

    def make():
        return ns[cls](*args, **kwargs).double().train()

    def rounded(before):
        mod = make()
        mod.load_state_dict(before)
        with torch.no_grad():
            if getattr(mod, "weight", None) is not None:
                mod.weight.copy_(G.bf16(mod.weight))
        G.round_output(mod)
        return mod
    G.record_module(path, torch.Generator().manual_seed(1500 + seed), make, shape,
                    dict(cls=cls, args=json.dumps(list(args)), kwargs=json.dumps(kwargs)), draw=draw, rounded=rounded)


if __name__ == "__main__":
    G.main(CASES, load_reference, record)
