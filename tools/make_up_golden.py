#!/usr/bin/env python3
"""Dev-time generator of tests/golden/up_*.npz: the decoder up-samplers run on the CPU in float64 — ``nn.ConvTranspose2d`` and
``nn.Upsample(mode='bicubic')`` from torch, ``DWConvTranspose2d`` from the reference's OWN class.

    python tools/make_up_golden.py --reference <checkout of the reference project>

Nothing of the reference is copied: the lines of models/common.py that hold DWConvTranspose2d (:73-76) are exec'd in a namespace that
provides math, torch and nn.  Only arrays are written, per case, in the layout of tools/make_cross_golden.py:

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
import argparse
import json
import math
import os

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
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
    path = os.path.join(ref, "models", "common.py")
    lines = open(path, encoding="utf-8").read().split("\n")
    ns = dict(math=math, torch=torch, nn=nn)
    for a, b in RANGES:
        exec(compile("\n" * (a - 1) + "\n".join(lines[a - 1:b]), path, "exec"), ns)
    ns["ConvTranspose2d"], ns["Upsample"] = nn.ConvTranspose2d, nn.Upsample
    return ns


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
    x = x.clone().requires_grad_(True)
    out = mod(x)
    out.backward(gout)
    res = {"out": out.detach(), "grad_x": x.grad}
    for key, p in mod.named_parameters():
        res["g." + key] = p.grad
    return res


def bf16_floor(make, before, x, gout, exact):
    mod = make()
    mod.load_state_dict(before)
    with torch.no_grad():
        if getattr(mod, "weight", None) is not None:
            mod.weight.copy_(bf16(mod.weight))
    mod.register_forward_hook(lambda _m, _i, o: RoundBoth.apply(o))
    got = run(mod, bf16(x), gout)
    floor = {"out": 0.0, "grad": 0.0}
    for k, want in exact.items():
        kind = "out" if k == "out" else "grad"
        scale = float(want.abs().max())
        floor[kind] = max(floor[kind], float((got[k] - want).abs().max()) / (scale if scale > 0 else 1.0))
    return floor


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    opt = ap.parse_args()
    ns = load_reference(opt.reference)
    os.makedirs(OUT, exist_ok=True)
    for seed, (name, (cls, args, kwargs, shape)) in enumerate(CASES.items()):
        gen = torch.Generator().manual_seed(1500 + seed)

        def make():
            return ns[cls](*args, **kwargs).double().train()
        mod = make()
        with torch.no_grad():
            for key, p in mod.named_parameters():
                if key == "weight":
                    k = p.shape[-1]
                    terms = ((k + 1) // 2) ** 2 * (p.shape[0] if mod.groups == 1 else 1)
                    p.copy_((torch.randn(p.shape, generator=gen, dtype=torch.float64) * terms ** -0.5).float().double())
                else:
                    p.copy_((torch.rand(p.shape, generator=gen, dtype=torch.float64) * 0.6 - 0.3).float().double())
        before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
        x = torch.randn(*shape, generator=gen, dtype=torch.float64).float().double()
        out_shape = mod(x).shape
        gout = torch.randn(out_shape, generator=gen, dtype=torch.float64).float().double()
        exact = run(mod, x, gout)
        floor = bf16_floor(make, before, x, gout, exact)
        keys = list(before.keys())
        arrs = dict(cls=np.array(cls), args=np.array(json.dumps(list(args))), kwargs=np.array(json.dumps(kwargs)), keys=np.array(keys, dtype=str),
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
        print(f"{path}: {os.path.getsize(path)} bytes, out {tuple(out_shape)}, {len(keys)} keys, floor "
              + ", ".join(f"{k} {v:.2e}" for k, v in floor.items()))


if __name__ == "__main__":
    main()
