#!/usr/bin/env python3
"""Dev-time generator of tests/golden/se_*.npz: the plain-torch float64 reference of tests/se_ref.py (nn.Conv2d, nn.BatchNorm2d,
F.adaptive_avg_pool2d, F.hardsigmoid, F.silu), on the CPU, train mode.

    python tools/make_se_golden.py [--out DIR]

torchvision is not needed and not used: the reference restates its SqueezeExcitation, InvertedResidual and MBConv.  Per case, in the
layout of tools/golden_blocks.py (write_fixture):

  cls, args     "SqueezeExcitation", "InvertedResidual" or "MBConv" with the arguments of yolo_dual_amd's class as a JSON list
  keep          the per-sample keep factors of the step (the ``_keep`` case: one sample dropped), absent otherwise
  keys, p.<key>, g.<key>, rm.<key>, rv.<key>, x, out, grad_out, grad_x
  floor.out, floor.grad, floor.run    the bf16 floor: the reference's own error under bf16 storage (``store=True``)

Parameters are drawn by tools/golden_blocks.py (BatchNorm weights uniform in [0.5, 1.5], biases in [-0.3, 0.3], weights ~ N(0, 1/fan_in))
except the SE parameters: fc weights ~ N(0, 4 / fan_in), fc1 biases ~ N(0, 0.5^2) and fc2 biases ~ N(0, 2^2), so that every branch is
taken: the generator asserts that some hidden units are dead and some alive (ReLU), that hardsigmoid arguments lie below -3, inside
(-3, 3) and above 3, and that no |z| lies within 1e-3 of 3.  Everything is rounded to float32 first; the modules run in float64."""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import golden_blocks as G                    # noqa: E402
from tests import se_ref as R                # noqa: E402

# name -> (class, arguments, input shape, keep factors or None)
CASES = {
    "se_gate_16_8_hsig": ("SqueezeExcitation", (16, 8, "relu", "hardsigmoid"), (2, 16, 6, 10), None),
    "se_gate_96_4_sig": ("SqueezeExcitation", (96, 4, "silu", "sigmoid"), (2, 96, 3, 5), None),
    "se_ir_16_s2": ("InvertedResidual", (16, 3, 16, 16, True, "RE", 2), (2, 16, 7, 9), None),
    "se_ir_40_res": ("InvertedResidual", (40, 5, 240, 40, True, "HS", 1), (2, 40, 5, 6), None),
    "se_mbconv_24_40_s2": ("MBConv", (6, 5, 2, 24, 40), (2, 24, 6, 10), None),
    "se_mbconv_24_keep": ("MBConv", (6, 3, 1, 24, 24, 0.5), (2, 24, 5, 7), (0.0, 2.0)),
}


def make(cls, args, keep, store=False):
    mod = getattr(R, cls)(*args, store=store).double().train()
    if keep is not None:
        mod.fixed_keep = torch.tensor(keep, dtype=torch.float64)
    return mod


def special(leaf, p, gen):
    kind = getattr(p, "_se", None)
    if kind is None:
        return None
    if leaf == "weight":
        return torch.randn(p.shape, generator=gen, dtype=torch.float64) * 2.0 * p[0].numel() ** -0.5
    return torch.randn(p.shape, generator=gen, dtype=torch.float64) * (0.5 if kind == 1 else 2.0)


def draw(mod, gen):
    for m in mod.modules():
        if isinstance(m, R.SqueezeExcitation):
            for i, fc in ((1, m.fc1), (2, m.fc2)):
                fc.weight._se = fc.bias._se = i
    G.draw_parameters(mod, gen, special)


def regimes(mod, x):
    """the SE gates' hidden values h and arguments z of the step, by hooks"""
    seen = []
    hooks = [m.fc1.register_forward_hook(lambda _m, _i, o: seen.append(("h", o.detach()))) for m in mod.modules() if isinstance(m, R.SqueezeExcitation)]
    hooks += [m.fc2.register_forward_hook(lambda _m, _i, o: seen.append(("z", o.detach()))) for m in mod.modules() if isinstance(m, R.SqueezeExcitation)]
    with torch.no_grad():
        copy.deepcopy(mod)(x)       # the hooks are copied with the module; the copy runs, so ``mod``'s running statistics see one forward
    for h in hooks:
        h.remove()
    return seen


def record(seed, case, path):
    cls, args, shape, keep = case
    gen = torch.Generator().manual_seed(2310 + seed)
    mod = make(cls, args, keep)
    draw(mod, gen)
    before = G.snapshot(mod)
    x, gout = G.draw_io(mod, shape, gen)
    se = [m for m in mod.modules() if isinstance(m, R.SqueezeExcitation)][0]
    for what, v in regimes(mod, x):
        if what == "h" and se.act == "relu":
            assert bool((v < 0).any()) and bool((v > 0).any()), "dead and live ReLU units"
        if what == "z" and se.gate == "hardsigmoid":
            assert bool((v < -3).any()) and bool((v > 3).any()) and bool((v.abs() < 3).any()), "hardsigmoid regimes"
            assert float(((v.abs() - 3).abs()).min()) > 1e-3, "a hardsigmoid argument within 1e-3 of a corner"
    exact = G.run(mod, x, gout)

    def rounded(state):
        m = make(cls, args, keep, store=True)
        m.load_state_dict(state)
        return m
    floor = G.bf16_floor(rounded, before, x, gout, exact)
    meta = dict(cls=cls, args=json.dumps(list(args)))
    if keep is not None:
        meta["keep"] = torch.tensor(keep, dtype=torch.float32).numpy()
    G.write_fixture(path, meta, before, x, gout, exact, floor)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=G.OUT, help="directory the .npz files are written to")
    opt = ap.parse_args()
    os.makedirs(opt.out, exist_ok=True)
    for seed, (name, case) in enumerate(CASES.items()):
        record(seed, case, os.path.join(opt.out, name + ".npz"))
