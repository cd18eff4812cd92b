#!/usr/bin/env python3
"""Dev-time generator of tests/golden/convnext_*.npz: the plain-torch float64 reference of tests/convnext_ref.py (nn.Conv2d,
F.layer_norm, nn.Linear, exact F.gelu), on the CPU, train mode.

    python tools/make_convnext_golden.py [--out DIR]

torchvision is not needed and not used: the reference restates its ``convnext_tiny`` pieces.  Per case, in the layout of
tools/golden_blocks.py (write_fixture):

  cls, args     "CNBlock" (dim, layer_scale, stochastic_depth_prob), "stem" (c1, c2, k) or "down" (c1, c2), arguments as a JSON list
  keep          the per-sample keep factors of the step (the ``_keep`` case: one sample dropped), absent otherwise
  keys, p.<key>, g.<key>, x, out, grad_out, grad_x
  floor.out, floor.grad    the bf16 floor, see below

Parameters are drawn by tools/golden_blocks.py (weights and biases ~ N(0, 1/fan_in)) except the LayerNorm weights and ``layer_scale``,
uniform in [0.5, 1.5], and the LayerNorm biases, uniform in [-0.3, 0.3]: at the initial layer_scale of 1e-6 an error in the branch would
not show in the output.  Everything is rounded to float32 first; the modules run in float64; arrays are stored as float32.  Full rows
are not stored (1.2 to 15 M parameters): their tests seed the weights and run the reference at test time.

The bf16 floor is the reference's own error under bf16 storage (``store=True``): the image, every GEMM weight on the way forward and
every tensor a bf16 implementation stores (the depth-wise output before its bias, the LayerNorm output, the fc1 output before its
bias, the GELU output, the fc2 output, the block output, a patchify convolution's output) with its incoming gradient are rounded."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import golden_blocks as G                    # noqa: E402
from tests import convnext_ref as R          # noqa: E402

# name -> (class, arguments, input shape, keep factors or None)
CASES = {
    "convnext_cnblock_16": ("CNBlock", (16, 1.0, 0.0), (2, 16, 6, 10), None),
    "convnext_cnblock_24_keep": ("CNBlock", (24, 1.0, 0.5), (2, 24, 5, 7), (0.0, 2.0)),
    "convnext_stem_3_16": ("stem", (3, 16, 4), (2, 3, 12, 20), None),
    "convnext_down_16_32": ("down", (16, 32), (2, 16, 6, 10), None),
}


def make(cls, args, keep, store=False):
    mod = (R.CNBlock(*args, store=store) if cls == "CNBlock" else getattr(R, cls)(*args, store=store)).double().train()
    if keep is not None:
        mod.fixed_keep = torch.tensor(keep, dtype=torch.float64)
    return mod


def special(leaf, p, gen):
    if leaf == "layer_scale" or (leaf == "weight" and p.dim() == 1):
        return torch.rand(p.shape, generator=gen, dtype=torch.float64) + 0.5
    if leaf == "bias" and getattr(p, "_ln", False):
        return torch.rand(p.shape, generator=gen, dtype=torch.float64) * 0.6 - 0.3
    return None


def draw(mod, gen):
    for m in mod.modules():
        if isinstance(m, (torch.nn.LayerNorm, R.LayerNorm2d)):
            m.bias._ln = True
    G.draw_parameters(mod, gen, special)


def record(seed, case, path):
    cls, args, shape, keep = case
    gen = torch.Generator().manual_seed(1700 + seed)
    mod = make(cls, args, keep)
    draw(mod, gen)
    before = G.snapshot(mod)
    x, gout = G.draw_io(mod, shape, gen)
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
