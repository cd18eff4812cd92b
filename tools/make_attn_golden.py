#!/usr/bin/env python3
"""Dev-time generator of tests/golden/attn_conv_*.npz and attn_stem_*.npz: the reference's OWN AttentionConv / AttentionStem
classes, run on the CPU in float64.

    python tools/make_attn_golden.py --reference <checkout of the reference project> [--out DIR]

Nothing of the reference is copied: the line range of models/common.py that holds the two classes (:1509-1627) is exec'd in a
namespace that provides torch, nn and F.  Only arrays are written, per case:

  args          (in_channels, out_channels, kernel_size, stride, padding, groups, m)   (m = 0 for AttentionConv)
  keys          the state_dict keys, in order;  p.<key> the parameter,  g.<key> its gradient
  x, out, grad_out, grad_x

Inputs keep |logit| below about 4: x, rel_* and emb_* ~ N(0, 1), projection weights ~ N(0, 1/c1)."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

import golden_blocks as G

RANGES = ((1509, 1627),)

# name -> (class, constructor arguments, (N, H, W))
CASES = {
    "attn_conv_16_24_k3": ("AttentionConv", dict(in_channels=16, out_channels=24, kernel_size=3, stride=1, padding=1, groups=1), (2, 7, 5)),
    "attn_conv_8_16_k5_g4": ("AttentionConv", dict(in_channels=8, out_channels=16, kernel_size=5, stride=1, padding=2, groups=4), (2, 6, 6)),
    "attn_stem_16_24_k3_m4": ("AttentionStem", dict(in_channels=16, out_channels=24, kernel_size=3, stride=1, padding=1, groups=1, m=4),
                              (2, 7, 5)),
    "attn_stem_8_8_k3_m1_g2": ("AttentionStem", dict(in_channels=8, out_channels=8, kernel_size=3, stride=1, padding=1, groups=2, m=1),
                               (2, 5, 4)),
}


def load_reference(ref):
    return G.load_ranges(os.path.join(ref, "models", "common.py"), RANGES, dict(torch=torch, nn=nn, F=F))


def record(ns, seed, case, path):
    cls, kw, (N, H, W) = case
    gen = torch.Generator().manual_seed(100 + seed)
    mod = ns[cls](**kw).double()
    c1 = kw["in_channels"]
    with torch.no_grad():                               # this family's own draw, in float64 throughout
        for key, p in mod.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64) * (c1 ** -0.5 if key.endswith(".weight") else 1.0))
    x = torch.randn(N, c1, H, W, generator=gen, dtype=torch.float64)
    gout = torch.randn(G.out_shape(mod, x), generator=gen, dtype=torch.float64)
    args = [c1, kw["out_channels"], kw["kernel_size"], kw["stride"], kw["padding"], kw["groups"], kw.get("m", 0)]
    G.write_fixture(path, dict(args=args), G.snapshot(mod), x, gout, G.run(mod, x, gout), as_f32=lambda k: False)
    print(f"  |logit| proxy max|x| {float(x.abs().max()):.2f}")


if __name__ == "__main__":
    G.main(CASES, load_reference, record)
