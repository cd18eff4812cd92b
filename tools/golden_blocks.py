"""The shared half of the block-family fixture generators (tools/make_*_golden.py, all but make_aug_golden.py).

A generator keeps what is its own -- its docstring, the line ranges of the reference it execs, its CASES, its seed base and any special
construction -- and takes from here: the exec of line ranges, the parameter draw, the one train-mode step, the bf16 floor, the npz layout
and the command line.  Nothing of the reference is copied: its text is exec'd at run time and only arrays are written.

The fixtures depend on the ORDER of the draws from the generator: parameters in ``named_parameters`` order, then x, then grad_out."""
import argparse
import copy
import os

import numpy as np
import torch
import torch.nn as nn

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def load_ranges(path, ranges, ns):
    """exec the 1-based inclusive line ranges of ``path`` in the namespace ``ns`` (line numbers kept for tracebacks)"""
    lines = open(path, encoding="utf-8").read().split("\n")
    for a, b in ranges:
        exec(compile("\n" * (a - 1) + "\n".join(lines[a - 1:b]), path, "exec"), ns)
    return ns


def f32(t):
    """rounded through float32: the f32 GPU path then starts from the same numbers"""
    return t.float().double()


def draw_parameters(mod, gen, special=None):
    """BatchNorm weights uniform in [0.5, 1.5] and biases in [-0.3, 0.3]; everything else ~ N(0, 1/fan_in) with the fan-in of its layer's
    weight (of the tensor itself where the layer has none), unless ``special(leaf, p, gen)`` returns a draw of its own.  Rounded through
    float32."""
    named = dict(mod.named_parameters())
    bn = {n for n, m in mod.named_modules() if isinstance(m, nn.BatchNorm2d)}
    with torch.no_grad():
        for key, p in named.items():
            owner, _, leaf = key.rpartition(".")
            if owner in bn:
                lo, hi = (0.5, 1.5) if leaf == "weight" else (-0.3, 0.3)
                v = torch.rand(p.shape, generator=gen, dtype=torch.float64) * (hi - lo) + lo
            else:
                v = special(leaf, p, gen) if special is not None else None
                if v is None:
                    fan_in = named.get(owner + ".weight", p)[0].numel()
                    v = torch.randn(p.shape, generator=gen, dtype=torch.float64) * (fan_in ** -0.5)
            p.copy_(f32(v))


def snapshot(mod):
    return {k: v.detach().clone() for k, v in mod.state_dict().items()}


def out_shape(mod, x, call=None):
    """the output's shape, from a copy of the module: the running statistics of ``mod`` see one forward only"""
    m = copy.deepcopy(mod)
    with torch.no_grad():
        return (m(x) if call is None else call(m, x)).shape


def draw_io(mod, shape, gen, call=None):
    x = f32(torch.randn(*shape, generator=gen, dtype=torch.float64))
    return x, f32(torch.randn(out_shape(mod, x, call), generator=gen, dtype=torch.float64))


def run(mod, x, gout, call=None):
    """one train-mode forward + backward -> tensors by the fixture's names"""
    x = x.clone().requires_grad_(True)
    out = mod(x) if call is None else call(mod, x)
    out.backward(gout)
    res = {"out": out.detach(), "grad_x": x.grad}
    for key, p in mod.named_parameters():
        res["g." + key] = p.grad
    for key, v in mod.state_dict().items():
        if key.endswith("running_mean"):
            res["rm." + key] = v.detach().clone()
        elif key.endswith("running_var"):
            res["rv." + key] = v.detach().clone()
    return res


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


def round_output(m):
    m.register_forward_hook(lambda _m, _i, o: RoundBoth.apply(o))


def round_convs(mod, conv_cls):
    """every nn.Conv2d weight through bf16; every nn.Conv2d output and every ``conv_cls`` output through RoundBoth"""
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(bf16(m.weight))
    for m in mod.modules():
        if isinstance(m, (nn.Conv2d, conv_cls)):
            round_output(m)
    return mod


def kind(k):
    return "out" if k == "out" else "run" if k[:3] in ("rm.", "rv.") else "grad"


def bf16_floor(rounded, before, x, gout, exact):
    """the module's own error when its tensors pass through bf16 where a bf16 implementation stores them: ``rounded(before)`` is the
    family's module with the parameters ``before`` and its roundings in place; the same step on the bf16-rounded input against ``exact``,
    worst error relative to each tensor's max, per kind"""
    got = run(rounded(before), bf16(x), gout)
    floor = {}
    for k, want in exact.items():
        scale = float(want.abs().max())
        floor[kind(k)] = max(floor.get(kind(k), 0.0), float((got[k] - want).abs().max()) / (scale if scale > 0 else 1.0))
    return floor


def write_fixture(path, meta, before, x, gout, exact, floor=None, as_f32=lambda k: True):
    """npz layout: ``meta`` (cls, args, ...), keys, p.<key> the state BEFORE the step, x, grad_out, and ``exact`` (out, grad_x, g.<key>,
    rm.<key>, rv.<key>) as ``run`` names them; floor.<kind> in float64.  A float64 array is stored as float32 where ``as_f32(name)``."""
    arrs = {k: np.array(v) for k, v in meta.items()}
    arrs.update(keys=np.array(list(before), dtype=str), x=x.numpy(), grad_out=gout.numpy())
    arrs.update(("p." + k, v.numpy()) for k, v in before.items())
    arrs.update((k, v.numpy()) for k, v in exact.items())
    arrs = {k: v.astype(np.float32) if v.dtype == np.float64 and as_f32(k) else v for k, v in arrs.items()}
    for k, v in (floor or {}).items():
        arrs["floor." + k] = np.array(v, dtype=np.float64)
    np.savez_compressed(path, **arrs)
    print(f"{path}: {os.path.getsize(path)} bytes, out {tuple(exact['out'].shape)}, {len(before)} keys"
          + (", floor " + ", ".join(f"{k} {v:.2e}" for k, v in floor.items()) if floor else ""))


def record_module(path, gen, make, shape, meta, draw=draw_parameters, rounded=None, as_f32=lambda k: True):
    """the common case: build, draw the parameters, x and grad_out, take the step (and the bf16 floor where the family records one), write"""
    mod = make()
    draw(mod, gen)
    before = snapshot(mod)
    x, gout = draw_io(mod, shape, gen)
    exact = run(mod, x, gout)
    floor = bf16_floor(rounded, before, x, gout, exact) if rounded is not None else None
    write_fixture(path, meta, before, x, gout, exact, floor, as_f32)


def main(cases, load_reference, record):
    """``record(ns, seed, case, path)`` once per case, in the order of ``cases``: the seed is the case's position"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=OUT, help="directory the .npz files are written to")
    opt = ap.parse_args()
    ns = load_reference(opt.reference)
    os.makedirs(opt.out, exist_ok=True)
    for seed, (name, case) in enumerate(cases.items()):
        record(ns, seed, case, os.path.join(opt.out, name + ".npz"))
