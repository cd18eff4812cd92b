"""CPU: tests/local_attn_ref.py (the closed form the GPU tests compare against) reproduces the fixtures recorded from the reference's
own AttentionConv / AttentionStem classes (tools/make_attn_golden.py): the output and every gradient, float64 on both sides, to
1e-12 relative to each tensor's max."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import local_attn_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "attn_conv_*.npz")) + glob.glob(os.path.join(GOLDEN, "attn_stem_*.npz")))


def load(path):
    z = np.load(path)
    keys = [str(k) for k in z["keys"]]
    params = {k: torch.from_numpy(z["p." + k]).requires_grad_(True) for k in keys}
    grads = {k: torch.from_numpy(z["g." + k]) for k in keys}
    return z, keys, params, grads


def run_ref(z, params):
    _c1, _c2, ks, _s, _p, _g, m = (int(v) for v in z["args"])
    x = torch.from_numpy(z["x"]).requires_grad_(True)
    out = R.attention_stem(x, params, ks, m) if m else R.attention_conv(x, params, ks)
    out.backward(torch.from_numpy(z["grad_out"]))
    return x, out


def test_fixture_set():
    assert [os.path.basename(f) for f in FILES] == ["attn_conv_16_24_k3.npz", "attn_conv_8_16_k5_g4.npz", "attn_stem_16_24_k3_m4.npz",
                                                    "attn_stem_8_8_k3_m1_g2.npz"]


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_restatement_reproduces_the_reference(path):
    z, keys, params, grads = load(path)
    assert z["x"].dtype == np.float64 and z["out"].dtype == np.float64
    x, out = run_ref(z, params)

    def err(got, want):
        want = torch.as_tensor(want)
        scale = float(want.abs().max())         # an all-zero gradient (the mixing table of m = 1 is constant): absolute error
        return float((got.detach() - want).abs().max()) / (scale if scale > 0 else 1.0)
    errs = {"out": err(out, z["out"]), "grad_x": err(x.grad, z["grad_x"])}
    for k in keys:
        errs["g." + k] = err(params[k].grad, grads[k])
    print(os.path.basename(path), {k: f"{v:.1e}" for k, v in errs.items()})
    assert all(v < 1e-12 for v in errs.values()), errs
