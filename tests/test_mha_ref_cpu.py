"""CPU: tests/mha_ref.py (the float64 closed form of dense multi-head self-attention and of its gradients, which pins the HIP kernels)
is itself pinned
* against torch autograd of the same composition in float64 (<= 1e-12 of each tensor's max), and against
  torch.nn.functional.scaled_dot_product_attention;
* against the fixtures recorded from the reference's own TransformerLayer / TransformerBlock / C3TR (tools/make_transformer_golden.py),
  by composing the layers from it: out and grad_x (stored in float64) to 1e-10, parameter gradients (stored rounded to float32) to 1e-6."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import mha_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "tr_*.npz")))


def _err(got, want):
    """relative to the reference tensor's max; a tensor that is analytically zero (out_proj.bias of C3TR: a per-channel constant in
    front of cv3's train-mode BatchNorm; the reference holds float64 rounding noise, 1e-14) is compared absolutely"""
    scale = float(want.abs().max())
    return float((got - want).abs().max()) / (scale if scale > 1e-10 else 1.0)


@pytest.mark.parametrize("N,S,heads,d", [(1, 1, 1, 8), (2, 35, 4, 8), (2, 20, 2, 24), (1, 70, 2, 16)])
def test_closed_form_gradients_equal_autograd(N, S, heads, d):
    gen = torch.Generator().manual_seed(S)
    q, k, v, dout = (torch.randn(N, S, heads * d, generator=gen, dtype=torch.float64) for _ in range(4))
    scale = d ** -0.5
    dq, dk, dv = R.mha_grad(q, k, v, dout, heads, scale)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    out, lse = R.mha(qa, ka, va, heads, scale)
    out.backward(dout)
    for got, want in ((dq, qa.grad), (dk, ka.grad), (dv, va.grad)):
        assert _err(got, want) <= 1e-12
    h = lambda t: t.reshape(N, S, heads, d).permute(0, 2, 1, 3)
    sd = torch.nn.functional.scaled_dot_product_attention(h(q), h(k), h(v)).permute(0, 2, 1, 3).reshape(N, S, heads * d)
    assert _err(out.detach(), sd) <= 1e-12
    s = scale * h(q) @ h(k).transpose(-1, -2)
    assert _err(lse.detach(), torch.logsumexp(s, -1)) <= 1e-12


def forward(z, p, x):
    cls, args = str(z["cls"]), [int(a) for a in z["args"]]
    if cls == "TransformerLayer":
        N, C, H, W = x.shape
        return R.transformer_layer(x.flatten(2).permute(0, 2, 1), p, "", args[1]).permute(0, 2, 1).reshape(N, C, H, W)
    if cls == "TransformerBlock":
        return R.transformer_block(x, p, "", args[2], args[3])
    return R.c3tr(x, p, "", args[2])


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_layers_composed_from_the_closed_form_match_the_reference_fixtures(path):
    z = np.load(path)
    p = {str(k): torch.from_numpy(z["p." + str(k)]).double().requires_grad_(z["p." + str(k)].dtype.kind == "f" and "running" not in str(k))
         for k in z["keys"]}
    x = torch.from_numpy(z["x"]).double().requires_grad_(True)
    out = forward(z, p, x)
    out.backward(torch.from_numpy(z["grad_out"]).double())
    assert _err(out.detach(), torch.from_numpy(z["out"])) <= 1e-10
    assert _err(x.grad, torch.from_numpy(z["grad_x"])) <= 1e-10
    n = 0
    for k in p:
        if "g." + k in z.files:
            assert p[k].grad is not None, k
            assert _err(p[k].grad, torch.from_numpy(z["g." + k]).double()) <= 1e-6, k
            n += 1
    assert n >= 9


def test_there_are_four_fixtures_within_the_size_limit_of_a_committed_file():
    """every parameter and its gradient are stored (8 bytes per parameter, 44 208 parameters in the largest case): the files are
    larger than the 100 000 bytes of the smaller fixture families; the limit that holds for them is the repository's 1 MiB"""
    assert len(FILES) == 4 and all(os.path.getsize(f) < (1 << 20) for f in FILES)
