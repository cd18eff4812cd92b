"""CPU: tests/spp_ref.py (the numpy statement of the parallel pooling pyramid that the GPU kernels are compared with) against
``torch.nn.functional.max_pool2d(..., return_indices=True)`` and autograd in float64.  The data is integer-valued (x in [-3, 3], dy in
{-1, 0, 1}): ties are everywhere, so the scan-order rule decides almost every arg-max, and every sum is exact.  On the same data the
gradient of SPPF's chain differs from the gradient of the parallel pools although the outputs agree: the fact that makes
ydl_spp_pool_* necessary next to ydl_sppf_pool_*."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import spp_ref

SHAPES = [(2, 3, 20, 13), (1, 2, 1, 1), (1, 2, 3, 20)]
KS = (5, 9, 13)


def _data(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, size=shape).astype(np.float64)
    dys = [rng.integers(-1, 2, size=shape).astype(np.float64) for _ in KS]
    return x, dys


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_equals_aten(shape):
    x, dys = _data(shape, 5)
    N, C, H, W = shape
    xt = torch.from_numpy(x).requires_grad_(True)
    got = spp_ref.spp_fwd(x, KS)
    total = 0
    for k, dy, (y, code) in zip(KS, dys, got):
        yt, it = F.max_pool2d(xt, k, 1, k // 2, return_indices=True)
        assert np.array_equal(y, yt.detach().numpy())
        # the byte code is a window offset; ATen returns the flat position in the plane
        p = k // 2
        ho, wo = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        flat = (ho - p + code.astype(np.int64) // k) * W + (wo - p + code.astype(np.int64) % k)
        assert np.array_equal(flat, it.numpy())
        total = total + (yt * torch.from_numpy(dy)).sum()
    total.backward()
    dx = spp_ref.spp_bwd(dys, [c for _y, c in got], KS)
    assert np.array_equal(dx, xt.grad.numpy())
    dx0 = np.full(shape, 2.0)
    assert np.array_equal(spp_ref.spp_bwd(dys, [c for _y, c in got], KS, dx=dx0), xt.grad.numpy() + 2.0)
    assert np.array_equal(dx0, np.full(shape, 2.0))          # the caller's array is left alone


def test_a_nan_wins_its_windows_and_the_last_one_stays():
    x = np.zeros((1, 1, 5, 5))
    x[0, 0, 1, 1] = np.nan
    x[0, 0, 2, 3] = np.nan
    x[0, 0, 4, 4] = 7.0
    y, code = spp_ref.pool_fwd(x, 3)
    yt, it = F.max_pool2d(torch.from_numpy(x), 3, 1, 1, return_indices=True)
    assert np.array_equal(np.isnan(y), torch.isnan(yt).numpy())
    assert np.array_equal(np.nan_to_num(y, nan=-9.0), torch.nan_to_num(yt, nan=-9.0).numpy())
    ho, wo = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
    flat = (ho - 1 + code[0, 0].astype(np.int64) // 3) * 5 + (wo - 1 + code[0, 0].astype(np.int64) % 3)
    assert np.array_equal(flat, it[0, 0].numpy())
    assert flat[2, 2] == 2 * 5 + 3                          # window (2, 2) holds both NaNs: the later one in scan order


def test_the_chain_has_the_same_outputs_and_another_gradient():
    x, dys = _data(SHAPES[0], 5)
    par = spp_ref.spp_fwd(x, KS)
    chain = spp_ref.chain_fwd(x, 5)
    for (yp, _cp), (yc, _cc) in zip(par, chain):
        assert np.array_equal(yp, yc)                       # mp5(mp5(x)) = mp9(x), mp5(mp5(mp5(x))) = mp13(x)
    # ATen agrees on both counts, for the 9 x 9 pool alone
    g = torch.from_numpy(dys[1])
    xa = torch.from_numpy(x).requires_grad_(True)
    ya = F.max_pool2d(xa, 9, 1, 4)
    ya.backward(g)
    xb = torch.from_numpy(x).requires_grad_(True)
    yb = F.max_pool2d(F.max_pool2d(xb, 5, 1, 2), 5, 1, 2)
    yb.backward(g)
    assert torch.equal(ya, yb)
    assert not torch.equal(xa.grad, xb.grad)
    assert float(xa.grad.sum()) == float(xb.grad.sum()) == float(g.sum())      # the same mass, routed elsewhere
    # and the reference's two routes reproduce both
    dpar = spp_ref.pool_bwd(dys[1], par[1][1], 9)
    dchain = spp_ref.pool_bwd(spp_ref.pool_bwd(dys[1], chain[1][1], 5), chain[0][1], 5)
    assert np.array_equal(dpar, xa.grad.numpy()) and np.array_equal(dchain, xb.grad.numpy())
