"""CPU: the f64 restatement of deform_conv2d (tests/deform_ref.py) is pinned by answers F.conv2d gives on its own, so the GPU
tests compare against something that does not only agree with itself."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests.deform_ref import deform_conv2d_ref


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _out_hw(H, k, s, p, d):
    return (H + 2 * p - (d * (k - 1) + 1)) // s + 1


@pytest.mark.parametrize("k,s,p,d,G", [c for c in itertools.product((1, 3, 5), (1, 2), (0, 1, 2), (1, 2), (1, 2))
                                       if _out_hw(9, c[0], c[1], c[2], c[3]) > 0])
def test_zero_offsets_equal_conv2d(k, s, p, d, G):
    x, w, b = _rand(2, 4, 9, 9), _rand(3, 4, k, k, seed=1), _rand(3, seed=2)
    Ho = _out_hw(9, k, s, p, d)
    off = torch.zeros(2, 2 * G * k * k, Ho, Ho, dtype=torch.float64)
    ref = F.conv2d(x, w, b, s, p, d)
    out = deform_conv2d_ref(x, off, w, b, s, p, d)
    assert (out - ref).abs().max() <= 1e-12


def _shift(x, dy, dx):
    """x sampled at (h + dy, w + dx), zero outside"""
    out = torch.zeros_like(x)
    H, W = x.shape[-2:]
    for h in range(H):
        for w_ in range(W):
            if 0 <= h + dy < H and 0 <= w_ + dx < W:
                out[..., h, w_] = x[..., h + dy, w_ + dx]
    return out


def test_integer_offset_and_constant_mask():
    x, w = _rand(2, 3, 8, 7), _rand(5, 3, 3, 3, seed=1)
    off = torch.zeros(2, 18, 8, 7, dtype=torch.float64)
    off[:, 0::2], off[:, 1::2] = 1.0, -2.0
    ref = F.conv2d(_shift(F.pad(x, (1, 1, 1, 1)), 1, -2), w, None, 1, 0)     # shift the zero-padded input, then convolve
    out = deform_conv2d_ref(x, off, w, None, 1, 1)
    assert (out - ref).abs().max() <= 1e-12
    mask = torch.full((2, 9, 8, 7), 0.37, dtype=torch.float64)
    out_m = deform_conv2d_ref(x, off, w, None, 1, 1, mask=mask)
    assert (out_m - 0.37 * ref).abs().max() <= 1e-12


def test_half_pixel_offset_is_the_mean_of_two_neighbours():
    x = _rand(1, 2, 6, 6)
    w = torch.zeros(2, 2, 1, 1, dtype=torch.float64)
    w[0, 0, 0, 0] = w[1, 1, 0, 0] = 1.0                          # identity 1x1
    off = torch.zeros(1, 2, 6, 6, dtype=torch.float64)
    off[:, 1] = 0.5                                              # dx = +0.5
    out = deform_conv2d_ref(x, off, w)
    ref = 0.5 * (x + _shift(x, 0, 1))
    assert (out - ref).abs().max() <= 1e-12


def test_positions_past_the_border_are_zero():
    x = _rand(1, 2, 5, 5)
    w = torch.ones(1, 2, 1, 1, dtype=torch.float64)
    for dy, dx in ((-1.0, 0.0), (-3.5, 0.0), (5.0, 0.0), (0.0, -1.0), (0.0, -1.25), (0.0, 5.2), (2.5, 0.0)):
        off = torch.zeros(1, 2, 5, 5, dtype=torch.float64)
        off[:, 0], off[:, 1] = dy, dx
        out = deform_conv2d_ref(x, off, w)[0, 0]
        for h in range(5):
            for w_ in range(5):
                y, xx = h + dy, w_ + dx
                if y <= -1 or y >= 5 or xx <= -1 or xx >= 5:
                    assert out[h, w_] == 0, (dy, dx, h, w_)
                else:
                    assert out[h, w_] != 0, (dy, dx, h, w_)


def test_gradcheck_generic_positions():
    x = _rand(1, 4, 5, 6).requires_grad_()
    w = _rand(3, 4, 3, 3, seed=1).requires_grad_()
    b = _rand(3, seed=2).requires_grad_()
    off = (0.37 + 0.6 * _rand(1, 2 * 2 * 9, 5, 6, seed=3)).requires_grad_()     # G = 2, generic (non-integer) positions
    mask = torch.sigmoid(_rand(1, 2 * 9, 5, 6, seed=4)).requires_grad_()
    assert torch.autograd.gradcheck(lambda *a: deform_conv2d_ref(a[0], a[1], a[2], a[3], 1, 1, 1, a[4]), (x, off, w, b, mask),
                                     eps=1e-6, atol=1e-6)
