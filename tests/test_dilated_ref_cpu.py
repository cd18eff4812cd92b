"""CPU: tests/dilated_ref.py (the float64 statement of ydl_dilated_cols / ydl_dilated_cols_bwd the GPU tests compare against) is the
column form of torch's dilated convolution, and its backward is the exact transpose of its forward."""
import numpy as np
import pytest
import torch

from tests.dilated_ref import dilated_cols, dilated_cols_bwd, round_up

SHAPES = [(2, 5, 7, 8, 3, 1), (2, 9, 7, 16, 3, 2), (1, 8, 8, 12, 3, 3), (2, 6, 5, 40, 3, 5), (1, 4, 4, 8, 3, 6), (1, 7, 6, 5, 5, 2)]


@pytest.mark.parametrize("N,H,W,C,k,d", SHAPES)
def test_cols_times_weight_is_the_dilated_convolution(N, H, W, C, k, d):
    rs = np.random.RandomState(N * 100 + C + d)
    x = rs.randn(N, H, W, C)
    wgt = rs.randn(6, C, k, k)                                          # OIHW
    col = dilated_cols(x, k, d)
    assert col.shape == (N * H * W, round_up(k * k * C, 8))
    assert not col[:, k * k * C:].any()
    w2 = wgt.transpose(0, 2, 3, 1).reshape(6, k * k * C)                # KRSC: the 1x1 weight over col, unchanged
    got = (col[:, :k * k * C] @ w2.T).reshape(N, H, W, 6).transpose(0, 3, 1, 2)
    want = torch.nn.functional.conv2d(torch.from_numpy(x.transpose(0, 3, 1, 2).copy()), torch.from_numpy(wgt), stride=1,
                                      padding=d * (k - 1) // 2, dilation=d).numpy()
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_ones_column_and_zero_padding():
    x = np.random.RandomState(1).randn(1, 3, 4, 12)
    col = dilated_cols(x, 3, 2, ones_col=True)
    assert col.shape[1] == 112 and (col[:, 108] == 1).all() and not col[:, 109:].any()
    assert (col[:, :108] == dilated_cols(x, 3, 2)[:, :108]).all()


@pytest.mark.parametrize("N,H,W,C,k,d", SHAPES)
def test_backward_is_the_transpose_of_the_forward(N, H, W, C, k, d):
    rs = np.random.RandomState(7 + C + d)
    x = rs.randn(N, H, W, C)
    width = round_up(k * k * C, 8)
    g = rs.randn(N * H * W, width)
    lhs = float((dilated_cols(x, k, d)[:, :k * k * C] * g[:, :k * k * C]).sum())
    rhs = float((x * dilated_cols_bwd(g, (N, H, W, C), k, d)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_every_off_centre_tap_is_outside_when_d_reaches_the_image():
    x = np.random.RandomState(3).randn(1, 4, 4, 8)
    col = dilated_cols(x, 3, 6).reshape(1, 4, 4, -1)
    assert (col[..., 4 * 8:5 * 8] == x).all()
    assert not np.delete(col, np.s_[32:40], axis=-1).any()
