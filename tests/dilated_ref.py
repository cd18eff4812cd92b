"""numpy float64 restatement of ydl_dilated_cols / ydl_dilated_cols_bwd (include/ydl.h): the column form of a k x k convolution with
dilation d, stride 1 and padding d*(k-1)/2 on NHWC arrays.  tests/test_dilated_ref_cpu.py pins it against torch's conv2d."""
import numpy as np


def round_up(a, b):
    return (a + b - 1) // b * b


def _taps(k, d):
    r = k // 2
    return [((ky - r) * d, (kx - r) * d) for ky in range(k) for kx in range(k)]


def dilated_cols(x, k, d, ones_col=False):
    """x [N, H, W, C] -> col [N*H*W, round_up(k*k*C + ones, 8)]: col[pix][tap*C + c] = x[n, h + dy, w + dx, c] or 0 outside the image,
    then the ones column, then zeros"""
    N, H, W, C = x.shape
    width = round_up(k * k * C + int(bool(ones_col)), 8)
    col = np.zeros((N, H, W, width), dtype=x.dtype)
    for t, (dy, dx) in enumerate(_taps(k, d)):
        h0, h1 = max(0, -dy), min(H, H - dy)
        w0, w1 = max(0, -dx), min(W, W - dx)
        if h0 < h1 and w0 < w1:
            col[:, h0:h1, w0:w1, t * C:(t + 1) * C] = x[:, h0 + dy:h1 + dy, w0 + dx:w1 + dx, :]
    if ones_col:
        col[..., k * k * C] = 1
    return col.reshape(N * H * W, width)


def dilated_cols_bwd(dcol, shape, k, d):
    """dcol [N*H*W, >= k*k*C] -> dx [N, H, W, C] in float64: dx[n, h, w, c] = sum over taps of dcol[n, h - dy, w - dx][tap*C + c]"""
    N, H, W, C = shape
    g = np.asarray(dcol, dtype=np.float64).reshape(N, H, W, -1)
    dx_ = np.zeros((N, H, W, C), dtype=np.float64)
    for t, (dy, dx) in enumerate(_taps(k, d)):
        h0, h1 = max(0, -dy), min(H, H - dy)          # output pixels whose tap t is inside the image
        w0, w1 = max(0, -dx), min(W, W - dx)
        if h0 < h1 and w0 < w1:
            dx_[:, h0 + dy:h1 + dy, w0 + dx:w1 + dx, :] += g[:, h0:h1, w0:w1, t * C:(t + 1) * C]
    return dx_
