"""The reference of the space-to-depth / depth-to-space tests: the two index maps of include/ydl.h written as torch slice assignments on
(N, C, H, W) tensors of any dtype (copies are exact).  tests/test_sd_ref_cpu.py pins it to Focus's four slices and to Contract's and
Expand's reshape / permute.  Not collected."""
import torch


def block(sy, sx, s, order):
    return sy * s + sx if order == 0 else sx * s + sy


def space_to_depth_ref(x, s, order):
    """(N, C, H, W) -> (N, s*s*C, H/s, W/s): out[:, blk(sy, sx)*C + c, ho, wo] = x[:, c, ho*s + sy, wo*s + sx]"""
    x = torch.as_tensor(x)
    N, C, H, W = x.shape
    assert H % s == 0 and W % s == 0
    out = torch.empty((N, s * s * C, H // s, W // s), dtype=x.dtype)
    for sy in range(s):
        for sx in range(s):
            b = block(sy, sx, s, order)
            out[:, b * C:(b + 1) * C] = x[:, :, sy::s, sx::s]
    return out


def depth_to_space_ref(x, s, order):
    """(N, s*s*C, H, W) -> (N, C, H*s, W*s): out[:, c, h*s + sy, w*s + sx] = x[:, blk(sy, sx)*C + c, h, w]"""
    x = torch.as_tensor(x)
    N, CC, H, W = x.shape
    assert CC % (s * s) == 0
    C = CC // (s * s)
    out = torch.empty((N, C, H * s, W * s), dtype=x.dtype)
    for sy in range(s):
        for sx in range(s):
            b = block(sy, sx, s, order)
            out[:, :, sy::s, sx::s] = x[:, b * C:(b + 1) * C]
    return out
