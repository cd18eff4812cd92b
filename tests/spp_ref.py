"""numpy float64 restatement of the parallel pooling pyramid (ydl_spp_pool_fwd / _bwd, csrc/spp.hip): y_i = max-pool(x; k_i, stride 1,
pad k_i // 2, -inf padding), every pool of the same x.

* ``pool_fwd(x, k)`` -> (y, code): for every output position the window is scanned ky then kx ascending, out-of-plane taps skipped,
  the first in-range tap initialises and a later one replaces the running maximum when ``v > best or isnan(v)`` (ATen's rule): the
  FIRST maximum in scan order wins a tie, the LAST NaN wins a window that holds one.  ``code`` = ky * k + kx of the winner (uint8).
* ``pool_bwd(dy, code, k)`` -> dx: every input element gathers dy from the output positions whose code names it, ky then kx
  ascending (the summation order of maxpool_bwd_kernel).
* ``spp_fwd`` / ``spp_bwd``: the pyramid; dx = ((dx0 + mp1'(dy1)) + mp2'(dy2)) + mp3'(dy3) in that order.

Arrays are (N, C, H, W).  Plain loops over the window: the test planes are tiny."""
import numpy as np


def pool_fwd(x, k):
    x = np.asarray(x, dtype=np.float64)
    N, C, H, W = x.shape
    p = k // 2
    y = np.empty_like(x)
    code = np.zeros(x.shape, dtype=np.uint8)
    for ho in range(H):
        for wo in range(W):
            best = None
            bc = np.zeros((N, C), dtype=np.uint8)
            for ky in range(k):
                ih = ho - p + ky
                if ih < 0 or ih >= H:
                    continue
                for kx in range(k):
                    iw = wo - p + kx
                    if iw < 0 or iw >= W:
                        continue
                    v = x[:, :, ih, iw]
                    if best is None:
                        best = v.copy()
                        bc[:] = ky * k + kx
                        continue
                    with np.errstate(invalid="ignore"):
                        upd = (v > best) | np.isnan(v)
                    best = np.where(upd, v, best)
                    bc = np.where(upd, np.uint8(ky * k + kx), bc)
            y[:, :, ho, wo] = best
            code[:, :, ho, wo] = bc
    return y, code


def pool_bwd(dy, code, k, dx=None):
    dy = np.asarray(dy, dtype=np.float64)
    N, C, H, W = dy.shape
    p = k // 2
    dx = np.zeros_like(dy) if dx is None else np.array(dx, dtype=np.float64)
    for ih in range(H):
        for iw in range(W):
            g = dx[:, :, ih, iw].copy()
            for ky in range(k):
                ho = ih + p - ky
                if ho < 0 or ho >= H:
                    continue
                for kx in range(k):
                    wo = iw + p - kx
                    if wo < 0 or wo >= W:
                        continue
                    g = g + np.where(code[:, :, ho, wo] == ky * k + kx, dy[:, :, ho, wo], 0.0)
            dx[:, :, ih, iw] = g
    return dx


def spp_fwd(x, ks):
    """[(y, code)] per window size"""
    return [pool_fwd(x, k) for k in ks]


def spp_bwd(dys, codes, ks, dx=None):
    for dy, code, k in zip(dys, codes, ks):
        dx = pool_bwd(dy, code, k, dx)
    return dx


def chain_fwd(x, k, n=3):
    """SPPF's chain y1 = mp(x), y2 = mp(y1), ...: [(y, code)]"""
    out = []
    for _ in range(n):
        y, c = pool_fwd(x, k)
        out.append((y, c))
        x = y
    return out
