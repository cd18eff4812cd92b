"""The bicubic resize of csrc/spatial.hip (ydl_bicubic_fwd / ydl_bicubic_bwd; the tape's modes 3 = align_corners False and 4 = True are
their ``align`` argument 0 and 1) through the C ABI against the float64 reference of tests/up_ref.py, per element, in the Layout /
sentinel / check_rounded scheme of tests/spatial_ref.py: every tensor is a view inside a buffer of sentinels (ld == Cp, or a channel slice of a wider buffer one chunk in)
and nothing outside the answer may change.

Bounds (tests/up_ref.py, named roundings in units of U = 2^-24):
  forward    10 U of the element's own sum |ch cw x| (the products and additions on the path of one term of the 4 x 4 sum; sum |c| <=
             1.375 per axis) + 2^-8 |ref| for a bf16 store
  backward   (contributing outputs + 8) U of sum (sum |ch|)(sum |cw|) |dy| + (outputs) U |previous contents| + the bf16 store
The same reference evaluated in float32 in the kernel's order (the floor) must pass its own bound.  Every test prints GPU error, floor
and bound (pytest -s).

Worst share of a bound measured on an MI355X (GPU error (floor) / bound): forward f32 1.33e-8 (1.34e-8) / 4.87e-8 = 0.27 (5x7 -> 10x14, wide);
bf16 0.99, all of it the store rounding; backward f32 2.44e-9 (2.44e-9) / 2.78e-9 = 0.88 (6x6 <- 3x3, mode 4, accumulate: three
contributing outputs, the roundings of the piled weights and of the previous contents); bf16 1.00, the store rounding.  The GPU answer
equals the float32 floor in most cases to the printed digits.

Shapes: up-sampling by 2 with two samples and a wide buffer, a scale_factor of 1.5, down-sampling 6 -> 3, a single input pixel (every
tap clamped onto it) and a one-column input with 136 channels (more than one 16-byte chunk per thread row; two chunk widths)."""
import numpy as np
import pytest
import torch

from tests import spatial_gpu as G
from tests import spatial_ref as R
from tests import up_ref as B

pytestmark = pytest.mark.gpu
F32 = np.float32

# (N, Hi, Wi, Ho, Wo, C, wide, scale_factor)
SHAPES = [(2, 5, 7, 10, 14, 24, True, None), (1, 5, 7, 7, 10, 8, False, 1.5), (1, 6, 6, 3, 3, 40, False, None),
          (1, 1, 1, 4, 4, 8, False, None), (1, 3, 1, 6, 2, 136, False, None)]
IDS = ["5x7-10x14-C24-wide", "5x7-7x10-C8-sf1.5", "6x6-3x3-C40", "1x1-4x4-C8", "3x1-6x2-C136"]


def rng(seed):
    return np.random.RandomState(seed)


def _given(mode, sf):
    return float(F32(1.0 / sf)) if (sf is not None and mode == 3) else 0.0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("N,Hi,Wi,Ho,Wo,C,wide,sf", SHAPES, ids=IDS)
def test_bicubic_forward(dtype, mode, N, Hi, Wi, Ho, Wo, C, wide, sf):
    d, tdt, es, V = G.dt(dtype)
    g = _given(mode, sf)
    lay = G.slice_layout(N * Ho * Wo, C, dtype, wide)
    c = B.case_bicubic(rng(11).standard_normal((N, Hi, Wi, C)).astype(F32), mode == 4, Ho, Wo, dtype, ld=lay.ld, gh=g, gw=g, lead=lay.lead)
    xb = G.Buf(G.slice_layout(N * Hi * Wi, C, dtype, wide), tdt, c["x"])
    yb = G.Buf(lay, tdt)
    G.call("ydl_bicubic_fwd", d, int(mode == 4), xb.p, xb.lay.ld, yb.p, lay.ld, N, Hi, Wi, Ho, Wo, C, g, g, G.stream())
    G.sync()
    G.check(f"bicubic forward | {dtype} mode {mode} {Hi}x{Wi}->{Ho}x{Wo} C{C} wide={wide}", B.check_bicubic, yb.host(), c)
    assert xb.lay.violations(xb.host()) == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("N,Hi,Wi,Ho,Wo,C,wide,sf", SHAPES, ids=IDS)
def test_bicubic_backward(dtype, mode, N, Hi, Wi, Ho, Wo, C, wide, sf):
    """overwrite and accumulate, per element; two runs of each are equal to the bit (gather form, no atomics)"""
    d, tdt, es, V = G.dt(dtype)
    g = _given(mode, sf)
    dy = rng(12).standard_normal((N, Ho, Wo, C)).astype(F32)
    prev = rng(13).standard_normal((N, Hi, Wi, C)).astype(F32)
    lay = G.slice_layout(N * Hi * Wi, C, dtype, wide)
    for acc in (0, 1):
        c = B.case_bicubic_bwd(dy, mode == 4, Hi, Wi, dtype, prev if acc else None, ld=lay.ld, gh=g, gw=g, lead=lay.lead)
        dyb = G.Buf(G.slice_layout(N * Ho * Wo, C, dtype, wide), tdt, c["dy"])
        runs = []
        for _ in range(2):
            dxb = G.Buf(lay, tdt, c["prev"]) if acc else G.Buf(lay, tdt)
            G.call("ydl_bicubic_bwd", d, int(mode == 4), dyb.p, dyb.lay.ld, dxb.p, lay.ld, acc, N, Hi, Wi, Ho, Wo, C, g, g, G.stream())
            G.sync()
            runs.append(dxb.host())
        G.check(f"bicubic backward | {dtype} mode {mode} {Hi}x{Wi}<-{Ho}x{Wo} C{C} wide={wide} acc={acc}", B.check_bicubic_bwd, runs[0], c)
        assert np.array_equal(lay.answer(runs[0]), lay.answer(runs[1])), "two backward runs differ"


@pytest.mark.parametrize("mode", [3, 4])
def test_the_three_resize_entry_points_refuse_the_bicubic_modes(mode):
    """ydl_resize_fwd / ydl_resize_bwd / ydl_resize_acc_sums keep their three modes and say on the host where bicubic lives"""
    d, tdt, es, V = G.dt("f32")
    xb = G.Buf(R.Layout(4 * 4, 8, 8), tdt, np.zeros((16, 8)))
    yb = G.Buf(R.Layout(8 * 8, 8, 8), tdt)
    G.refused("ydl_resize_fwd", (d, mode, xb.p, 8, yb.p, 8, 1, 4, 4, 8, 8, 8, 0.0, 0.0, G.stream()), [yb], "ydl_bicubic_fwd")
    G.refused("ydl_resize_bwd", (d, mode, xb.p, 8, yb.p, 8, 0, 1, 8, 8, 4, 4, 8, 0.0, 0.0, G.stream()), [yb], "ydl_bicubic_bwd")
    G.refused("ydl_resize_acc_sums", (d, mode, xb.p, 8, yb.p, 8, 1, 4, 4, 8, 8, 8, 0.0, 0.0, None, 0, G.stream()), [yb], "bicubic")


def test_bad_arguments_are_refused():
    d, tdt, es, V = G.dt("f32")
    xb = G.Buf(R.Layout(4 * 4, 8, 8), tdt, np.zeros((16, 8)))
    yb = G.Buf(R.Layout(8 * 8, 8, 8), tdt)
    st = G.stream()
    G.refused("ydl_bicubic_fwd", (d, 0, None, 8, yb.p, 8, 1, 4, 4, 8, 8, 8, 0.0, 0.0, st), [yb])
    G.refused("ydl_bicubic_fwd", (d, 0, xb.p, 4, yb.p, 8, 1, 4, 4, 8, 8, 8, 0.0, 0.0, st), [yb])                  # ld < Cp
    G.refused("ydl_bicubic_fwd", (d, 0, xb.p, 8, yb.p, 8, 1, 4, 4, 0, 8, 8, 0.0, 0.0, st), [yb])                  # an empty output
    G.refused("ydl_bicubic_bwd", (d, 1, xb.p, 8, None, 8, 0, 1, 8, 8, 4, 4, 8, 0.0, 0.0, st), [yb])
    G.refused("ydl_bicubic_bwd", (d, 1, xb.p, 8, yb.p, 10, 0, 1, 8, 8, 4, 4, 8, 0.0, 0.0, st), [yb], "alignment")
