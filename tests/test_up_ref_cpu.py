"""tests/up_ref.py held to torch on the CPU: the float64 form of the bicubic restatement (source coordinate, coefficients, clamped taps,
the separable 4 x 4 sum and its explicit transpose) against F.interpolate(mode='bicubic') and its autograd in float64, for both
align_corners conventions, up- and down-sampling, a scale_factor that is no integer, the identity size, a single output pixel and a
one-row input.  The restatement agrees with torch to a few 1e-15 at these shapes (asserted: 1e-13 of the largest element).  The float32
form the GPU tests use must pick the same floor(src) as the float64 form at every size used here and in tests/test_gpu_bicubic.py, and
the comparison helper must reject three plausible wrong answers."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import spatial_ref as R
from tests import up_ref as B

F32, F64 = np.float32, np.float64

# (Hi, Wi, Ho, Wo, scale_factor or None)
SHAPES = [(5, 7, 10, 14, 2.0), (5, 7, 7, 10, 1.5), (5, 7, 3, 4, None), (5, 7, 1, 1, None), (5, 7, 5, 7, None), (1, 6, 3, 9, None)]
# the sizes of tests/test_gpu_bicubic.py on top of those
GPU_SHAPES = [(6, 6, 3, 3, None), (1, 1, 4, 4, None), (3, 1, 6, 2, None)]


def rng(seed):
    return np.random.RandomState(seed)


def _given(sf):
    return 0.0 if sf is None else 1.0 / sf


def _torch(x, Ho, Wo, sf, align):
    """F.interpolate on the NHWC array x in float64 -> (y NHWC, function dy -> dx)"""
    t = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).double().requires_grad_(True)
    if sf is not None:
        y = F.interpolate(t, scale_factor=sf, mode="bicubic", align_corners=align)
    else:
        y = F.interpolate(t, size=(Ho, Wo), mode="bicubic", align_corners=align)
    assert tuple(y.shape[2:]) == (Ho, Wo)

    def grad(dy):
        g, = torch.autograd.grad(y, t, torch.from_numpy(np.ascontiguousarray(dy.transpose(0, 3, 1, 2))).double(), retain_graph=True)
        return g.numpy().transpose(0, 2, 3, 1)
    return y.detach().numpy().transpose(0, 2, 3, 1), grad


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("Hi,Wi,Ho,Wo,sf", SHAPES)
def test_float64_form_equals_interpolate_and_its_autograd(Hi, Wi, Ho, Wo, sf, align):
    x = rng(1).standard_normal((2, Hi, Wi, 3))
    dy = rng(2).standard_normal((2, Ho, Wo, 3))
    g = 0.0 if align else _given(sf)
    th, tw = B.cub_taps(align, Hi, Ho, g, F64), B.cub_taps(align, Wi, Wo, g, F64)
    y, _ = B.bicubic_fwd_ref(x, th, tw)
    want, grad = _torch(x, Ho, Wo, sf, align)
    err = np.abs(y - want).max()
    dx, _, _ = B.bicubic_bwd_ref(dy, th, tw, Hi, Wi)
    gerr = np.abs(dx - grad(dy)).max()
    print(f"  bicubic {Hi}x{Wi}->{Ho}x{Wo} align={align}: forward {err:.1e}  backward {gerr:.1e}")
    assert err <= 1e-13 * np.abs(want).max() and gerr <= 1e-13 * np.abs(dx).max()
    # previous contents are added first
    prev = rng(3).standard_normal((2, Hi, Wi, 3))
    assert np.abs(B.bicubic_bwd_ref(dy, th, tw, Hi, Wi, prev)[0] - (prev + dx)).max() <= 1e-14 * np.abs(dx).max() + 1e-14


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("Hi,Wi,Ho,Wo,sf", SHAPES + GPU_SHAPES)
def test_float32_and_float64_floor_agree(Hi, Wi, Ho, Wo, sf, align):
    """the float32 source coordinate falls into the same cell as the exact one at every size the tests use, so the float64 reference
    on float32 taps and F.interpolate(float64) describe the same operator up to the coefficients' rounding"""
    g = 0.0 if align else _given(sf)
    for n_in, n_out in ((Hi, Ho), (Wi, Wo)):
        i32, t32 = B.cub_src(n_out, B.cub_scale(align, n_in, n_out, g, F32), align, F32)
        i64, t64 = B.cub_src(n_out, B.cub_scale(align, n_in, n_out, g, F64), align, F64)
        assert (i32 == i64).all(), (n_in, n_out, i32, i64)
        assert np.abs(t32.astype(F64) - t64).max() <= 4 * (n_in + 1) * R.U
        c32, c64 = B.cub_taps(align, n_in, n_out, g, F32)[1], B.cub_taps(align, n_in, n_out, g, F64)[1]
        assert np.abs(c32.astype(F64) - c64).max() <= 64 * (n_in + 1) * R.U
        assert np.abs(c64.sum(1) - 1).max() <= 1e-14 and np.abs(c64).sum(1).max() <= 1.375 + 1e-12


def test_float32_reference_is_close_to_interpolate():
    """the float64 sum over float32 taps (what the GPU tests compare with) against torch: the coefficients' rounding only"""
    x = rng(4).standard_normal((2, 5, 7, 4)).astype(F32)
    for align in (False, True):
        c = B.case_bicubic(x, align, 10, 14, "f32")
        want, _ = _torch(x.astype(F64), 10, 14, None, align)
        assert np.abs(c["ref"] - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_helper_accepts_the_floor_and_rejects_three_wrong_answers(dtype):
    """A = -0.5 (the other common cubic), the source coordinate clamped at 0 as bilinear does, border taps that wrap instead of
    clamping: each is evaluated exactly (float64, then stored) and must miss the bound; forward and backward"""
    N, Hi, Wi, Ho, Wo, C = 2, 5, 7, 10, 14, 8
    x = rng(5).standard_normal((N, Hi, Wi, C)).astype(F32)
    dy = rng(6).standard_normal((N, Ho, Wo, C)).astype(F32)
    fc = B.case_bicubic(x, False, Ho, Wo, dtype)
    bc = B.case_bicubic_bwd(dy, False, Hi, Wi, dtype)
    for c, fn in ((fc, B.check_bicubic), (bc, B.check_bicubic_bwd)):
        res = fn(c["layout"].embed(c["floor"]), c)
        assert R.accepted(res) and res[1] <= res[2], res
    for kw in (dict(A=-0.5), dict(clamp0=True), dict(wrap=True)):
        th, tw = B.cub_taps(False, Hi, Ho, **kw), B.cub_taps(False, Wi, Wo, **kw)
        wrong = R.store(B.bicubic_fwd_ref(fc["x"].astype(F64), th, tw)[0], dtype)
        assert not R.accepted(B.check_bicubic(fc["layout"].embed(wrong), fc)), kw
        wrong = R.store(B.bicubic_bwd_ref(bc["dy"].astype(F64), th, tw, Hi, Wi)[0], dtype)
        assert not R.accepted(B.check_bicubic_bwd(bc["layout"].embed(wrong), bc)), kw
    # a disturbed sentinel is a violation whatever the values are
    buf = fc["layout"].embed(fc["floor"])
    buf[0] = 0.0
    assert not R.accepted(B.check_bicubic(buf, fc))
