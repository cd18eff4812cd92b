"""The rounded kernels of csrc/spatial.hip (bilinear resize forward and backward, ydl_resize_acc_sums, global average, the average
branch of the global pool backward, ydl_channel_dot, ydl_scale_channels, the sigmoid gate), the group soft-max of csrc/dcn_blocks.hip
and ydl_bn_eval_coeffs of csrc/bn.hip through the C ABI against the float64 reference of tests/spatial_ref.py, per element.  The exact
kernels of the same files are in tests/test_gpu_spatial_exact.py.  Every output is a view inside a buffer of sentinels (ld == Cp, and
a channel slice of a wider buffer 16 bytes in); everything outside the documented output must still hold the sentinel.

Bounds.  tests/spatial_ref.py adds up named worst-case terms in units of U = 2^-24 per element, plus BF16 = 2^-8 relative for a bf16
store (the convention of tests/census.py); no bound is looser than what the suite asserted before for the same quantity (2e-6 / 1e-2
of the largest element for the resize backward, 2e-5 for the statistics of ydl_resize_acc_sums).  Every test also evaluates the same
reference in float32 on the CPU, in the kernel's own order of operations, and requires that this floor passes the same bound.  Every
test prints GPU error, floor and bound (pytest -s); an error is the largest |got - ref| / bound_i, scaled to the smallest bound_i.

__expf.  The group soft-max uses __expf, which is v_exp_f32 of the argument times log2(e): the rounded product and the rounded constant
move the exponent by 2 |d| U (d = v - max, counted with the data's largest |d|), and the instruction is documented at 1 ulp = 2 U.
EXPF = 4 U = 2 ulp is taken, twice the documented figure.  Measured against float64 with logits within 2^-4 of each other, where the
argument roundings stay under U / 4 (test_group_softmax_of_a_narrow_spread_shows_expf): a probability of two points is off by at most
1.17e-7 = 2.0 U relative, all roundings together (two __expf, one addition, the division, the product), so __expf itself showed at most
about half an ulp; the 4 U taken is above twice that, and the margin is kept because 300 x 8 arguments do not search the instruction.
At logits in [-8, 8] the largest relative error of a probability is 1.5e-6 against a bound of 6.7e-6, most of it |v - max| U.

Measured on one MI355X, worst case per family: GPU error (float32 floor) / bound of that element, and the share of the bound used
  bilinear forward                 f32 6.2e-10 (6.2e-10) / 1.3e-9, 0.48;  bf16 1.00 of the bound, all of it the store rounding
  bilinear backward                f32 1.3e-10 (1.3e-10) / 1.3e-10, 0.98 (generic kernel, 40 x 40 <- 20 x 20: one contributing output, the
                                   three roundings of wh * ww * dy and the one of the previous contents);  bf16 1.00, the store rounding
  resize_acc_sums values           1.00 of the bound in both types (one float32 addition, U |result|, respectively the bf16 store)
  resize_acc_sums statistics       f32 4.6e-6 (1.0e-5) / 2.0e-4 of the largest statistic, 0.02;  bf16 5.8e-6 (1.5e-5) / 3.7e-4, 0.02
  global average                   f32 5.2e-8 (5.2e-8) / 6.6e-6, 0.01;  bf16 1.8e-5 (1.8e-5) / 2.1e-5, 0.87 (the store)
  global pool backward (average)   f32 9.3e-11 (9.3e-11) / 1.7e-10, 0.55;  bf16 0.99 (the store)
  channel_dot                      f32 7.8e-8 (7.8e-8) / 5.4e-7, 0.14;  bf16 inputs 3.0e-6 (2.9e-6) / 8.0e-5, 0.04
  scale_channels                   1.00 of the bound in both types (one product, respectively the bf16 store)
  gate forward                     4.9e-32 (3.2e-32) / 9.7e-32 at the saturated end, 0.50; away from it at most 0.4 of the bound
  gate backward                    f32 1.1e-10 (1.1e-10) / 1.2e-10, 0.97;  bf16 0.96 (the store)
  group soft-max forward           f32 0.23 of the bound (floor 0.11);  bf16 0.99 (the store)
  group soft-max backward          f32 1.6e-10 (1.6e-10) / 1.6e-10, 0.99 (accumulate form: the addition of the previous contents);  bf16 0.99
  bn_eval_coeffs                   1.7e-10 (1.7e-10) / 1.9e-10, 0.91
In every family the GPU error equals the float32 floor to two digits wherever a single rounding dominates, and is never above 1.6x
the floor.  The exact module has no figures: 0 differing elements.  The kernels passed as they were, but for the NaN rule of the global
maximum (test_global_max_of_a_plane_with_nan of the exact module, fixed in global_pool_fwd_kernel's merge).
225 tests in the two modules (128 here, 97 there), 7 s for both on the GPU; the slowest test 0.6 s (the 513 x 512 max pool).
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import spatial_ref as R
from tests import spatial_gpu as G

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = ["f32", "bf16"]
CS = {"f32": (4, 12), "bf16": (8, 20)}
SHAPES = [(10, 12, 40, 48), (7, 9, 14, 18), (5, 6, 17, 11), (40, 40, 20, 20), (1, 5, 2, 10), (3, 300, 7, 33)]
HWS = [1, 5, 255, 256, 257, 1000]


def rng(seed):
    return np.random.RandomState(seed)


def combos(dtype):
    """(C, wide): the small C with ld == Cp, the C that is no chunk multiple as a slice of a wider buffer"""
    return [(CS[dtype][0], False), (CS[dtype][1], True), (CS[dtype][1], False)]


# ---------------------------------------------------------------------------------------------------------------------------
# bilinear resize
# ---------------------------------------------------------------------------------------------------------------------------
def _bilinear_fwd(dtype, mode, N, Hi, Wi, Ho, Wo, C, wide, g=0.0, variants=(1, 0)):
    L = G.lib()
    d, tdt, es, V = G.dt(dtype)
    x = rng(Hi * 31 + Wo + C).randn(N, Hi, Wi, C)
    lay = G.slice_layout(N * Ho * Wo, C, dtype, wide)
    c = R.case_bilinear(x, mode, Ho, Wo, dtype, ld=lay.ld, lead=lay.lead, gh=g, gw=g)
    xb = G.Buf(G.slice_layout(N * Hi * Wi, C, dtype, wide), tdt, c["x"])
    for rows in variants:
        yb = G.Buf(c["layout"], tdt)
        L.debug_set(11, rows)
        try:
            G.call("ydl_resize_fwd", d, mode, xb.p, xb.lay.ld, yb.p, yb.lay.ld, N, Hi, Wi, Ho, Wo, C, g, g, G.stream())
            G.sync()
        finally:
            L.debug_set(11, 1)
        G.check(f"bilinear forward | {dtype} mode {mode} {Hi}x{Wi}->{Ho}x{Wo} C{C} wide={wide} rows={rows}", R.check_bilinear, yb.host(), c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("Hi,Wi,Ho,Wo", SHAPES)
def test_bilinear_forward(dtype, mode, Hi, Wi, Ho, Wo):
    """ydl_resize_fwd, both kernels, per element within 6 U of the element's own sum w |v|: up- and down-sampling, one-row inputs, both
    align_corners conventions.  The reference shares no index or weight code with the kernels beyond the documented formula."""
    for C, wide in combos(dtype):
        _bilinear_fwd(dtype, mode, 2, Hi, Wi, Ho, Wo, C, wide)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bilinear_forward_with_a_given_scale(dtype):
    """scale_factor 2.05: the output is twice the input, the source coordinates follow 1 / 2.05"""
    for C, wide in combos(dtype):
        _bilinear_fwd(dtype, 1, 2, 10, 12, 20, 24, C, wide, g=1 / 2.05)


def _bilinear_bwd(dtype, mode, N, Hi, Wi, Ho, Wo, C, wide, g=0.0):
    L = G.lib()
    d, tdt, es, V = G.dt(dtype)
    dy = rng(Ho * 31 + Wi + C).randn(N, Ho, Wo, C)
    prev = rng(Ho + C).randn(N, Hi, Wi, C)
    lay = G.slice_layout(N * Hi * Wi, C, dtype, wide)
    integer = mode == 1 and g == 0.0 and Ho == Hi * (Wo // Wi) and Wo % Wi == 0 and Wo // Wi in (2, 4)
    for acc in (0, 1):
        c = R.case_resize_bwd(dy, mode, Hi, Wi, dtype, prev if acc else None, ld=lay.ld, lead=lay.lead, gh=g, gw=g)
        dyb = G.Buf(G.slice_layout(N * Ho * Wo, C, dtype, wide), tdt, c["dy"])
        for fast in ((1, 0) if integer else (1,)):
            dxb = G.Buf(lay, tdt, c["prev"]) if acc else G.Buf(lay, tdt)
            L.debug_set(10, fast)
            try:
                G.call("ydl_resize_bwd", d, mode, dyb.p, dyb.lay.ld, dxb.p, lay.ld, acc, N, Hi, Wi, Ho, Wo, C, g, g, G.stream())
                G.sync()
            finally:
                L.debug_set(10, 1)
            kern = "integer-factor" if (integer and fast) else "generic"
            G.check(f"bilinear backward | {kern} {dtype} mode {mode} {Hi}x{Wi}<-{Ho}x{Wo} C{C} wide={wide} acc={acc}", R.check_resize_bwd,
                    dxb.host(), c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("Hi,Wi,Ho,Wo", SHAPES + [(17, 13, 5, 4)])
def test_bilinear_backward(dtype, mode, Hi, Wi, Ho, Wo):
    """ydl_resize_bwd per element: the generic gather (its cand_range window at scales above 1: 40 -> 20, 17 x 13 -> 5 x 4, 300 -> 33) and
    the integer-factor kernel where the dispatch takes it (x2, x4, mode 1), overwrite and accumulate"""
    for C, wide in combos(dtype)[:2]:
        _bilinear_bwd(dtype, mode, 2, Hi, Wi, Ho, Wo, C, wide)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bilinear_backward_with_a_given_scale(dtype):
    C, wide = combos(dtype)[1]
    _bilinear_bwd(dtype, 1, 2, 10, 12, 20, 24, C, wide, g=1 / 2.05)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,N,Hi,Wi,Ho,Wo,C", [(1, 2, 10, 12, 40, 48, 24), (1, 3, 7, 9, 14, 18, 16), (2, 1, 5, 6, 17, 11, 8), (0, 2, 4, 4, 8, 8, 40),
                                                  (1, 2, 40, 40, 20, 20, 12)])
def test_resize_acc_sums_values_and_statistics(dtype, mode, N, Hi, Wi, Ho, Wo, C):
    """ydl_resize_acc_sums against float64 directly: y0 + resize(x) per element, and the per-channel (sum, sum of squares) of the float32
    results, bounded by the depth of the sum (pixels per thread, the threads of a chunk in LDS order, the replica atomics)"""
    L = G.lib()
    d, tdt, es, V = G.dt(dtype)
    Cp = R.rup(C, V)
    vals, stats = R.case_acc_sums(dtype, mode, N, Hi, Wi, Ho, Wo, C, rng(C).randn(N, Hi, Wi, C), rng(C + 1).randn(N, Ho, Wo, C))
    xb = G.Buf(R.Layout(N * Hi * Wi, Cp, C, Cp), tdt, vals["x"], pad=0.0)
    yb = G.Buf(vals["layout"], tdt, vals["y0"], pad=0.0)
    slay = R.Layout(2 * L.BN_REPLICAS, Cp + 4, Cp)
    sb = G.Buf(slay, torch.float32, np.zeros((2 * L.BN_REPLICAS, Cp)))
    G.call("ydl_resize_acc_sums", d, mode, xb.p, Cp, yb.p, Cp, N, Hi, Wi, Ho, Wo, C, 0.0, 0.0, sb.p, Cp + 4, G.stream())
    G.sync()
    tag = f"{dtype} mode {mode} {Hi}x{Wi}->{Ho}x{Wo} C{C}"
    G.check("resize_acc_sums values | " + tag, R.check_acc_sums, yb.host(), vals)
    sh = sb.host()
    assert slay.violations(sh) == 0, "statistics rows: sentinels"
    got = slay.answer(sh).astype(F64).reshape(L.BN_REPLICAS, 2, Cp).sum(0)[:, :C]
    G.check("resize_acc_sums statistics | " + tag, R.check_acc_sums, stats["layout"].embed(got, F64), stats)


# ---------------------------------------------------------------------------------------------------------------------------
# global average, the average branch of the backward, per-(n, c) dot, channel scaling
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW", HWS)
def test_global_average_and_max_of_random_planes(dtype, HW):
    """ydl_global_pool_fwd: the 256 strided partial sums and their merge, per (n, c); the maximum and its index of the same call exactly"""
    d, tdt, es, V = G.dt(dtype)
    N = 3
    for C, wide in combos(dtype) + [(7, True)]:
        Cp = R.rup(C, V)
        lay = G.slice_layout(N, C, dtype, wide)
        c = R.case_global_avg(rng(HW + C).randn(N, HW, C), dtype, ld=lay.ld, lead=lay.lead)
        xb = G.Buf(G.slice_layout(N * HW, C, dtype, wide), tdt, c["x"], pad=0.0)
        ab, mb = G.Buf(lay, tdt), G.Buf(lay, tdt)
        ib = G.Buf(R.Layout(N, Cp, C, Cp), torch.int32, sent=-7)
        G.call("ydl_global_pool_fwd", d, xb.p, xb.lay.ld, ab.p, lay.ld, mb.p, lay.ld, ib.p, N, HW, C, G.stream())
        G.sync()
        G.check(f"global average | {dtype} HW={HW} C={C} wide={wide}", R.check_global_avg, ab.host(), c)
        _, mx, am = R.global_pool_ref(c["x"])
        assert R.accepted(R.check_global_max(mb.host(), dict(layout=lay, ref=mx)))
        assert R.accepted(R.check_global_max(ib.host(), dict(layout=ib.lay, ref=am, sent=-7)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW", [5, 257, 1000])
def test_global_pool_backward_with_the_average_branch(dtype, HW):
    d, tdt, es, V = G.dt(dtype)
    N = 3
    for C, wide in combos(dtype)[:2]:
        Cp = R.rup(C, V)
        r = rng(HW + C)
        am = r.randint(0, HW, size=(N, C)).astype(np.int32)
        davg, dmx, prev = r.randn(N, C), r.randn(N, C), r.randn(N, HW, C)
        ib = G.Buf(R.Layout(N, Cp, C, Cp), torch.int32, am, pad=0, sent=-7)
        lay = G.slice_layout(N * HW, C, dtype, wide)
        sl = G.slice_layout(N, C, dtype, wide)
        for what, a, m in [("avg", davg, None), ("both", davg, dmx)]:
            for acc in (0, 1):
                c = R.case_global_pool_bwd(a, m, am, HW, dtype, prev if acc else None, ld=lay.ld, lead=lay.lead)
                ab = G.Buf(sl, tdt, c["davg"])
                mb = None if m is None else G.Buf(sl, tdt, c["dmx"])
                dxb = G.Buf(lay, tdt, c["prev"]) if acc else G.Buf(lay, tdt)
                G.call("ydl_global_pool_bwd", d, ab.p, sl.ld, mb.p if mb else None, sl.ld, ib.p, dxb.p, lay.ld, acc, N, HW, C, G.stream())
                G.sync()
                G.check(f"global pool backward | {dtype} HW={HW} C={C} {what} acc={acc}", R.check_rounded, dxb.host(), c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW", HWS)
def test_channel_dot(dtype, HW):
    d, tdt, es, V = G.dt(dtype)
    N = 3
    for C, wide in combos(dtype) + [(7, True)]:
        c = R.case_channel_dot(rng(HW + C).randn(N, HW, C), rng(HW + C + 1).randn(N, HW, C), dtype)
        ab = G.Buf(G.slice_layout(N * HW, C, dtype, wide), tdt, c["a"])
        bb = G.Buf(G.slice_layout(N * HW, C, dtype, not wide), tdt, c["b"])
        ob = G.Buf(c["layout"], torch.float32)
        G.call("ydl_channel_dot", d, ab.p, ab.lay.ld, bb.p, bb.lay.ld, ob.p, N, HW, C, G.stream())
        G.sync()
        G.check(f"channel_dot | {dtype} HW={HW} C={C} wide={wide}", R.check_channel_dot, ob.host(), c)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_channels(dtype):
    """one product per element; the pad channels [C, Cp) of the output are zeros whatever the input holds there"""
    d, tdt, es, V = G.dt(dtype)
    for HW in (1, 37, 300):
        for C, wide in combos(dtype) + [(7, True)]:
            lay = G.slice_layout(3 * HW, C, dtype, wide, pad="zero")
            c = R.case_scale_channels(rng(HW + C).randn(3, HW, C), rng(C).randn(3, C), dtype, ld=lay.ld, lead=lay.lead)
            xb = G.Buf(G.slice_layout(3 * HW, C, dtype, wide), tdt, c["x"])
            gb = torch.from_numpy(c["gate"]).cuda()
            yb = G.Buf(c["layout"], tdt)
            G.call("ydl_scale_channels", d, xb.p, xb.lay.ld, ctypes.c_void_p(gb.data_ptr()), yb.p, lay.ld, 3, HW, C, G.stream())
            G.sync()
            G.check(f"scale_channels | {dtype} HW={HW} C={C} wide={wide}", R.check_scale_channels, yb.host(), c)


# ---------------------------------------------------------------------------------------------------------------------------
# sigmoid gate
# ---------------------------------------------------------------------------------------------------------------------------
def _gate_inputs(N, C, seed):
    r = rng(seed)
    a, b = r.uniform(-15, 15, (N, C)), r.uniform(-15, 15, (N, C))
    a[0, :5], b[0, :5] = [30, -30, 30, 0, 12], [30, -30, -30, 0, 13]            # both saturations, the middle, a sum of 25
    return a, b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("C", [5, 64, 300])
def test_gate_forward_and_backward(dtype, N, C):
    """ydl_gate_fwd: sigmoid(a + b) with v_exp_f32 and v_rcp_f32 at 1 ulp each (csrc/common.h), inputs over [-60, 60] in the sum;
    ydl_gate_bwd: dgate g (1 - g) into both operands, every acc_a / acc_b combination; N C = 900 needs four CTAs"""
    d, tdt, es, V = G.dt(dtype)
    a, b = _gate_inputs(N, C, C + N)
    c = R.case_gate_fwd(a, b, dtype)
    ab = G.Buf(R.Layout(N, C + 3, C), tdt, c["a"])
    bb = G.Buf(R.Layout(N, C, C), tdt, c["b"])
    gb = G.Buf(c["layout"], torch.float32)
    G.call("ydl_gate_fwd", d, ab.p, C + 3, bb.p, C, gb.p, N, C, G.stream())
    G.sync()
    G.check(f"gate forward | {dtype} N={N} C={C}", R.check_gate, gb.host(), c)
    gate = c["layout"].answer(gb.host()).copy()
    dgate = rng(C).randn(N, C).astype(F32)
    dgb = G.Buf(R.Layout(N, C, C), torch.float32, dgate)
    gin = G.Buf(R.Layout(N, C, C), torch.float32, gate)
    pa, pb = rng(1).randn(N, C), rng(2).randn(N, C)
    for acc_a in (0, 1):
        for acc_b in (0, 1):
            ca = R.case_gate_bwd(gate, dgate, dtype, pa if acc_a else None, ld=C + 3)
            cb = R.case_gate_bwd(gate, dgate, dtype, pb if acc_b else None, ld=C)
            da = G.Buf(ca["layout"], tdt, ca["prev"]) if acc_a else G.Buf(ca["layout"], tdt)
            db = G.Buf(cb["layout"], tdt, cb["prev"]) if acc_b else G.Buf(cb["layout"], tdt)
            G.call("ydl_gate_bwd", d, gin.p, dgb.p, da.p, C + 3, acc_a, db.p, C, acc_b, N, C, G.stream())
            G.sync()
            G.check(f"gate backward | {dtype} N={N} C={C} da acc={acc_a}", R.check_gate, da.host(), ca)
            G.check(f"gate backward | {dtype} N={N} C={C} db acc={acc_b}", R.check_gate, db.host(), cb)


# ---------------------------------------------------------------------------------------------------------------------------
# group soft-max
# ---------------------------------------------------------------------------------------------------------------------------
def _group_softmax(dtype, npix, Gn, P, ld, seed=0, spread=8.0):
    d, tdt, es, V = G.dt(dtype)
    r = rng(seed + Gn * P + npix)
    c = R.case_group_softmax(r.uniform(-spread, spread, (npix, Gn * P)), Gn, P, dtype, ld=ld)
    xb = G.Buf(R.Layout(npix, ld, Gn * P), tdt, c["x"])
    yb = G.Buf(c["layout"], tdt)
    G.call("ydl_group_softmax_fwd", d, xb.p, ld, yb.p, ld, npix, Gn, P, G.stream())
    G.sync()
    tag = f"{dtype} npix={npix} G={Gn} P={P} ld={ld}"
    res = G.check("group soft-max forward | " + tag, R.check_group_softmax, yb.host(), c)
    if dtype == "f32":
        rel = float((np.abs(c["layout"].answer(yb.host()).astype(F64) - c["ref"]) / c["ref"]).max())
        print(f"  group soft-max forward relative | {tag}: gpu {rel:.2e}  bound {c['rel']:.2e}")
    y = c["layout"].answer(yb.host()).copy()
    dy, prev = r.randn(npix, Gn * P), r.randn(npix, Gn * P)
    for acc in (0, 1):
        cb = R.case_group_softmax_bwd(y, dy, Gn, P, dtype, prev if acc else None, ld=ld)
        pb = G.Buf(R.Layout(npix, ld, Gn * P), tdt, cb["y"])
        db = G.Buf(R.Layout(npix, Gn * P + 1, Gn * P), tdt, cb["dy"])
        ob = G.Buf(cb["layout"], tdt, cb["prev"]) if acc else G.Buf(cb["layout"], tdt)
        G.call("ydl_group_softmax_bwd", d, pb.p, ld, db.p, Gn * P + 1, ob.p, ld, acc, npix, Gn, P, G.stream())
        G.sync()
        G.check(f"group soft-max backward | {tag} acc={acc}", R.check_group_softmax, ob.host(), cb)
    return res


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Gn,P", [(1, 9), (4, 9), (3, 25)])
@pytest.mark.parametrize("npix", [1, 300])
def test_group_softmax_forward_and_backward(dtype, Gn, P, npix):
    for ld in (Gn * P, Gn * P + 3):
        _group_softmax(dtype, npix, Gn, P, ld)


def test_group_softmax_of_a_narrow_spread_shows_expf():
    """logits within 2^-4 of each other: the rounding of v - max and of its scaling by log2(e) stays under U / 4, so what is left of the
    relative error of a probability is __expf itself (twice: numerator and sum), one addition, the division and the product.  The
    printed figure is the one recorded in the module docstring."""
    _group_softmax("f32", 300, 4, 2, 8, spread=2.0 ** -5)


def test_group_softmax_grid_stride_second_trip():
    """npix G = 1 048 577 groups: one more than the 4096 x 256 threads of stream_grid's cap"""
    d, tdt, es, V = G.dt("f32")
    npix, P = 4096 * 256 + 1, 2
    c = R.case_group_softmax(rng(0).uniform(-8, 8, (npix, P)), 1, P, "f32")
    xb, yb = G.Buf(R.Layout(npix, P, P), tdt, c["x"]), G.Buf(c["layout"], tdt)
    G.call("ydl_group_softmax_fwd", d, xb.p, P, yb.p, P, npix, 1, P, G.stream())
    G.sync()
    G.check("group soft-max forward | second trip", R.check_group_softmax, yb.host(), c)


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm evaluation coefficients
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 7, 300])
def test_bn_eval_coeffs(C):
    """scale = gamma / sqrt(rv + eps), shift = beta - rm scale: sqrtf, one division, one product, one subtraction"""
    r = rng(C)
    c = R.case_bn_eval(r.randn(C), r.randn(C), r.randn(C), r.uniform(0.01, 2, C), 1e-3)
    dev = [torch.from_numpy(c[k]).cuda() for k in ("gamma", "beta", "rm", "rv")]
    ob = G.Buf(c["layout"], torch.float32)
    G.call("ydl_bn_eval_coeffs", C, *[ctypes.c_void_p(t.data_ptr()) for t in dev], 1e-3, ob.p, ctypes.c_void_p(ob.p.value + 4 * C), G.stream())
    G.sync()
    G.check(f"bn_eval_coeffs | C={C}", R.check_bn_eval, ob.host(), c)


# ---------------------------------------------------------------------------------------------------------------------------
# the second trip of the grid-stride loop of the resize backward, per element
# ---------------------------------------------------------------------------------------------------------------------------
def test_bilinear_backward_grid_stride_second_trip():
    """513 x 512 input pixels x 4 chunks (just over 4096 x 256 threads) gather from a 257 x 256 output: the generic kernel at a scale of
    about 1/2 downwards; the reference is the matrix form of the same operator (tests/test_spatial_ref_cpu.py holds it to the loop form)"""
    d, tdt, es, V = G.dt("f32")
    Hi, Wi, Ho, Wo, C = 513, 512, 257, 256, 16
    dy = rng(3).randint(-8, 9, size=(1, Ho, Wo, C)).astype(F32)
    c = R.case_resize_bwd(dy, 1, Hi, Wi, "f32", matrix=True)
    dyb = G.Buf(R.Layout(Ho * Wo, C, C), tdt, c["dy"])
    dxb = G.Buf(c["layout"], tdt)
    G.call("ydl_resize_bwd", d, 1, dyb.p, C, dxb.p, C, 0, 1, Hi, Wi, Ho, Wo, C, 0.0, 0.0, G.stream())
    G.sync()
    G.check("bilinear backward | second trip", R.check_resize_bwd, dxb.host(), c)
