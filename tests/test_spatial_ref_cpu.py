"""tests/spatial_ref.py held to torch on the CPU (float64 operators and autograd), the gap between its bilinear weights (float32, as the
kernels and ATen's float path form them) and F.interpolate(float64) derived and asserted, ATen's NaN rule of the global max pinned, and
the sensitivity of every comparison helper: wrong answers that were never on a GPU must be rejected, the float32 evaluation of the same
reference (the floor) accepted.  A wrong answer that a family cannot give (a tie rule for a resize, a weight swap for a copy) is not
listed for it."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import spatial_ref as R

F32, F64 = np.float32, np.float64
RESIZES = [(10, 12, 40, 48), (7, 9, 14, 18), (5, 6, 17, 11), (40, 40, 20, 20), (1, 5, 2, 10), (3, 300, 7, 33), (17, 13, 5, 4)]
POOLS = [(2, 2, 0), (3, 2, 1), (5, 1, 2), (3, 1, 1)]
POOL_CASES = [(k, s, p, H, W) for (k, s, p) in POOLS for (H, W) in [(7, 9), (1, 5), (12, 12)] if R.pool_out(H, k, s, p) >= 1]   # 2x2 / 2 has no 1 x 5 output
MODE = {0: dict(mode="nearest"), 1: dict(mode="bilinear", align_corners=False), 2: dict(mode="bilinear", align_corners=True)}


def rng(seed):
    return np.random.RandomState(seed)


def ties(seed, shape):
    return rng(seed).randint(-3, 4, size=shape).astype(F64)


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(np.asarray(a), -1, 1)))


def nhwc(t):
    return np.moveaxis(t.detach().numpy(), 1, -1)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference against torch
# ---------------------------------------------------------------------------------------------------------------------------
def _torch_codes(ind, H, W, k, s, p):
    """flat input index ih * W + iw of F.max_pool2d -> window offset ky * k + kx"""
    ind = nhwc(ind)
    N, Ho, Wo, C = ind.shape
    ih, iw = ind // W, ind % W
    ky = ih - (np.arange(Ho) * s - p)[None, :, None, None]
    kx = iw - (np.arange(Wo) * s - p)[None, None, :, None]
    return (ky * k + kx).astype(np.uint8)


@pytest.mark.parametrize("k,s,p,H,W", POOL_CASES)
def test_max_pool_values_codes_and_backward_equal_torch(k, s, p, H, W):
    x = ties(k * 100 + H, (2, H, W, 5))
    xt = nchw(x).requires_grad_(True)
    yt, it = F.max_pool2d(xt, k, s, p, return_indices=True)
    y, code = R.maxpool_ref(x, k, s, p)
    assert np.array_equal(y, nhwc(yt))
    assert np.array_equal(code, _torch_codes(it, H, W, k, s, p))
    dy = rng(3).randint(-2, 3, size=y.shape).astype(F64)
    yt.backward(nchw(dy))
    assert np.array_equal(R.maxpool_bwd_ref(dy, code, H, W, k, s, p), nhwc(xt.grad))
    prev = rng(4).randint(-4, 5, size=x.shape).astype(F64)
    assert np.array_equal(R.maxpool_bwd_ref(dy, code, H, W, k, s, p, prev), nhwc(xt.grad) + prev)


def test_max_pool_nan_rule_is_atens():
    x = ties(5, (1, 6, 6, 3))
    x[0, 2, 3, 0] = np.nan
    x[0, 2, 4, 0] = np.nan
    x[0, 5, 5, 1] = np.nan
    yt, it = F.max_pool2d(nchw(x), 3, 1, 1, return_indices=True)
    y, code = R.maxpool_ref(x, 3, 1, 1)
    assert np.array_equal(y, nhwc(yt), equal_nan=True)
    assert np.array_equal(code, _torch_codes(it, 6, 6, 3, 1, 1))


def _interp(x, mode, Ho, Wo, sf, dtype):
    xt = nchw(x).to(dtype).requires_grad_(True)
    if sf is None:
        y = F.interpolate(xt, size=(Ho, Wo), **MODE[mode])
    else:
        y = F.interpolate(xt, scale_factor=sf, recompute_scale_factor=False, **MODE[mode])
    assert tuple(y.shape[-2:]) == (Ho, Wo)
    return xt, y


def _resize_cases():
    out = [(m, hi, wi, ho, wo, None) for m in (0, 1, 2) for (hi, wi, ho, wo) in RESIZES]
    # (nearest with a given scale: ATen takes ``dst >> 1`` whenever the output is twice the input, whatever the scale says; the kernels
    #  follow include/ydl.h, min(floor(dst * scale), in - 1), for every size, so the two are compared where ATen evaluates that formula)
    out += [(0, 10, 12, 23, 28, 2.35), (1, 10, 12, 20, 24, 2.05), (1, 9, 7, 4, 3, 0.5)]
    return out


@pytest.mark.parametrize("mode,Hi,Wi,Ho,Wo,sf", _resize_cases())
def test_resize_forward_and_backward_against_interpolate(mode, Hi, Wi, Ho, Wo, sf):
    """float32: same indices and weights as ATen's float path, so the float64 combination of those float32 weights is within the
    roundings of ATen's own float32 combination.  float64: the restated result differs from F.interpolate(float64) only through the
    float32 weights: the gap is bounded from the weight rounding (interpolate_gap_bound) and asserted.  Nearest: exact."""
    x = rng(mode * 7 + Hi).randn(2, Hi, Wi, 3).astype(F32)
    g = 0.0 if sf is None else 1.0 / sf
    th, tw = R.axis_taps(mode, Hi, Ho, g), R.axis_taps(mode, Wi, Wo, g)
    ref, mag = R.resize_fwd_ref(x.astype(F64), th, tw)
    assert np.abs(R.resize_fwd_matrix(x, th, tw) - ref).max() <= 4 * 2.0 ** -53 * mag.max()
    x32, y32 = _interp(x, mode, Ho, Wo, sf, torch.float32)
    x64, y64 = _interp(x, mode, Ho, Wo, sf, torch.float64)
    dy = rng(5).randn(*ref.shape).astype(F32)
    y64.backward(nchw(dy).double())
    dref, dmag, cnt = R.resize_bwd_ref(dy.astype(F64), th, tw, Hi, Wi)
    dmat = R.resize_bwd_matrix(dy, th, tw, Hi, Wi)
    assert np.abs(dmat[0] - dref).max() <= 2.0 ** -50 * dmag.max() and np.array_equal(dmat[2], cnt)
    if mode == 0:
        assert np.array_equal(ref, nhwc(y64)) and np.array_equal(ref.astype(F32), nhwc(y32))
        assert np.array_equal(dref, nhwc(x64.grad))
        return
    # (ATen's CPU build may contract scale * (dst + 0.5) - 0.5 into one fused multiply-add, which the kernels forbid themselves: its
    #  float32 source coordinate then differs by one rounding of the product, at most (in + 0.5) U per axis, and a weight with it)
    e32 = np.abs(nhwc(y32).astype(F64) - ref)
    fma_gap = 2 * float(np.abs(x).max()) * ((Hi + 0.5) + (Wi + 0.5)) * R.U
    print(f"  interpolate(float32) against the restated weights: {float(e32.max()):.2e}, allowed {float((6 * R.U * mag).max() + fma_gap):.2e}")
    assert (e32 <= 6 * R.U * mag + R.U * np.abs(ref) + fma_gap).all()
    gap = float(np.abs(nhwc(y64) - ref).max())
    gap_bound = R.interpolate_gap_bound(x, mode, Hi, Wi, Ho, Wo)
    print(f"  interpolate gap mode {mode} {Hi}x{Wi}->{Ho}x{Wo} sf={sf}: measured {gap:.2e}  derived bound {gap_bound:.2e}")
    assert gap <= gap_bound
    # backward: every output moves its weight by at most the same dw per axis; an input element collects that from the outputs that
    # reference it through the float32 or the exact taps
    eh, ew = R.exact_taps(mode, Hi, Ho, g), R.exact_taps(mode, Wi, Wo, g)
    Ah = ((R.axis_matrix(th, Hi) != 0) | (R.axis_matrix(eh, Hi) != 0)).astype(F64)
    Aw = ((R.axis_matrix(tw, Wi) != 0) | (R.axis_matrix(ew, Wi) != 0)).astype(F64)
    S = np.einsum("ah,nabc,bw->nhwc", Ah, np.abs(dy).astype(F64), Aw)
    dw = ((3 * (Hi + 0.5) + 1) + (3 * (Wi + 0.5) + 1)) * R.U
    bgap = np.abs(nhwc(x64.grad) - dref)
    print(f"  interpolate backward gap: measured {float(bgap.max()):.2e}  derived bound {float((dw * S).max()):.2e}")
    assert (bgap <= dw * S + 1e-300).all()
    # and the exact-weight form of the same expressions IS F.interpolate(float64), to float64 rounding
    assert np.abs(R.resize_fwd_ref(x.astype(F64), eh, ew)[0] - nhwc(y64)).max() <= 8 * 2.0 ** -53 * np.abs(x).max()


@pytest.mark.parametrize("HW", [1, 5, 255, 256, 257, 1000])
def test_global_pools_against_adaptive_pools(HW):
    x = ties(HW, (3, HW, 5))
    xt = torch.from_numpy(x.transpose(0, 2, 1).reshape(3, 5, 1, HW).copy()).requires_grad_(True)
    avg, mx, am = R.global_pool_ref(x)
    mt, it = F.adaptive_max_pool2d(xt, 1, return_indices=True)
    at = F.adaptive_avg_pool2d(xt, 1)
    assert np.array_equal(mx, mt.detach().numpy()[:, :, 0, 0]) and np.array_equal(am, it.numpy()[:, :, 0, 0])
    assert np.allclose(avg, at.detach().numpy()[:, :, 0, 0], rtol=1e-14, atol=0)
    davg, dmx = rng(1).randn(3, 5), rng(2).randn(3, 5)
    (at[:, :, 0, 0] * torch.from_numpy(davg)).sum().backward(retain_graph=True)
    ga = xt.grad.clone()
    xt.grad = None
    (mt[:, :, 0, 0] * torch.from_numpy(dmx)).sum().backward()
    gm = xt.grad
    to = lambda t: t.numpy().reshape(3, 5, HW).transpose(0, 2, 1)
    assert np.allclose(R.global_pool_bwd_ref(davg, None, am, HW), to(ga), rtol=1e-14, atol=0)
    assert np.array_equal(R.global_pool_bwd_ref(None, dmx, am, HW), to(gm))
    assert np.allclose(R.global_pool_bwd_ref(davg, dmx, am, HW), to(ga) + to(gm), rtol=1e-14, atol=0)


NAN_HW = 1000
NAN_ONE, NAN_TWO = [601], [300, 777]           # pixels owned by threads 601 % 256 = 89, 300 % 256 = 44 and 777 % 256 = 9: none is thread 0


@pytest.mark.parametrize("where", [NAN_ONE, NAN_TWO], ids=["one", "two"])
def test_what_adaptive_max_pool_returns_for_nan(where):
    """pinned on this torch: the pooled value is NaN and the index is that of the LAST NaN (ATen scans with ``v > best || isnan(v)``);
    global_pool_ref says the same, and the gradient of the max branch goes to that index"""
    x = ties(9, (1, NAN_HW, 2))
    x[0, where, 0] = np.nan
    xt = torch.from_numpy(x.transpose(0, 2, 1).reshape(1, 2, 25, 40).copy()).requires_grad_(True)
    mt, it = F.adaptive_max_pool2d(xt, 1, return_indices=True)
    assert math.isnan(float(mt.detach()[0, 0, 0, 0])) and int(it[0, 0, 0, 0]) == where[-1]
    avg, mx, am = R.global_pool_ref(x)
    assert np.isnan(mx[0, 0]) and am[0, 0] == where[-1] and am[0, 1] == int(it[0, 1, 0, 0]) and mx[0, 1] == float(mt.detach()[0, 1, 0, 0])
    mt[0, 0, 0, 0].backward()
    assert int(xt.grad.reshape(2, -1)[0].argmax()) == where[-1]
    assert R.global_pool_bwd_ref(None, np.ones((1, 2)), am, NAN_HW)[0, :, 0].argmax() == where[-1]


def test_small_expressions_against_torch():
    r = rng(0)
    a, b = r.uniform(-30, 30, (3, 7)), r.uniform(-30, 30, (3, 7))
    at, bt = torch.from_numpy(a).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    gt = torch.sigmoid(at + bt)
    assert np.allclose(R.gate_fwd_ref(a, b), gt.detach().numpy(), rtol=1e-13, atol=1e-300)
    dg = r.randn(3, 7)
    gt.backward(torch.from_numpy(dg))
    assert np.allclose(R.gate_bwd_ref(gt.detach().numpy(), dg), at.grad.numpy(), rtol=1e-12, atol=1e-300)
    assert np.array_equal(at.grad.numpy(), bt.grad.numpy())
    x, y = r.randn(2, 11, 5), r.randn(2, 11, 5)
    assert np.allclose(R.channel_dot_ref(x, y), (torch.from_numpy(x) * torch.from_numpy(y)).sum(1).numpy(), rtol=1e-13)
    assert np.array_equal(R.scale_channels_ref(x, a[:2, :5]), (torch.from_numpy(x) * torch.from_numpy(a[:2, :5])[:, None]).numpy())
    for G, P in [(1, 9), (4, 9), (3, 25)]:
        v = r.uniform(-8, 8, (6, G * P))
        vt = torch.from_numpy(v).requires_grad_(True)
        st = torch.softmax(vt.view(6, G, P), 2).reshape(6, G * P)
        assert np.allclose(R.group_softmax_ref(v, G, P), st.detach().numpy(), rtol=1e-13)
        dy = r.randn(6, G * P)
        st.backward(torch.from_numpy(dy))
        assert np.allclose(R.group_softmax_bwd_ref(st.detach().numpy(), dy, G, P), vt.grad.numpy(), rtol=1e-11, atol=1e-16)
    g, be, m, var = r.randn(7), r.randn(7), r.randn(7), r.uniform(0.1, 2, 7)
    x = torch.from_numpy(r.randn(4, 7, 3, 3))
    want = F.batch_norm(x, torch.from_numpy(m), torch.from_numpy(var), torch.from_numpy(g), torch.from_numpy(be), False, 0.0, 1e-3)
    sc, sh = R.bn_eval_ref(g, be, m, var, 1e-3)
    assert np.allclose((x * torch.from_numpy(sc)[None, :, None, None] + torch.from_numpy(sh)[None, :, None, None]).numpy(), want.numpy(),
                       rtol=1e-12, atol=1e-13)


# ---------------------------------------------------------------------------------------------------------------------------
# checker sensitivity: the float32 floor is accepted, every wrong answer rejected
# ---------------------------------------------------------------------------------------------------------------------------
def _accept(check, got, case, what):
    res = check(got, case)
    print(f"  {what}: error {res[0]:.2e} floor {res[1]:.2e} bound {res[2]:.2e}")
    assert res[1] <= res[2], (what, "the float32 floor misses the bound", res)
    assert R.accepted(res), (what, res)


def _reject(check, got, case, what):
    res = check(got, case)
    assert not R.accepted(res), (what, "a wrong answer passes", res)


def _sentinel_variants(lay, buf):
    """one sentinel overwritten: in front, behind, and (where the rows are wider than what is written) between the rows"""
    out = []
    for pos in [lay.lead - 1, lay.lead + lay.rows * lay.ld]:
        b = buf.copy()
        b[pos] = 1
        out.append(b)
    if lay.ld > lay.Cw:
        b = buf.copy()
        lay.rows_of(b)[lay.rows // 2, lay.Cw] = 0
        out.append(b)
    return out


def _swap(t):
    return t[0], t[1], t[3], t[2]


def _last_off(t):
    i0, i1, w0, w1 = t
    i0, i1 = i0.copy(), i1.copy()
    i0[-1] = max(i0[-1] - 1, 0) if i0[-1] > 0 else 1
    i1[-1] = i0[-1]
    return i0, i1, w0, w1


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mode,Hi,Wi,Ho,Wo", [(1, 5, 6, 17, 11), (2, 5, 6, 17, 11), (1, 40, 40, 20, 20), (1, 7, 9, 14, 18), (2, 17, 13, 5, 4)])
def test_bilinear_checkers_reject_wrong_answers(dtype, mode, Hi, Wi, Ho, Wo):
    C = 8 if dtype == "bf16" else 4
    x = rng(Hi).randn(2, Hi, Wi, C)
    for ld in (C, C + 8):
        c = R.case_bilinear(x, mode, Ho, Wo, dtype, ld=ld)
        lay = c["layout"]
        good = lay.embed(c["floor"])
        _accept(R.check_bilinear, good, c, f"bilinear forward mode {mode} {dtype} ld {ld}")
        xs = c["x"].astype(F64)
        for what, th, tw in [("row weights swapped", _swap(c["th"]), c["tw"]), ("column weights swapped", c["th"], _swap(c["tw"])),
                             ("last row off by one", _last_off(c["th"]), c["tw"]), ("last column off by one", c["th"], _last_off(c["tw"]))]:
            if "swapped" in what and np.array_equal(c["th"][2], c["th"][3]) and np.array_equal(c["tw"][2], c["tw"][3]):
                continue                                    # exact halving: both weights are 1/2 everywhere and the swap is no error
            wrong = R.store(R.resize_fwd_ref(xs, th, tw)[0].astype(F32), dtype)
            _reject(R.check_bilinear, lay.embed(wrong), c, what)
        for b in _sentinel_variants(lay, good):
            _reject(R.check_bilinear, b, c, "sentinel")
    dy = rng(Ho).randn(2, Ho, Wo, C)
    prev = rng(Wo).randn(2, Hi, Wi, C)
    for acc in (0, 1):
        c = R.case_resize_bwd(dy, mode, Hi, Wi, dtype, prev if acc else None, ld=C + 8)
        lay = c["layout"]
        good = lay.embed(c["floor"])
        _accept(R.check_resize_bwd, good, c, f"bilinear backward mode {mode} {dtype} acc {acc}")
        d64, p64 = c["dy"].astype(F64), (c["prev"].astype(F64) if acc else None)
        for what, th, tw in [("row weights swapped", _swap(c["th"]), c["tw"]), ("column weights swapped", c["th"], _swap(c["tw"])),
                             ("last row off by one", _last_off(c["th"]), c["tw"]), ("last column off by one", c["th"], _last_off(c["tw"]))]:
            if "swapped" in what and np.array_equal(c["th"][2], c["th"][3]) and np.array_equal(c["tw"][2], c["tw"][3]):
                continue
            wrong = R.store(R.resize_bwd_ref(d64, th, tw, Hi, Wi, p64)[0].astype(F32), dtype)
            _reject(R.check_resize_bwd, lay.embed(wrong), c, what)
        if acc:
            wrong = R.store(R.resize_bwd_ref(d64, c["th"], c["tw"], Hi, Wi)[0].astype(F32), dtype)
            _reject(R.check_resize_bwd, lay.embed(wrong), c, "accumulate without the previous contents")
        for b in _sentinel_variants(lay, good):
            _reject(R.check_resize_bwd, b, c, "sentinel")


@pytest.mark.parametrize("Hi,Wi,Ho,Wo,g", [(4, 4, 8, 8, 0.0), (5, 6, 17, 11, 0.0), (40, 40, 20, 20, 0.0), (3, 300, 7, 33, 0.0), (10, 12, 20, 24, 1 / 2.05)])
def test_nearest_checker_rejects_wrong_answers(Hi, Wi, Ho, Wo, g):
    x = rng(Hi).randint(-3, 4, size=(2, Hi, Wi, 8)) + np.arange(Hi * Wi).reshape(Hi, Wi)[None, :, :, None] * 8.0   # every pixel distinct
    c = R.case_bilinear(x, 0, Ho, Wo, "bf16", ld=16, gh=g, gw=g)
    lay = c["layout"]
    good = lay.embed(c["floor"])
    _accept(R.check_nearest, good, dict(c, ref=c["floor"]), "nearest")
    _accept(R.check_bilinear, good, c, "nearest through the per-element checker")
    for what, th, tw in [("last row off by one", _last_off(c["th"]), c["tw"]), ("last column off by one", c["th"], _last_off(c["tw"]))]:
        wrong = R.resize_fwd_ref(c["x"].astype(F64), th, tw)[0]
        _reject(R.check_nearest, lay.embed(wrong), dict(c, ref=c["floor"]), what)
    for b in _sentinel_variants(lay, good):
        _reject(R.check_nearest, b, dict(c, ref=c["floor"]), "sentinel")


@pytest.mark.parametrize("k,s,p", POOLS)
def test_max_pool_checker_rejects_wrong_answers(k, s, p):
    H, W, C, Cp = 7, 9, 20, 24
    x = ties(k, (2, H, W, C))
    y, code = R.maxpool_ref(x, k, s, p)
    Ho, Wo = y.shape[1:3]
    lay = R.Layout(2 * Ho * Wo, Cp + 8, C, Cp)
    layc = R.Layout(2 * Ho * Wo, Cp, C, Cp)
    cy, cc = dict(layout=lay, ref=y), dict(layout=layc, ref=code, sent=255)
    good_c = layc.embed(code, np.uint8, 0, 255)
    _accept(R.check_maxpool, lay.embed(y), cy, "values")
    _accept(R.check_maxpool, good_c, cc, "codes")
    y2, code2 = R.maxpool_ref(x, k, s, p, last_tie=True)
    assert np.array_equal(y2, y) and not np.array_equal(code2, code), "the data must hold ties"
    _reject(R.check_maxpool, layc.embed(code2, np.uint8, 0, 255), cc, "tie broken towards the last maximum")
    # one code moved to an equal-valued neighbour
    n, ho, wo, ch = np.argwhere(code2 != code)[0]
    moved = code.copy()
    moved[n, ho, wo, ch] = code2[n, ho, wo, ch]
    _reject(R.check_maxpool, layc.embed(moved, np.uint8, 0, 255), cc, "one arg-max code moved to an equal-valued neighbour")
    for b in _sentinel_variants(lay, lay.embed(y)):
        _reject(R.check_maxpool, b, cy, "sentinel")
    b = good_c.copy()
    b[layc.lead - 1] = 0
    _reject(R.check_maxpool, b, cc, "sentinel in front of the codes")
    dy = rng(1).randint(-2, 3, size=y.shape).astype(F64)
    prev = rng(2).randint(-4, 5, size=x.shape).astype(F64)
    layx = R.Layout(2 * H * W, Cp, C, Cp)
    cb = dict(layout=layx, ref=R.maxpool_bwd_ref(dy, code, H, W, k, s, p, prev))
    _accept(R.check_maxpool, layx.embed(cb["ref"]), cb, "backward")
    _reject(R.check_maxpool, layx.embed(R.maxpool_bwd_ref(dy, code, H, W, k, s, p)), cb, "accumulate without the previous contents")
    _reject(R.check_maxpool, layx.embed(R.maxpool_bwd_ref(dy, moved, H, W, k, s, p, prev)), cb, "gradient routed by a moved code")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("HW", [5, 257, 1000])
def test_global_pool_checkers_reject_wrong_answers(dtype, HW):
    C = 12 if dtype == "f32" else 20
    Cp = R.rup(C, R.vec(dtype))
    x = ties(HW, (3, HW, C))
    c = R.case_global_avg(x, dtype, ld=Cp + 8)
    lay = c["layout"]
    good = lay.embed(c["floor"])
    _accept(R.check_global_avg, good, c, f"global average HW {HW} {dtype}")
    for b in _sentinel_variants(lay, good):
        _reject(R.check_global_avg, b, c, "sentinel")
    avg, mx, am = R.global_pool_ref(x)
    _, _, am_last = R.global_pool_ref(x, last_tie=True)
    laym = R.Layout(3, Cp, C, Cp)
    cm = dict(layout=laym, ref=am, sent=-7)
    _accept(R.check_global_max, laym.embed(am, np.int32, 0, -7), cm, "arg-max")
    assert not np.array_equal(am, am_last)
    _reject(R.check_global_max, laym.embed(am_last, np.int32, 0, -7), cm, "tie broken towards the last maximum")
    moved = am.copy()
    n, ch = np.argwhere(am_last != am)[0]
    moved[n, ch] = am_last[n, ch]
    _reject(R.check_global_max, laym.embed(moved, np.int32, 0, -7), cm, "one arg-max moved to an equal-valued pixel")
    dmx = rng(2).randint(-2, 3, (3, C)).astype(F64)
    prev = rng(3).randint(-4, 5, (3, HW, C)).astype(F64)
    layx = R.Layout(3 * HW, Cp, C, Cp)
    cb = dict(layout=layx, ref=R.global_pool_bwd_ref(None, dmx, am, HW, prev))
    _accept(R.check_global_max, layx.embed(cb["ref"]), cb, "backward of the max branch")
    _reject(R.check_global_max, layx.embed(R.global_pool_bwd_ref(None, dmx, am, HW)), cb, "accumulate without the previous contents")
    _reject(R.check_global_max, layx.embed(R.global_pool_bwd_ref(None, dmx, moved, HW, prev)), cb, "gradient at a moved arg-max")


def test_the_average_divided_by_hw_minus_one_is_rejected_in_float32():
    """(with a bf16 store the two differ by 1 / (HW - 1) relative, less than the store's own rounding from HW = 258 on: the float32
    cases are the ones that can tell)"""
    for HW in (5, 255, 256, 257, 1000):
        x = rng(HW).uniform(1, 3, (3, HW, 12))
        c = R.case_global_avg(x, "f32")
        _accept(R.check_global_avg, c["layout"].embed(c["floor"]), c, f"HW {HW}")
        wrong = R.global_pool_ref(c["x"].astype(F64), div=HW - 1)[0].astype(F32)
        _reject(R.check_global_avg, c["layout"].embed(wrong), c, f"the average divided by HW - 1, HW {HW}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_exact_family_checkers_reject_wrong_answers(dtype):
    """copy2d, layout, zero fills, casts and the chunk reduction share check_exact: the accumulate form without the previous contents,
    a non-zero pad channel where zeros are documented, one sentinel, one element off by one unit in the last place"""
    C, Cp, rows = 12, R.rup(12, R.vec(dtype)), 9
    src = rng(1).randint(-2, 3, (rows, C)).astype(F64)
    prev = rng(2).randint(-4, 5, (rows, C)).astype(F64)
    lay = R.Layout(rows, Cp + 8, C, Cp, "zero")
    c = dict(layout=lay, ref=src + prev)
    good = lay.embed(src + prev)
    _accept(R.check_copy2d, good, c, "accumulate form")
    _reject(R.check_copy2d, lay.embed(src), c, "the accumulate form without the previous contents")
    if Cp > C:
        _reject(R.check_layout, lay.embed(src + prev, pad_value=1.0), c, "one pad channel non-zero")
        b = good.copy()
        lay.rows_of(b)[3, C] = 2.0 ** -20
        _reject(R.check_layout, b, c, "one pad channel non-zero")
    for b in _sentinel_variants(lay, good):
        _reject(R.check_copy2d, b, c, "sentinel")
    b = good.copy()
    lay.rows_of(b)[rows - 1, C - 1] = np.nextafter(F32(lay.rows_of(b)[rows - 1, C - 1]), F32(100))
    _reject(R.check_cast, b, c, "one unit in the last place")
    # the chunk reduction's contract is the float32 sum in the order r = 0, 1, ...: another order differs in the last place
    ch = np.array([[2.0 ** 24], [1.0], [1.0], [-2.0 ** 24]], dtype=F32)
    fwd = np.cumsum(ch, axis=0, dtype=F32)[-1]
    rev = np.cumsum(ch[::-1], axis=0, dtype=F32)[-1]
    assert fwd[0] != rev[0]
    lay1 = R.Layout(1, 1, 1)
    _accept(R.check_reduce, lay1.embed(fwd), dict(layout=lay1, ref=fwd), "chunks in order")
    _reject(R.check_reduce, lay1.embed(rev), dict(layout=lay1, ref=fwd), "chunks in another order")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_small_expression_checkers_reject_wrong_answers(dtype):
    r = rng(3)
    C = 12 if dtype == "f32" else 20
    # channel scaling: pad channels are documented as 0
    x, gate = r.randn(2, 9, C), r.uniform(0, 1, (2, C))
    c = R.case_scale_channels(x, gate, dtype, ld=R.rup(C, R.vec(dtype)) + 8)
    lay = c["layout"]
    good = lay.embed(c["floor"])
    _accept(R.check_scale_channels, good, c, "scale_channels")
    if lay.Cw > lay.C:
        _reject(R.check_scale_channels, lay.embed(c["floor"], pad_value=2.0 ** -30), c, "one pad channel non-zero")
    _reject(R.check_scale_channels, lay.embed(R.store(R.scale_channels_ref(c["x"], np.roll(c["gate"], 1, 0), F32), dtype)), c, "the other image's gate")
    for b in _sentinel_variants(lay, good):
        _reject(R.check_scale_channels, b, c, "sentinel")
    # per-(n, c) dot
    for HW in (5, 257, 1000):
        a, b = r.randn(3, HW, C), r.randn(3, HW, C)
        c = R.case_channel_dot(a, b, dtype)
        _accept(R.check_channel_dot, c["layout"].embed(c["floor"]), c, f"channel_dot HW {HW}")
        wrong = R.channel_dot_ref(c["a"][:, :-1], c["b"][:, :-1]).astype(F32)
        _reject(R.check_channel_dot, c["layout"].embed(wrong), c, "the last pixel left out")
    # gate
    a, b = r.uniform(-15, 15, (3, 64)), r.uniform(-15, 15, (3, 64))
    a[0, :4], b[0, :4] = [30, -30, 30, 0], [30, -30, -30, 0]
    c = R.case_gate_fwd(a, b, dtype)
    _accept(R.check_gate, c["layout"].embed(c["floor"]), c, "gate forward")
    _reject(R.check_gate, c["layout"].embed(c["floor"] * F32(1 + 2.0 ** -18)), c, "gate off by 2^-18")
    _reject(R.check_gate, c["layout"].embed(R.gate_fwd_ref(c["a"], -c["b"], F32)), c, "a - b")
    g, dg, prev = c["floor"], r.randn(3, 64), r.randn(3, 64)
    for acc in (0, 1):
        cb = R.case_gate_bwd(g, dg, dtype, prev if acc else None, ld=72)
        _accept(R.check_gate, cb["layout"].embed(cb["floor"]), cb, f"gate backward acc {acc}")
        if acc:
            _reject(R.check_gate, cb["layout"].embed(R.store(R.gate_bwd_ref(g, dg, F32), dtype)), cb, "accumulate without the previous contents")
        _reject(R.check_gate, cb["layout"].embed(R.store((dg * g).astype(F32) + (cb["prev"] if acc else 0), dtype)), cb, "the factor 1 - g left out")
        for bb in _sentinel_variants(cb["layout"], cb["layout"].embed(cb["floor"])):
            _reject(R.check_gate, bb, cb, "sentinel")
    # group soft-max
    for G, P in [(1, 9), (4, 9), (3, 25)]:
        v = r.uniform(-8, 8, (7, G * P))
        c = R.case_group_softmax(v, G, P, dtype, ld=G * P + 3)
        _accept(R.check_group_softmax, c["layout"].embed(c["floor"]), c, f"group soft-max {G}x{P}")
        if G > 1:
            _reject(R.check_group_softmax, c["layout"].embed(R.store(R.group_softmax_ref(c["x"], 1, G * P, F32), dtype)), c, "one soft-max over all groups")
        _reject(R.check_group_softmax, c["layout"].embed(R.store(R.group_softmax_ref(c["x"] * F32(1.01), G, P, F32), dtype)), c, "logits scaled by 1.01")
        y, dy, prev = c["floor"], r.randn(7, G * P), r.randn(7, G * P)
        for acc in (0, 1):
            cb = R.case_group_softmax_bwd(y, dy, G, P, dtype, prev if acc else None, ld=G * P + 3)
            _accept(R.check_group_softmax, cb["layout"].embed(cb["floor"]), cb, f"group soft-max backward acc {acc}")
            if acc:
                _reject(R.check_group_softmax, cb["layout"].embed(R.store(R.group_softmax_bwd_ref(cb["y"], cb["dy"], G, P, None, F32), dtype)), cb,
                        "accumulate without the previous contents")
            if G > 1:
                _reject(R.check_group_softmax, cb["layout"].embed(R.store(R.group_softmax_bwd_ref(cb["y"], cb["dy"], 1, G * P, cb["prev"], F32), dtype)), cb,
                        "the dot over all groups")
    # BatchNorm evaluation coefficients
    c = R.case_bn_eval(r.randn(7), r.randn(7), r.randn(7), r.uniform(0.01, 2, 7), 1e-3)
    _accept(R.check_bn_eval, c["layout"].embed(c["floor"]), c, "bn_eval_coeffs")
    w = R.bn_eval_ref(c["gamma"], c["beta"], c["rm"], c["rv"], 1.1e-3, F32)
    _reject(R.check_bn_eval, c["layout"].embed(np.stack(w)), c, "another eps")


def test_acc_sums_checker():
    N, Hi, Wi, Ho, Wo, C = 2, 5, 6, 17, 11, 8
    for dtype in ("f32", "bf16"):
        vals, stats = R.case_acc_sums(dtype, 1, N, Hi, Wi, Ho, Wo, C, rng(1).randn(N, Hi, Wi, C), rng(2).randn(N, Ho, Wo, C))
        lay = vals["layout"]
        _accept(R.check_acc_sums, lay.embed(vals["floor"]), vals, f"values {dtype}")
        resized = R.resize_fwd_ref(vals["x"], *[R.axis_taps(1, a, b) for a, b in ((Hi, Ho), (Wi, Wo))], F32)[0]
        _reject(R.check_acc_sums, lay.embed(R.store(resized, dtype)), vals, "the accumulate form without the previous contents")
        for b in _sentinel_variants(lay, lay.embed(vals["floor"])):
            _reject(R.check_acc_sums, b, vals, "sentinel")
        lay = stats["layout"]
        _accept(R.check_acc_sums, lay.embed(stats["floor"]), stats, f"statistics {dtype}")
        _reject(R.check_acc_sums, lay.embed(R.acc_sums_ref(resized).astype(F32)), stats, "statistics of the resized part alone")
        _reject(R.check_acc_sums, lay.embed(R.acc_sums_ref(vals["ref"][:, :-1]).astype(F32)), stats, "the last row left out")
        _reject(R.check_acc_sums, lay.embed(R.acc_sums_ref(R.store(vals["ref"].astype(F32), "bf16")).astype(F32)), stats,
                "statistics of values rounded to bf16: they are taken before the store")
