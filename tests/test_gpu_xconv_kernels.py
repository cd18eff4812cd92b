"""GPU: the cross-convolution kernels (ydl_xconv_fwd / _dgrad / _wgrad) through the C ABI against float64 ``F.conv2d``,
``torch.nn.grad.conv2d_input`` and ``conv2d_weight`` on the CPU, on the same operands: x, dy and dx0 rounded to the compute dtype first,
and the weight the kernels read (the master rounded to the compute dtype by ydl_weight_prep with kk = k).  Scheme and helpers of
tests/test_gpu_gconv_kernels.py.

Bounds are derived, not tuned.  An output is a sum of K = k*Cin products accumulated in f32 (one rounding per product of a partial sum
no larger than S, the same convolution of absolute values), so |err| <= K * 2^-24 * S; the bound used is twice that, plus 2^-8 |ref| for
the bf16 rounding of the store.  With ``accumulate`` the previous value joins the sum: one more term and one more rounding.  A weight
gradient sums n = N*Ho*Wo products: 2 * n * 2^-24 * S.  (At stride 2 an input gradient has fewer than k*Cout terms: the bound holds.)

x is read from the upper half and y is written into the lower half of buffers twice as wide that are filled with a NaN sentinel: the
other half keeps it (and a kernel that read it would spread NaNs), as does the guarded statistics workspace beyond its rows.  The
rows, finalised by ydl_bn_finalize, are the float64 mean / variance of the STORED output at BN_STATS_TOLS[0] of
tests/test_gpu_bn_statistics.py.  Two weight-gradient runs are bitwise equal; dw and dx accumulate.

The wrap tests aim at the two classic errors of a shifted read.  W axis: an x that is non-zero only in the last column gives an output
column 0 of zeros, bit for bit (a tap that wraps reads the end of the previous row).  H axis: an x that is non-zero only in the last
row of sample 0 gives a row 0 of sample 1 of zeros (a tap that wraps reads the previous sample).  The same for the input gradient."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_bn_statistics import BN_STATS_TOLS, EPS, MOM, SENT, _bn_errors, _coef_buffers, _guarded_ws, _intact, _sentinel
from tests.test_gpu_gconv_kernels import MIB, _P, _st, half_ptr, raw, sentinel_like, to_nchw, wide

pytestmark = pytest.mark.gpu

W_, H_ = 0, 1
# tag -> (N, H, W, Cin, Cout, axis, k, s)
CASES = {"a_w3": (2, 9, 7, 16, 24, W_, 3, 1),            # 126 pixels: a tile boundary in mid-row
         "b_h3": (2, 9, 7, 16, 24, H_, 3, 1),            # a tile boundary between samples
         "c_w5s2": (1, 20, 13, 64, 32, W_, 5, 2),        # odd extent at stride 2
         "d_h5s2": (1, 13, 20, 64, 32, H_, 5, 2),
         "e_w7": (3, 4, 3, 40, 8, W_, 7, 1),             # extent 3 < k: padding on both sides of every output; K = 280
         "f_h7": (3, 3, 4, 40, 8, H_, 7, 1),
         "g_w9s2": (2, 8, 6, 136, 8, W_, 9, 2),          # even extent at stride 2, k = 9, more than 128 input channels
         "h_h9s2": (2, 6, 8, 8, 136, H_, 9, 2),          # ... more than 128 output channels
         "i_w1px": (1, 1, 1, 8, 8, W_, 3, 1),            # one pixel
         "j_h1px": (1, 1, 1, 8, 8, H_, 3, 1)}
PARAMS = [(t, d) for t in CASES for d in ("f32", "bf16")]
IDS = [f"{t}-{d}" for t, d in PARAMS]
# the wrap tests: the W cases whose last column is out of reach of column 0 in both directions, the H cases with more than one sample
WRAP = [(t, d) for t in ("a_w3", "c_w5s2", "b_h3", "f_h7", "h_h9s2") for d in ("f32", "bf16")]
_CACHE = {}


def _L():
    from yolo_dual_amd import _lib as L
    return L


def case(tag, dtype):
    """operands (host; exact in the compute dtype) and the float64 references, computed once"""
    key = (tag, dtype)
    if key in _CACHE:
        return _CACHE[key]
    L = _L()
    N, H, W, Cin, Cout, axis, k, s = CASES[tag]
    p = k // 2
    ks, ss, ps = ((1, k), (1, s), (0, p)) if axis == W_ else ((k, 1), (s, 1), (p, 0))
    Ho = (H + 2 * p - k) // s + 1 if axis == H_ else H
    Wo = (W + 2 * p - k) // s + 1 if axis == W_ else W
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(3000 + 31 * list(CASES).index(tag))
    x = (torch.randn(N, Cin, H, W, generator=g) + 0.25).to(tdt)
    K = k * Cin
    master = torch.randn(Cout, Cin, *ks, generator=g) / K ** 0.5
    dy = torch.randn(N, Cout, Ho, Wo, generator=g).to(tdt)
    dx0 = torch.randn(N, Cin, H, W, generator=g).to(tdt)
    dw0 = torch.randn(Cout, Cin, *ks, generator=g)
    xd, wd, dyd = x.double(), master.to(tdt).double(), dy.double()
    kw = dict(stride=ss, padding=ps)
    c = dict(N=N, H=H, W=W, Ho=Ho, Wo=Wo, Cin=Cin, Cout=Cout, axis=axis, k=k, s=s, p=p, ks=ks, ss=ss, ps=ps, K=K, Kd=k * Cout,
             npix=N * Ho * Wo, npix_in=N * H * W, tdt=tdt, es=2 if dtype == "bf16" else 4, dt=L.YDL_BF16 if dtype == "bf16" else L.YDL_F32,
             x=x, master=master, dy=dy, dx0=dx0, dw0=dw0,
             y=F.conv2d(xd, wd, **kw), y_abs=F.conv2d(xd.abs(), wd.abs(), **kw),
             dx=torch.nn.grad.conv2d_input(xd.shape, wd, dyd, **kw), dx_abs=torch.nn.grad.conv2d_input(xd.shape, wd.abs(), dyd.abs(), **kw),
             dw=torch.nn.grad.conv2d_weight(xd, wd.shape, dyd, **kw), dw_abs=torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, dyd.abs(), **kw))
    assert c["y"].shape == (N, Cout, Ho, Wo)
    _CACHE[key] = c
    return c


def store_eps(c):
    return 2.0 ** -8 if c["tdt"] == torch.bfloat16 else 0.0


def geom_of(c):
    L = _L()
    return L.ConvGeom(c["N"], c["H"], c["W"], c["Cin"], c["Ho"], c["Wo"], c["Cout"], c["k"], c["s"], c["p"], 2 * c["Cin"], 2 * c["Cout"], 0)


def weights(c):
    """-> (w, wt) compute-dtype device copies from ydl_weight_prep with kk = k, each followed by a sentinel guard that is checked; the
    KRSC master [Cout][k][Cin] is the channels_last storage of the (1, k) or (k, 1) weight"""
    L = _L()
    Cin, Cout, k = c["Cin"], c["Cout"], c["k"]
    n = Cout * k * Cin
    mk = c["master"].permute(0, 2, 3, 1).contiguous().view(Cout, k, Cin).cuda()
    w, wt = sentinel_like(n + 64, c["tdt"]), sentinel_like(n + 64, c["tdt"])
    L.call("ydl_weight_prep", c["dt"], _P(mk), _P(w), _P(wt), Cout, k, Cin, _st())
    torch.cuda.synchronize()
    sent = raw(sentinel_like(1, c["tdt"]))[0]
    assert bool((raw(w)[n:] == sent).all()) and bool((raw(wt)[n:] == sent).all()), "weight_prep wrote beyond its outputs"
    assert torch.equal(raw(w[:n].view(Cout, k, Cin)), raw(mk.to(c["tdt"]))), "w is not the master rounded to the compute dtype"
    return w, wt


def run_forward(c, w, stats=True, x=None):
    L = _L()
    lib = L.lib()
    Cin, Cout = c["Cin"], c["Cout"]
    geom = geom_of(c)
    gp = ctypes.byref(geom)
    xw = wide(c["x"] if x is None else x, c["tdt"], upper=True)
    yw = sentinel_like(c["npix"] * 2 * Cout, c["tdt"]).view(c["npix"], 2 * Cout)
    wsi, ws, q = _guarded_ws(lib.ydl_xconv_fwd_stats_ws_bytes(gp, c["axis"], c["dt"]))
    L.call("ydl_xconv_fwd", gp, c["axis"], c["dt"], half_ptr(xw, Cin, c["es"], True), _P(w), half_ptr(yw, Cout, c["es"], False),
           _P(ws) if stats else None, _st())
    torch.cuda.synchronize()
    return yw, (wsi, ws, q), gp, geom


def run_dgrad(c, wt, accumulate, dy=None):
    L = _L()
    Cin, Cout = c["Cin"], c["Cout"]
    geom = geom_of(c)
    dyw = wide(c["dy"] if dy is None else dy, c["tdt"], upper=True)
    dxw = wide(c["dx0"], c["tdt"], upper=False)
    L.call("ydl_xconv_dgrad", ctypes.byref(geom), c["axis"], c["dt"], half_ptr(dyw, Cout, c["es"], True), _P(wt),
           half_ptr(dxw, Cin, c["es"], False), accumulate, _st())
    torch.cuda.synchronize()
    return dxw


@pytest.mark.parametrize("tag,dtype", PARAMS, ids=IDS)
def test_forward_with_fused_statistics(tag, dtype):
    L = _L()
    lib = L.lib()
    c = case(tag, dtype)
    N, Ho, Wo, Cout, npix = c["N"], c["Ho"], c["Wo"], c["Cout"], c["npix"]
    w, _wt = weights(c)
    yw, (wsi, ws, q), gp, _geom = run_forward(c, w)
    sent = raw(sentinel_like(1, c["tdt"]))[0]
    assert bool((raw(yw)[:, Cout:] == sent).all()), "upper half of the wide output buffer written"
    got = to_nchw(yw[:, :Cout], N, Ho, Wo)
    assert bool(torch.isfinite(got).all()), "the kernel read outside its input slice (NaN sentinel) or left an output unwritten"
    bound = 2 * c["K"] * 2.0 ** -24 * c["y_abs"] + store_eps(c) * c["y"].abs()
    err = (got - c["y"]).abs()
    print(f"[xconv fwd {tag} {dtype}] max err/bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-30)).max())
    # the statistics rows: exactly ceil(npix / block_m) of them, nothing else of the guarded workspace changed
    bm = lib.ydl_xconv_fwd_block_m(gp, c["axis"], c["dt"])
    assert bm > 0
    nb = (npix + bm - 1) // bm
    assert q >= (nb + (nb + 63) // 64) * 2 * Cout
    assert bool((wsi[nb * 2 * Cout:] == SENT).all()) and _intact(wsi, q), "written beyond the statistics rows"
    assert not bool((wsi[:nb * 2 * Cout] == SENT).any()), "promised row not written"
    cb = _coef_buffers(Cout)
    gam, bet = torch.ones(Cout, device="cuda"), torch.zeros(Cout, device="cuda")
    L.call("ydl_bn_finalize", _P(ws), nb, bm, npix, Cout, _P(gam), _P(bet), EPS, MOM, _P(cb["rm"]), _P(cb["rv"]), _P(cb["mean"]),
           _P(cb["invstd"]), _P(cb["scale"]), _P(cb["shift"]), 1, _st())
    torch.cuda.synchronize()
    assert _intact(wsi, q), "finalize wrote beyond ydl_xconv_fwd_stats_ws_bytes"
    yr = yw[:, :Cout].double()
    mean = yr.mean(0)
    var = ((yr - mean) ** 2).mean(0)
    mean_tol, var_tol = BN_STATS_TOLS[0]
    if npix > 1:
        errs = _bn_errors(cb, dict(S=yr.sum(0), Q=(yr * yr).sum(0), mean=mean, var=var), torch.ones(Cout), torch.zeros(Cout), npix)
        print(f"[xconv stats {tag} {dtype}] mean {errs['mean']:.1e} var {errs['var']:.1e}")
        assert errs["mean"] < mean_tol and errs["var"] < var_tol, errs
    else:
        # one pixel: the variance is zero, so errors in units of sigma do not exist; the mean is the stored value itself (relative to
        # it) and the variance recovered from invstd is zero within the same relative bound of the eps it is added to
        assert bool(((cb["mean"].double() - mean).abs() <= mean_tol * mean.abs()).all())
        assert bool(((1.0 / cb["invstd"].double() ** 2 - EPS).abs() <= var_tol * EPS).all())
    # without a workspace: the same output
    yw2, _ws, _gp, _g = run_forward(c, w, stats=False)
    assert torch.equal(raw(yw), raw(yw2))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("tag,dtype", PARAMS, ids=IDS)
def test_input_gradient(tag, dtype, accumulate):
    c = case(tag, dtype)
    N, H, W, Cin = c["N"], c["H"], c["W"], c["Cin"]
    _w, wt = weights(c)
    dxw = run_dgrad(c, wt, accumulate)
    sent = raw(sentinel_like(1, c["tdt"]))[0]
    assert bool((raw(dxw)[:, Cin:] == sent).all()), "upper half of the wide gradient buffer written"
    got = to_nchw(dxw[:, :Cin], N, H, W)
    assert bool(torch.isfinite(got).all())
    want = c["dx"] + (c["dx0"].double() if accumulate else 0.0)
    mag = c["dx_abs"] + (c["dx0"].double().abs() if accumulate else 0.0)
    bound = 2 * (c["Kd"] + accumulate) * 2.0 ** -24 * mag + store_eps(c) * want.abs()
    err = (got - want).abs()
    print(f"[xconv dgrad {tag} {dtype} acc={accumulate}] max err/bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-30)).max())


@pytest.mark.parametrize("tag,dtype", PARAMS, ids=IDS)
def test_weight_gradient(tag, dtype):
    L = _L()
    c = case(tag, dtype)
    Cin, Cout, k = c["Cin"], c["Cout"], c["k"]
    geom = geom_of(c)
    gp = ctypes.byref(geom)
    xw, dyw = wide(c["x"], c["tdt"], upper=True), wide(c["dy"], c["tdt"], upper=True)
    xp, dyp = half_ptr(xw, Cin, c["es"], True), half_ptr(dyw, Cout, c["es"], True)
    ndw = Cout * k * Cin
    d0 = c["dw0"].permute(0, 2, 3, 1).contiguous().reshape(-1).cuda()         # KRSC, like dw
    runs = []
    for start in (None, None, d0):
        wsi, ws, q = _guarded_ws(L.lib().ydl_xconv_wgrad_ws_bytes(gp, c["axis"], c["dt"]))
        dwi = _sentinel(ndw + MIB)
        dwi[:ndw] = 0 if start is None else start.view(torch.int32)
        L.call("ydl_xconv_wgrad", gp, c["axis"], c["dt"], xp, dyp, _P(dwi), _P(ws), _st())
        torch.cuda.synchronize()
        assert _intact(wsi, q), "written beyond ydl_xconv_wgrad_ws_bytes"
        assert _intact(dwi, ndw), "written beyond dw"
        runs.append(dwi[:ndw].clone())
    assert torch.equal(runs[0], runs[1]), "two weight-gradient runs differ"

    def oihw(t):
        return t.view(torch.float32).double().cpu().view(Cout, *c["ks"], Cin).permute(0, 3, 1, 2)
    n = c["npix"]
    bound = 2 * n * 2.0 ** -24 * c["dw_abs"]
    err = (oihw(runs[0]) - c["dw"]).abs()
    print(f"[xconv wgrad {tag} {dtype}] max err/bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool(torch.isfinite(oihw(runs[0])).all())
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-30)).max())
    # the sum is ADDED into a non-zero dw (gradient accumulation): one more term, one more rounding
    want = c["dw"] + c["dw0"].double()
    bound2 = 2 * (n + 1) * 2.0 ** -24 * (c["dw_abs"] + c["dw0"].double().abs())
    err2 = (oihw(runs[2]) - want).abs()
    assert bool((err2 <= bound2).all()), float((err2 / bound2.clamp_min(1e-30)).max())


@pytest.mark.parametrize("tag,dtype", WRAP, ids=[f"{t}-{d}" for t, d in WRAP])
def test_a_tap_does_not_wrap_into_the_next_row_or_sample(tag, dtype):
    c = case(tag, dtype)
    N, H, W, Ho, Wo, Cin, Cout, p, s = c["N"], c["H"], c["W"], c["Ho"], c["Wo"], c["Cin"], c["Cout"], c["p"], c["s"]
    w, wt = weights(c)
    x, dy = torch.zeros_like(c["x"]), torch.zeros_like(c["dy"])
    if c["axis"] == W_:
        # column 0 of the output reads input columns -p..p; column 0 of dx reads dy columns <= p/s: the last column is out of reach
        assert W - 1 > p and Wo - 1 > p // s
        x[:, :, :, W - 1] = c["x"][:, :, :, W - 1]
        dy[:, :, :, Wo - 1] = c["dy"][:, :, :, Wo - 1]
        pick = lambda t: t[:, :, :, 0]
    else:
        assert N > 1
        x[0, :, H - 1, :] = c["x"][0, :, H - 1, :]
        dy[0, :, Ho - 1, :] = c["dy"][0, :, Ho - 1, :]
        pick = lambda t: t[1, :, 0, :]
    assert bool((x != 0).any()) and bool((dy != 0).any())
    yw, _ws, _gp, _g = run_forward(c, w, stats=False, x=x)
    y = raw(yw)[:, :Cout].reshape(N, Ho, Wo, Cout).permute(0, 3, 1, 2)
    assert bool((y != 0).any()), "the non-zero input reached nothing"
    assert bool((pick(y) == 0).all()), "forward: a tap wrapped"
    dxw = run_dgrad(c, wt, 0, dy=dy)
    dx = raw(dxw)[:, :Cin].reshape(N, H, W, Cin).permute(0, 3, 1, 2)
    assert bool((dx != 0).any()), "the non-zero gradient reached nothing"
    assert bool((pick(dx) == 0).all()), "input gradient: a tap wrapped"


def test_bad_arguments_are_refused():
    L = _L()
    x = torch.zeros(4096, device="cuda")
    # (Cin, Cout, k, s, p, axis, ldw): 12 channels; k = 4; k = 11; stride 3; p = 0; an unknown axis; a weight row stride
    for Cin, Cout, k, s, p, axis, ldw in ((12, 16, 3, 1, 1, 0, 0), (16, 16, 4, 1, 2, 0, 0), (16, 16, 11, 1, 5, 1, 0), (16, 16, 3, 3, 1, 1, 0),
                                          (16, 16, 3, 1, 0, 0, 0), (16, 16, 3, 1, 1, 2, 0), (16, 16, 3, 1, 1, 0, 64)):
        Lo = (4 + 2 * p - k) // s + 1
        geom = L.ConvGeom(1, 4, 4, Cin, Lo if axis == 1 else 4, 4 if axis == 1 else Lo, Cout, k, s, p, 16, 16, ldw)
        gp = ctypes.byref(geom)
        assert L.lib().ydl_xconv_supported(gp, axis, L.YDL_F32) == 0
        for rc in (L.lib().ydl_xconv_fwd(gp, axis, L.YDL_F32, _P(x), _P(x), _P(x), None, _st()),
                   L.lib().ydl_xconv_dgrad(gp, axis, L.YDL_F32, _P(x), _P(x), _P(x), 0, _st()),
                   L.lib().ydl_xconv_wgrad(gp, axis, L.YDL_F32, _P(x), _P(x), _P(x), _P(x), _st())):
            assert rc != 0 and L.lib().ydl_last_error()
    torch.cuda.synchronize()
