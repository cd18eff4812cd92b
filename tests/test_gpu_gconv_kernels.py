"""GPU: the grouped-convolution kernels (ydl_gconv_weight_prep / _fwd / _dgrad / _wgrad) through the C ABI against float64
``F.conv2d(groups=g)``, ``torch.nn.grad.conv2d_input`` and ``conv2d_weight`` on the CPU, on the same operands: x, dy and dx0 rounded to
the compute dtype first, and the weight the kernels read — in bf16 the copy ydl_gconv_weight_prep wrote, which is checked separately
(it equals the master rounded to bf16, and wt is its per-group transpose, bit for bit).

Bounds are derived, not tuned.  An output is a sum of K = k*k*C/g products accumulated in f32 (one rounding per product of a partial
sum no larger than S, the same convolution of absolute values), so |err| <= K * 2^-24 * S; the bound used is twice that, plus
2^-8 |ref| for the bf16 rounding of the store.  With ``accumulate`` the previous value joins the sum: one more term and one more
rounding.  A weight gradient sums n = N*H*W products: 2 * n * 2^-24 * S.

x is read from the upper half and y is written into the lower half of buffers twice as wide that are filled with a NaN sentinel: the
other half keeps it (and a kernel that read it would spread NaNs), as does the guarded statistics workspace beyond its rows.  The
rows, finalised by ydl_bn_finalize, are the float64 mean / variance of the STORED output at BN_STATS_TOLS[0] of
tests/test_gpu_bn_statistics.py.  Two weight-gradient runs are bitwise equal, and one group's input does not reach another group's
output bits."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_bn_statistics import BN_STATS_TOLS, EPS, MOM, SENT, _bn_errors, _coef_buffers, _guarded_ws, _intact, _sentinel

pytestmark = pytest.mark.gpu

# tag -> (N, H, W, Cin, Cout, g, k)
CASES = {"a_16_16": (2, 9, 7, 64, 64, 4, 3),          # 16 / 16 per group, 126 pixels, two samples
         "b_cv5": (2, 6, 5, 256, 64, 4, 1),           # 64 -> 16: the cv5 shape
         "c_16_48": (1, 20, 13, 32, 96, 2, 3),        # 16 -> 48, more than one pixel tile
         "d_48_w3": (3, 4, 3, 96, 32, 2, 3),          # 48 per group: K = 432 is no multiple of a bf16 MFMA K step; W = 3
         "e_1px": (1, 1, 1, 32, 32, 2, 3),            # every tap but the centre is padding
         "f_g8": (2, 17, 16, 128, 128, 8, 1)}         # g = 8
PARAMS = [(t, d) for t in CASES for d in ("f32", "bf16")]
IDS = [f"{t}-{d}" for t, d in PARAMS]
MIB = (1 << 20) // 4
_CACHE = {}


def _L():
    from yolo_dual_amd import _lib as L
    return L


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def case(tag, dtype):
    """operands (host; exact in the compute dtype) and the float64 references, computed once"""
    key = (tag, dtype)
    if key in _CACHE:
        return _CACHE[key]
    L = _L()
    N, H, W, Cin, Cout, G, k = CASES[tag]
    p = k // 2
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(2000 + 31 * list(CASES).index(tag))
    x = (torch.randn(N, Cin, H, W, generator=g) + 0.25).to(tdt)
    K = k * k * (Cin // G)
    master = torch.randn(Cout, Cin // G, k, k, generator=g) / K ** 0.5
    dy = torch.randn(N, Cout, H, W, generator=g).to(tdt)
    dx0 = torch.randn(N, Cin, H, W, generator=g).to(tdt)
    dw0 = torch.randn(Cout, Cin // G, k, k, generator=g)
    xd, wd, dyd = x.double(), master.to(tdt).double(), dy.double()
    c = dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, G=G, k=k, p=p, K=K, Kd=k * k * (Cout // G), npix=N * H * W, tdt=tdt,
             es=2 if dtype == "bf16" else 4, dt=L.YDL_BF16 if dtype == "bf16" else L.YDL_F32,
             x=x, master=master, dy=dy, dx0=dx0, dw0=dw0,
             y=F.conv2d(xd, wd, padding=p, groups=G), y_abs=F.conv2d(xd.abs(), wd.abs(), padding=p, groups=G),
             dx=torch.nn.grad.conv2d_input(xd.shape, wd, dyd, padding=p, groups=G),
             dx_abs=torch.nn.grad.conv2d_input(xd.shape, wd.abs(), dyd.abs(), padding=p, groups=G),
             dw=torch.nn.grad.conv2d_weight(xd, wd.shape, dyd, padding=p, groups=G),
             dw_abs=torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, dyd.abs(), padding=p, groups=G))
    _CACHE[key] = c
    return c


def sentinel_like(n, tdt):
    if tdt == torch.bfloat16:
        return torch.full((n,), 0x7FA5, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return _sentinel(n).view(torch.float32)


def raw(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def wide(t, tdt, upper):
    """(N,C,H,W) host tensor -> device [N*H*W][2C] of the compute dtype, t in the upper or the lower half, the sentinel in the other"""
    N, C, H, W = t.shape
    buf = sentinel_like(N * H * W * 2 * C, tdt).view(N * H * W, 2 * C)
    (buf[:, C:] if upper else buf[:, :C]).copy_(t.permute(0, 2, 3, 1).reshape(N * H * W, C).to(tdt).cuda())
    return buf


def half_ptr(buf, C, es, upper):
    return ctypes.c_void_p(buf.data_ptr() + (C * es if upper else 0))


def to_nchw(mat, N, H, W):
    return mat.reshape(N, H, W, mat.shape[-1]).permute(0, 3, 1, 2).double().cpu()


def store_eps(c):
    return 2.0 ** -8 if c["tdt"] == torch.bfloat16 else 0.0


def geom_of(c):
    L = _L()
    return L.ConvGeom(c["N"], c["H"], c["W"], c["Cin"], c["H"], c["W"], c["Cout"], c["k"], 1, c["p"], 2 * c["Cin"], 2 * c["Cout"], 0)


def weights(c):
    """-> (w, wt) compute-dtype device copies from ydl_gconv_weight_prep, each followed by a sentinel guard that is checked"""
    L = _L()
    Cin, Cout, G, k = c["Cin"], c["Cout"], c["G"], c["k"]
    n = Cout * k * k * (Cin // G)
    mk = c["master"].permute(0, 2, 3, 1).contiguous().cuda()               # KRSC [Cout][k*k][Cin/g]
    w, wt = sentinel_like(n + 64, c["tdt"]), sentinel_like(n + 64, c["tdt"])
    L.call("ydl_gconv_weight_prep", c["dt"], _P(mk), _P(w), _P(wt), Cout, k * k, Cin, G, _st())
    torch.cuda.synchronize()
    sent = raw(sentinel_like(1, c["tdt"]))[0]
    assert bool((raw(w)[n:] == sent).all()) and bool((raw(wt)[n:] == sent).all()), "weight_prep wrote beyond its outputs"
    return w, wt, mk


@pytest.mark.parametrize("tag,dtype", PARAMS, ids=IDS)
def test_weight_prep_rounds_and_transposes_per_group(tag, dtype):
    c = case(tag, dtype)
    Cin, Cout, G, kk = c["Cin"], c["Cout"], c["G"], c["k"] * c["k"]
    Cig, Cog = Cin // G, Cout // G
    w, wt, mk = weights(c)
    n = Cout * kk * Cig
    want = mk.to(c["tdt"])                                                   # round to nearest even, as the kernel's conversion
    assert torch.equal(raw(w[:n].view(Cout, kk, Cig)), raw(want.view(Cout, kk, Cig))), "w is not the master rounded to the compute dtype"
    want_t = want.view(G, Cog, kk, Cig).permute(0, 3, 2, 1).reshape(Cin, kk, Cog).contiguous()
    assert torch.equal(raw(wt[:n].view(Cin, kk, Cog)), raw(want_t)), "wt is not the per-group transpose of w"


def run_forward(c, w, stats=True, x=None):
    L = _L()
    lib = L.lib()
    Cin, Cout, G = c["Cin"], c["Cout"], c["G"]
    geom = geom_of(c)
    gp = ctypes.byref(geom)
    xw = wide(c["x"] if x is None else x, c["tdt"], upper=True)
    yw = sentinel_like(c["npix"] * 2 * Cout, c["tdt"]).view(c["npix"], 2 * Cout)
    wsi, ws, q = _guarded_ws(lib.ydl_gconv_fwd_stats_ws_bytes(gp, G, c["dt"]))
    L.call("ydl_gconv_fwd", gp, G, c["dt"], half_ptr(xw, Cin, c["es"], True), _P(w), half_ptr(yw, Cout, c["es"], False),
           _P(ws) if stats else None, _st())
    torch.cuda.synchronize()
    return yw, (wsi, ws, q), gp, geom


@pytest.mark.parametrize("tag,dtype", PARAMS, ids=IDS)
def test_forward_with_fused_statistics(tag, dtype):
    L = _L()
    lib = L.lib()
    c = case(tag, dtype)
    N, H, W, Cout, G, npix = c["N"], c["H"], c["W"], c["Cout"], c["G"], c["npix"]
    w, _wt, _mk = weights(c)
    yw, (wsi, ws, q), gp, _geom = run_forward(c, w)
    sent = raw(sentinel_like(1, c["tdt"]))[0]
    assert bool((raw(yw)[:, Cout:] == sent).all()), "upper half of the wide output buffer written"
    got = to_nchw(yw[:, :Cout], N, H, W)
    assert bool(torch.isfinite(got).all()), "the kernel read outside its input slice (NaN sentinel) or left an output unwritten"
    bound = 2 * c["K"] * 2.0 ** -24 * c["y_abs"] + store_eps(c) * c["y"].abs()
    err = (got - c["y"]).abs()
    print(f"[gconv fwd {tag} {dtype}] max err/bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-30)).max())
    # the statistics rows: exactly ceil(npix / block_m) of them, nothing else of the guarded workspace changed
    bm = lib.ydl_gconv_fwd_block_m(gp, G, c["dt"])
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
    assert _intact(wsi, q), "finalize wrote beyond ydl_gconv_fwd_stats_ws_bytes"
    yr = yw[:, :Cout].double()
    mean = yr.mean(0)
    var = ((yr - mean) ** 2).mean(0)
    mean_tol, var_tol = BN_STATS_TOLS[0]
    if npix > 1:
        errs = _bn_errors(cb, dict(S=yr.sum(0), Q=(yr * yr).sum(0), mean=mean, var=var), torch.ones(Cout), torch.zeros(Cout), npix)
        print(f"[gconv stats {tag} {dtype}] mean {errs['mean']:.1e} var {errs['var']:.1e}")
        assert errs["mean"] < mean_tol and errs["var"] < var_tol, errs
    else:
        # one pixel: the variance is zero, so errors in units of sigma do not exist; the mean is the stored value itself (relative to
        # it) and the variance recovered from invstd is zero within the same relative bound of the eps it is added to
        assert bool(((cb["mean"].double() - mean).abs() <= mean_tol * mean.abs()).all())
        assert bool(((1.0 / cb["invstd"].double() ** 2 - EPS).abs() <= var_tol * EPS).all())
    # without a workspace: the same output
    yw2, _ws, _gp, _g = run_forward(c, w, stats=False)
    assert torch.equal(raw(yw), raw(yw2))


@pytest.mark.parametrize("tag,dtype", PARAMS, ids=IDS)
def test_one_groups_input_does_not_reach_another_groups_output(tag, dtype):
    c = case(tag, dtype)
    Cin, Cout, G = c["Cin"], c["Cout"], c["G"]
    Cig, Cog = Cin // G, Cout // G
    w, _wt, _mk = weights(c)
    yw, _ws, _gp, _g = run_forward(c, w, stats=False)
    x2 = c["x"].clone()
    x2[:, Cig:2 * Cig] = (x2[:, Cig:2 * Cig].float() * -1.5 + 1.0).to(c["tdt"])          # group 1 of the input
    yw2, _ws, _gp, _g = run_forward(c, w, stats=False, x=x2)
    a, b = raw(yw)[:, :Cout], raw(yw2)[:, :Cout]
    assert torch.equal(a[:, :Cog], b[:, :Cog]) and torch.equal(a[:, 2 * Cog:], b[:, 2 * Cog:]), "another group's output changed"
    assert not torch.equal(a[:, Cog:2 * Cog], b[:, Cog:2 * Cog]), "the group's own output did not change"


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("tag,dtype", PARAMS, ids=IDS)
def test_input_gradient(tag, dtype, accumulate):
    L = _L()
    c = case(tag, dtype)
    N, H, W, Cin, Cout, G = c["N"], c["H"], c["W"], c["Cin"], c["Cout"], c["G"]
    _w, wt, _mk = weights(c)
    geom = geom_of(c)
    dyw = wide(c["dy"], c["tdt"], upper=True)
    dxw = wide(c["dx0"], c["tdt"], upper=False)
    L.call("ydl_gconv_dgrad", ctypes.byref(geom), G, c["dt"], half_ptr(dyw, Cout, c["es"], True), _P(wt), half_ptr(dxw, Cin, c["es"], False),
           accumulate, _st())
    torch.cuda.synchronize()
    sent = raw(sentinel_like(1, c["tdt"]))[0]
    assert bool((raw(dxw)[:, Cin:] == sent).all()), "upper half of the wide gradient buffer written"
    got = to_nchw(dxw[:, :Cin], N, H, W)
    assert bool(torch.isfinite(got).all())
    want = c["dx"] + (c["dx0"].double() if accumulate else 0.0)
    mag = c["dx_abs"] + (c["dx0"].double().abs() if accumulate else 0.0)
    bound = 2 * (c["Kd"] + accumulate) * 2.0 ** -24 * mag + store_eps(c) * want.abs()
    err = (got - want).abs()
    print(f"[gconv dgrad {tag} {dtype} acc={accumulate}] max err/bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-30)).max())


@pytest.mark.parametrize("tag,dtype", PARAMS, ids=IDS)
def test_weight_gradient(tag, dtype):
    L = _L()
    c = case(tag, dtype)
    N, H, W, Cin, Cout, G, k = c["N"], c["H"], c["W"], c["Cin"], c["Cout"], c["G"], c["k"]
    geom = geom_of(c)
    gp = ctypes.byref(geom)
    xw, dyw = wide(c["x"], c["tdt"], upper=True), wide(c["dy"], c["tdt"], upper=True)
    xp, dyp = half_ptr(xw, Cin, c["es"], True), half_ptr(dyw, Cout, c["es"], True)
    ndw = Cout * k * k * (Cin // G)
    d0 = c["dw0"].permute(0, 2, 3, 1).contiguous().reshape(-1).cuda()         # KRSC, like dw
    runs = []
    for start in (None, None, d0):
        wsi, ws, q = _guarded_ws(L.lib().ydl_gconv_wgrad_ws_bytes(gp, G, c["dt"]))
        dwi = _sentinel(ndw + MIB)
        dwi[:ndw] = 0 if start is None else start.view(torch.int32)
        L.call("ydl_gconv_wgrad", gp, G, c["dt"], xp, dyp, _P(dwi), _P(ws), _st())
        torch.cuda.synchronize()
        assert _intact(wsi, q), "written beyond ydl_gconv_wgrad_ws_bytes"
        assert _intact(dwi, ndw), "written beyond dw"
        runs.append(dwi[:ndw].clone())
    assert torch.equal(runs[0], runs[1]), "two weight-gradient runs differ"

    def oihw(t):
        return t.view(torch.float32).double().cpu().view(Cout, k, k, Cin // G).permute(0, 3, 1, 2)
    n = N * H * W
    bound = 2 * n * 2.0 ** -24 * c["dw_abs"]
    err = (oihw(runs[0]) - c["dw"]).abs()
    print(f"[gconv wgrad {tag} {dtype}] max err/bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool(torch.isfinite(oihw(runs[0])).all())
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-30)).max())
    # the sum is ADDED into a non-zero dw (gradient accumulation): one more term, one more rounding
    want = c["dw"] + c["dw0"].double()
    bound2 = 2 * (n + 1) * 2.0 ** -24 * (c["dw_abs"] + c["dw0"].double().abs())
    err2 = (oihw(runs[2]) - want).abs()
    assert bool((err2 <= bound2).all()), float((err2 / bound2.clamp_min(1e-30)).max())


def test_bad_arguments_are_refused():
    L = _L()
    x = torch.zeros(4096, device="cuda")
    # (Cin, Cout, k, s, p, groups, ldw): 12 per group; k = 5; stride 2; groups = 1; a weight row stride
    for Cin, Cout, k, s, p, G, ldw in ((24, 24, 3, 1, 1, 2, 0), (32, 32, 5, 1, 2, 2, 0), (32, 32, 3, 2, 1, 2, 0), (32, 32, 3, 1, 1, 1, 0),
                                       (32, 32, 1, 1, 0, 2, 64)):
        Ho = (4 + 2 * p - k) // s + 1
        geom = L.ConvGeom(1, 4, 4, Cin, Ho, Ho, Cout, k, s, p, Cin, Cout, ldw)
        gp = ctypes.byref(geom)
        assert L.lib().ydl_gconv_supported(gp, G, L.YDL_F32) == 0
        for rc in (L.lib().ydl_gconv_fwd(gp, G, L.YDL_F32, _P(x), _P(x), _P(x), None, _st()),
                   L.lib().ydl_gconv_dgrad(gp, G, L.YDL_F32, _P(x), _P(x), _P(x), 0, _st()),
                   L.lib().ydl_gconv_wgrad(gp, G, L.YDL_F32, _P(x), _P(x), _P(x), _P(x), _st())):
            assert rc != 0 and L.lib().ydl_last_error()
    torch.cuda.synchronize()
