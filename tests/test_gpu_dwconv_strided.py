"""GPU: the strided depth-wise kernels (ydl_dwconv2_fwd / _dgrad / _wgrad) through the C ABI against float64
``F.conv2d(groups=C)``, ``torch.nn.grad.conv2d_input`` and ``conv2d_weight`` on the same operands (x and dy rounded to the compute
dtype first; w is the f32 master weight the kernels read).

Bounds are derived, not tuned.  Every output is a chain of at most k*k fmaf (one rounding each, of a partial sum no larger than
S = sum |w x| over the taps), so |err| <= k*k * 2^-24 * S; the bound used is twice that, plus 2^-8 |y| for the one bf16 rounding of
the store.  With ``accumulate`` the previous value joins the sum (one more rounding).  A weight gradient adds n = N*Ho*Wo products:
2 * n * 2^-24 * sum |dy x|.

Bitwise: at s = 1 the output and the input gradient equal ydl_dwconv_fwd / ydl_dwconv_dgrad; the fused statistics rows equal
ydl_bn_stats of the stored output and nothing else of the guarded workspace changes; two weight-gradient runs are equal.  The forward
writes into the upper half of a buffer twice as wide: the lower half and the padding channels keep their sentinel."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_bn_statistics import BN_STATS_TOLS, EPS, MOM, SENT, _bn_errors, _coef_buffers, _guarded_ws, _intact, _sentinel

pytestmark = pytest.mark.gpu

# tag -> (N, H, W, C, k, s)
CASES = {"a_odd": (2, 7, 5, 8, 3, 2), "b_c20": (2, 6, 8, 20, 5, 2), "c_40px": (1, 15, 9, 8, 3, 2), "d_128px": (2, 16, 16, 16, 5, 2),
         "e_s1_363px": (3, 11, 11, 12, 5, 1), "f_k7": (1, 5, 5, 8, 7, 2)}
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


def _ru(a, b):
    return (a + b - 1) // b * b


def case(tag, dtype):
    """operands (host; x, dy, dx0 exact in the compute dtype) and the float64 references, computed once"""
    key = (tag, dtype)
    if key in _CACHE:
        return _CACHE[key]
    N, H, W, C, k, s = CASES[tag]
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(1000 + 17 * list(CASES).index(tag))
    x = (torch.randn(N, C, H, W, generator=g) + 0.25).to(tdt)
    w = torch.randn(C, 1, k, k, generator=g) / k
    dy = torch.randn(N, C, Ho, Wo, generator=g).to(tdt)
    dx0 = torch.randn(N, C, H, W, generator=g).to(tdt)
    xd, wd, dyd = x.double(), w.double(), dy.double()
    c = dict(N=N, H=H, W=W, C=C, k=k, s=s, p=p, Ho=Ho, Wo=Wo, tdt=tdt, es=2 if dtype == "bf16" else 4, ld=_ru(C, 8),
             x=x, w=w, dy=dy, dx0=dx0,
             y=F.conv2d(xd, wd, stride=s, padding=p, groups=C), y_abs=F.conv2d(xd.abs(), wd.abs(), stride=s, padding=p, groups=C),
             dx=torch.nn.grad.conv2d_input(xd.shape, wd, dyd, stride=s, padding=p, groups=C),
             dx_abs=torch.nn.grad.conv2d_input(xd.shape, wd.abs(), dyd.abs(), stride=s, padding=p, groups=C),
             dw=torch.nn.grad.conv2d_weight(xd, wd.shape, dyd, stride=s, padding=p, groups=C),
             dw_abs=torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, dyd.abs(), stride=s, padding=p, groups=C))
    L = _L()
    c["dt"] = L.YDL_BF16 if dtype == "bf16" else L.YDL_F32
    _CACHE[key] = c
    return c


def nhwc(t, ld, tdt, fill=3.0):
    """(N,C,H,W) host tensor -> device [N*H*W][ld] of the compute dtype; the padding channels hold ``fill`` (they must not matter)"""
    N, C, H, W = t.shape
    buf = torch.full((N, H, W, ld), fill, dtype=tdt)
    buf[..., :C] = t.permute(0, 2, 3, 1)
    return buf.reshape(N * H * W, ld).cuda()


def to_nchw(buf, N, H, W, C):
    return buf.reshape(N, H, W, buf.shape[-1])[..., :C].permute(0, 3, 1, 2).double().cpu()


def sentinel_like(n, tdt):
    if tdt == torch.bfloat16:
        return torch.full((n,), 0x7FA5, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return _sentinel(n).view(torch.float32)


def raw(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def store_eps(c):
    return 2.0 ** -8 if c["tdt"] == torch.bfloat16 else 0.0


def run_forward(c, stats=True):
    """-> (y as (N,C,Ho,Wo) view of the wide buffer's upper half, the wide buffer, guarded statistics workspace)"""
    L = _L()
    ld, C = c["ld"], c["C"]
    npix = c["N"] * c["Ho"] * c["Wo"]
    xg = nhwc(c["x"], ld, c["tdt"])
    wide = sentinel_like(npix * 2 * ld, c["tdt"]).view(npix, 2 * ld)
    wg = c["w"].reshape(C, -1).contiguous().cuda()
    wsi, ws, q = _guarded_ws(L.lib().ydl_bn_stats_ws_bytes(npix, C))
    yptr = ctypes.c_void_p(wide.data_ptr() + ld * c["es"])
    L.call("ydl_dwconv2_fwd", c["dt"], _P(xg), ld, _P(wg), yptr, 2 * ld, _P(ws) if stats else None, c["N"], c["H"], c["W"], C,
           c["k"], c["s"], _st())
    torch.cuda.synchronize()
    return wide, yptr, (wsi, ws, q), xg, wg


@pytest.mark.parametrize("tag,dtype", PARAMS, ids=IDS)
def test_forward_with_fused_statistics(tag, dtype):
    L = _L()
    lib = L.lib()
    c = case(tag, dtype)
    ld, C, N, Ho, Wo, k = c["ld"], c["C"], c["N"], c["Ho"], c["Wo"], c["k"]
    npix = N * Ho * Wo
    wide, yptr, (wsi, ws, q), xg, wg = run_forward(c)
    sent = raw(sentinel_like(1, c["tdt"]))[0]
    r = raw(wide)
    assert bool((r[:, :ld] == sent).all()), "lower half of the wide buffer written"
    assert bool((r[:, ld + C:] == sent).all()), "padding channels written"
    got = to_nchw(wide[:, ld:], N, Ho, Wo, C)
    bound = 2 * k * k * 2.0 ** -24 * c["y_abs"] + store_eps(c) * c["y"].abs()
    err = (got - c["y"]).abs()
    print(f"[dw fwd {tag} {dtype}] max err/bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-30)).max())
    # the rows equal ydl_bn_stats of the stored tensor, and nothing else of the workspace changed
    bm = lib.ydl_bn_stats_block_m()
    nb, cp = (npix + bm - 1) // bm, _ru(C, 8)
    wsi2, ws2, q2 = _guarded_ws(lib.ydl_bn_stats_ws_bytes(npix, C))
    L.call("ydl_bn_stats", c["dt"], yptr, 2 * ld, _P(ws2), npix, C, _st())
    torch.cuda.synchronize()
    assert torch.equal(wsi, wsi2), "fused statistics rows differ from ydl_bn_stats of the stored output"
    assert bool((wsi[nb * 2 * cp:] == SENT).all()) and _intact(wsi, q)
    assert not bool((wsi[:nb * 2 * cp].view(nb, 2, cp)[:, :, :C] == SENT).any()), "promised row not written"
    # through ydl_bn_finalize: mean and variance of the stored output
    cb = _coef_buffers(C)
    gam, bet = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    L.call("ydl_bn_finalize", _P(ws), nb, bm, npix, C, _P(gam), _P(bet), EPS, MOM, _P(cb["rm"]), _P(cb["rv"]), _P(cb["mean"]),
           _P(cb["invstd"]), _P(cb["scale"]), _P(cb["shift"]), 1, _st())
    torch.cuda.synchronize()
    assert _intact(wsi, q), "finalize wrote beyond ydl_bn_stats_ws_bytes"
    yr = wide[:, ld:ld + C].double()
    mean = yr.mean(0)
    var = ((yr - mean) ** 2).mean(0)
    errs = _bn_errors(cb, dict(S=yr.sum(0), Q=(yr * yr).sum(0), mean=mean, var=var), torch.ones(C), torch.zeros(C), npix)
    print(f"[dw stats {tag} {dtype}] mean {errs['mean']:.1e} var {errs['var']:.1e}")
    mean_tol, var_tol = BN_STATS_TOLS[0]
    assert errs["mean"] < mean_tol and errs["var"] < var_tol, errs
    # without a workspace: the same output
    wide2, _y, _w, _x, _wg = run_forward(c, stats=False)
    assert torch.equal(raw(wide), raw(wide2))
    if c["s"] == 1:
        yref = sentinel_like(npix * ld, c["tdt"]).view(npix, ld)
        L.call("ydl_dwconv_fwd", c["dt"], _P(xg), ld, _P(wg), _P(yref), ld, N, c["H"], c["W"], C, k, c["p"], _st())
        torch.cuda.synchronize()
        assert torch.equal(raw(wide[:, ld:ld + C]), raw(yref[:, :C])), "s = 1 output differs from ydl_dwconv_fwd"


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("tag,dtype", PARAMS, ids=IDS)
def test_input_gradient(tag, dtype, accumulate):
    L = _L()
    c = case(tag, dtype)
    ld, C, N, H, W, k = c["ld"], c["C"], c["N"], c["H"], c["W"], c["k"]
    dyg = nhwc(c["dy"], ld, c["tdt"])
    wg = c["w"].reshape(C, -1).contiguous().cuda()
    dx = nhwc(c["dx0"], ld, c["tdt"], fill=0.0)
    L.call("ydl_dwconv2_dgrad", c["dt"], _P(dyg), ld, _P(wg), _P(dx), ld, accumulate, N, H, W, C, k, c["s"], _st())
    torch.cuda.synchronize()
    got = to_nchw(dx, N, H, W, C)
    want = c["dx"] + (c["dx0"].double() if accumulate else 0.0)
    mag = c["dx_abs"] + (c["dx0"].double().abs() if accumulate else 0.0)
    bound = 2 * k * k * 2.0 ** -24 * mag + store_eps(c) * want.abs()
    err = (got - want).abs()
    print(f"[dw dgrad {tag} {dtype} acc={accumulate}] max err/bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-30)).max())
    if c["s"] == 1:
        ref = nhwc(c["dx0"], ld, c["tdt"], fill=0.0)
        L.call("ydl_dwconv_dgrad", c["dt"], _P(dyg), ld, _P(wg), _P(ref), ld, accumulate, N, H, W, C, k, c["p"], _st())
        torch.cuda.synchronize()
        assert torch.equal(raw(dx[:, :C]), raw(ref[:, :C])), "s = 1 input gradient differs from ydl_dwconv_dgrad"


@pytest.mark.parametrize("tag,dtype", PARAMS, ids=IDS)
def test_weight_gradient(tag, dtype):
    L = _L()
    c = case(tag, dtype)
    ld, C, N, H, W, k = c["ld"], c["C"], c["N"], c["H"], c["W"], c["k"]
    xg, dyg = nhwc(c["x"], ld, c["tdt"]), nhwc(c["dy"], ld, c["tdt"])
    ndw = C * k * k
    runs = []
    for _ in range(2):
        wsi, ws, q = _guarded_ws(L.lib().ydl_dwconv2_wgrad_ws_bytes(C, k))
        dwi = _sentinel(ndw + MIB)
        dwi[:ndw] = 0
        L.call("ydl_dwconv2_wgrad", c["dt"], _P(xg), ld, _P(dyg), ld, _P(dwi), _P(ws), N, H, W, C, k, c["s"], _st())
        torch.cuda.synchronize()
        assert _intact(wsi, q), "written beyond ydl_dwconv2_wgrad_ws_bytes"
        assert _intact(dwi, ndw), "written beyond dw"
        runs.append(dwi[:ndw].clone())
    assert torch.equal(runs[0], runs[1]), "two weight-gradient runs differ"
    got = runs[0].view(torch.float32).double().cpu().view(C, 1, k, k)
    n = N * c["Ho"] * c["Wo"]
    bound = 2 * n * 2.0 ** -24 * c["dw_abs"]
    err = (got - c["dw"]).abs()
    print(f"[dw wgrad {tag} {dtype}] max err/bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-30)).max())


def test_bad_arguments_are_refused():
    L = _L()
    x = torch.zeros(64, device="cuda")
    for k, s, ld in ((4, 1, 8), (3, 3, 8), (3, 2, 4)):
        rc = L.lib().ydl_dwconv2_fwd(L.YDL_F32, _P(x), ld, _P(x), _P(x), ld, None, 1, 2, 2, 8, k, s, _st())
        assert rc != 0 and L.lib().ydl_last_error()
