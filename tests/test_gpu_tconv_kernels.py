"""GPU: the transposed convolutions at the C ABI against float64 ``F.conv_transpose2d`` (forward), ``F.conv2d`` (input gradient) and
``torch.nn.grad.conv2d_weight`` (weight gradient) on the CPU, on the same rounded operands.  Scheme and helpers of
tests/test_gpu_xconv_kernels.py / tests/test_gpu_gconv_kernels.py.

Dense: ``nn.ConvTranspose2d(c1, c2, k, 2, p, op)`` has no kernel of its own.  It is ydl_conv_dgrad / ydl_conv_fwd / ydl_conv_wgrad_det
with the roles of x and dy exchanged on the mirrored geometry {N, 2H, 2W, Cin = c2, H, W, Cout = c1, k, 2, p} (include/ydl.h).  These
cases drive entry points that exist on the parent commit and may pass there: what they pin is that the mirrored recipe computes a
transposed convolution at (k, p, op) in {(2,0,0), (4,1,0), (3,1,1)}, two of which no model ran before.  The weight is the one the
kernels read: the channels_last parameter [c1][c2][k][k] = KRSC master [c1][k*k][c2], rounded to the compute dtype by ydl_weight_prep.

Depth-wise: ydl_dwtconv_fwd / _dgrad / _wgrad of csrc/tconv.hip (new symbols), which read the f32 master [C][k*k] directly.

Bounds are derived, not tuned: twice K * 2^-24 * S, S the same operation on absolute values, plus 2^-8 |ref| for each bf16 store.
  dense forward        K = ceil(k/2)^2 * c1: the taps of one output-parity class (+1 with the bias, which is a second pass over the
                       stored output: ydl_bn_act_fwd in place with scale 1, so in bf16 a second store rounding, 2^-8 |conv|, is added)
  dense dx             K = k^2 * c2 (+1 accumulate)
  depth-wise forward   K = ceil(k/2)^2 + 1 (the fused bias)
  depth-wise dgrad     K = k^2 (+1 accumulate)
  weight gradients     K = n = N*H*W terms (+1 when added into a non-zero dw)

Operands are read from the upper half of twice-wide NaN-sentinel buffers and answers written into the lower half: the other half and
the guards behind dw and the workspace keep the sentinel.  Weight-gradient runs are bitwise equal; dw and dx accumulate.  Wrap tests,
bit for bit: x non-zero only in the last column gives an output column 0 of zeros; x non-zero only in the last row of sample 0 gives a
zero row 0 of sample 1; the same for the input gradient with dy non-zero in the last output column / row."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_bn_statistics import _guarded_ws, _intact, _sentinel
from tests.test_gpu_gconv_kernels import MIB, _P, _st, half_ptr, raw, sentinel_like, to_nchw, wide

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FORMS = {2: (0, 0), 4: (1, 0), 3: (1, 1)}            # k -> (padding, output_padding)
# (N, H, W, c1, c2, k)
DENSE = [(2, 9, 7, 16, 24, 2), (2, 9, 7, 16, 24, 3), (2, 9, 7, 16, 24, 4), (1, 5, 3, 136, 8, 4), (1, 3, 5, 8, 136, 2), (3, 1, 1, 8, 8, 4),
         (2, 4, 3, 40, 24, 3)]
# (N, H, W, C, k)
DW = [(2, 9, 7, 24, 2), (2, 9, 7, 24, 3), (2, 9, 7, 24, 4), (1, 1, 1, 8, 4), (3, 4, 3, 40, 3), (1, 5, 6, 136, 4)]
DTYPES = ("f32", "bf16")
_CACHE = {}


def _L():
    from yolo_dual_amd import _lib as L
    return L


def _ids(cases):
    return ["x".join(str(v) for v in c) for c in cases]


def _common(dtype):
    L = _L()
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    return dict(tdt=tdt, es=2 if dtype == "bf16" else 4, dt=L.YDL_BF16 if dtype == "bf16" else L.YDL_F32, eps=2.0 ** -8 if dtype == "bf16" else 0.0)


def dense_case(cfg, dtype):
    key = ("dense", cfg, dtype)
    if key in _CACHE:
        return _CACHE[key]
    N, H, W, c1, c2, k = cfg
    p, op = FORMS[k]
    c = _common(dtype)
    tdt = c["tdt"]
    g = torch.Generator().manual_seed(5000 + 31 * DENSE.index(cfg))
    hk = (k + 1) // 2
    x = (torch.randn(N, c1, H, W, generator=g) + 0.25).to(tdt)
    master = torch.randn(c1, c2, k, k, generator=g) / (hk * hk * c1) ** 0.5
    bias = torch.randn(c2, generator=g)
    dy = torch.randn(N, c2, 2 * H, 2 * W, generator=g).to(tdt)
    dx0 = torch.randn(N, c1, H, W, generator=g).to(tdt)
    dw0 = torch.randn(c1, c2, k, k, generator=g)
    xd, wd, dyd = x.double(), master.to(tdt).double(), dy.double()
    tk = dict(stride=2, padding=p, output_padding=op)
    ck = dict(stride=2, padding=p)
    c.update(N=N, H=H, W=W, c1=c1, c2=c2, k=k, p=p, op=op, x=x, master=master, bias=bias, dy=dy, dx0=dx0, dw0=dw0,
             y=F.conv_transpose2d(xd, wd, **tk), y_abs=F.conv_transpose2d(xd.abs(), wd.abs(), **tk),
             dx=F.conv2d(dyd, wd, **ck), dx_abs=F.conv2d(dyd.abs(), wd.abs(), **ck),
             dw=torch.nn.grad.conv2d_weight(dyd, wd.shape, xd, **ck), dw_abs=torch.nn.grad.conv2d_weight(dyd.abs(), wd.shape, xd.abs(), **ck))
    assert c["y"].shape == (N, c2, 2 * H, 2 * W) and c["dx"].shape == x.shape
    _CACHE[key] = c
    return c


def dense_geom(c):
    """the mirrored convolution c2 -> c1 on the (2H, 2W) map; both tensors live in twice-wide buffers"""
    return _L().ConvGeom(c["N"], 2 * c["H"], 2 * c["W"], c["c2"], c["H"], c["W"], c["c1"], c["k"], 2, c["p"], 2 * c["c2"], 2 * c["c1"], 0)


def dense_weights(c):
    L = _L()
    c1, c2, kk = c["c1"], c["c2"], c["k"] * c["k"]
    n = c1 * kk * c2
    mk = c["master"].permute(0, 2, 3, 1).contiguous().view(c1, kk, c2).cuda()        # channels_last storage of [c1][c2][k][k]
    w, wt = sentinel_like(n + 64, c["tdt"]), sentinel_like(n + 64, c["tdt"])
    L.call("ydl_weight_prep", c["dt"], _P(mk), _P(w), _P(wt), c1, kk, c2, _st())
    torch.cuda.synchronize()
    sent = raw(sentinel_like(1, c["tdt"]))[0]
    assert bool((raw(w)[n:] == sent).all()) and bool((raw(wt)[n:] == sent).all()), "weight_prep wrote beyond its outputs"
    return w, wt


def _check(what, got, want, bound):
    err = (got - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"[{what}] max err/bound {ratio:.3f}")
    assert bool(torch.isfinite(got).all()), f"{what}: read outside its input slice (NaN sentinel) or left an element unwritten"
    assert bool((err <= bound).all()), (what, ratio)


def _upper_intact(buf, C, tdt):
    return bool((raw(buf)[:, C:] == raw(sentinel_like(1, tdt))[0]).all())


def dense_forward(c, wt, x=None, bias=False):
    L = _L()
    geom = dense_geom(c)
    c1, c2 = c["c1"], c["c2"]
    npo = c["N"] * 4 * c["H"] * c["W"]
    xw = wide(c["x"] if x is None else x, c["tdt"], upper=True)
    yw = sentinel_like(npo * 2 * c2, c["tdt"]).view(npo, 2 * c2)
    L.call("ydl_conv_dgrad", ctypes.byref(geom), c["dt"], half_ptr(xw, c1, c["es"], True), _P(wt), half_ptr(yw, c2, c["es"], False), 0, _st())
    if bias:
        ones, b = torch.ones(c2, device="cuda"), c["bias"].cuda()
        L.call("ydl_bn_act_fwd", c["dt"], _P(yw), 2 * c2, _P(ones), _P(b), None, 0, L.RES_NONE, L.ACT_NONE, _P(yw), 2 * c2, npo, c2, _st())
    torch.cuda.synchronize()
    return yw


def dense_dgrad(c, w, accumulate, dy=None):
    L = _L()
    geom = dense_geom(c)
    c1, c2 = c["c1"], c["c2"]
    dyw = wide(c["dy"] if dy is None else dy, c["tdt"], upper=True)
    dxw = wide(c["dx0"], c["tdt"], upper=False)
    L.call("ydl_conv_fwd", ctypes.byref(geom), c["dt"], half_ptr(dyw, c2, c["es"], True), _P(w), half_ptr(dxw, c1, c["es"], False), None,
           accumulate, _st())
    torch.cuda.synchronize()
    return dxw


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", DENSE, ids=_ids(DENSE))
def test_dense_forward_is_the_mirrored_dgrad(cfg, dtype, bias):
    c = dense_case(cfg, dtype)
    N, H, W, c1, c2, k = cfg
    _w, wt = dense_weights(c)
    yw = dense_forward(c, wt, bias=bias)
    assert _upper_intact(yw, c2, c["tdt"]), "upper half of the wide output buffer written"
    got = to_nchw(yw[:, :c2], N, 2 * H, 2 * W)
    K = ((k + 1) // 2) ** 2 * c1
    b = c["bias"].double().view(1, c2, 1, 1) if bias else 0.0
    want = c["y"] + b
    mag = c["y_abs"] + (b.abs() if bias else 0.0)
    bound = 2 * (K + int(bias)) * U * mag + c["eps"] * want.abs() + (c["eps"] * c["y"].abs() if bias else 0.0)
    _check(f"tconv fwd {cfg} {dtype} bias={bias}", got, want, bound)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", DENSE, ids=_ids(DENSE))
def test_dense_input_gradient_is_the_mirrored_forward(cfg, dtype, accumulate):
    c = dense_case(cfg, dtype)
    N, H, W, c1, c2, k = cfg
    w, _wt = dense_weights(c)
    dxw = dense_dgrad(c, w, accumulate)
    assert _upper_intact(dxw, c1, c["tdt"]), "upper half of the wide gradient buffer written"
    got = to_nchw(dxw[:, :c1], N, H, W)
    want = c["dx"] + (c["dx0"].double() if accumulate else 0.0)
    mag = c["dx_abs"] + (c["dx0"].double().abs() if accumulate else 0.0)
    _check(f"tconv dx {cfg} {dtype} acc={accumulate}", got, want, 2 * (k * k * c2 + accumulate) * U * mag + c["eps"] * want.abs())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", DENSE, ids=_ids(DENSE))
def test_dense_weight_gradient_is_the_mirrored_wgrad(cfg, dtype):
    L = _L()
    c = dense_case(cfg, dtype)
    N, H, W, c1, c2, k = cfg
    geom = dense_geom(c)
    gp = ctypes.byref(geom)
    dyw, xw = wide(c["dy"], c["tdt"], upper=True), wide(c["x"], c["tdt"], upper=True)
    ndw = c1 * k * k * c2
    d0 = c["dw0"].permute(0, 2, 3, 1).contiguous().reshape(-1).cuda()
    runs = []
    for start in (None, None, d0):
        wsi, ws, q = _guarded_ws(max(L.lib().ydl_conv_wgrad_ws_bytes(gp, c["dt"]), 16))
        dwi = _sentinel(ndw + MIB)
        dwi[:ndw] = 0 if start is None else start.view(torch.int32)
        L.call("ydl_conv_wgrad_det", gp, c["dt"], half_ptr(dyw, c2, c["es"], True), half_ptr(xw, c1, c["es"], True), _P(dwi), _P(ws), _st())
        torch.cuda.synchronize()
        assert _intact(wsi, q), "written beyond ydl_conv_wgrad_ws_bytes"
        assert _intact(dwi, ndw), "written beyond dw"
        runs.append(dwi[:ndw].clone())
    assert torch.equal(runs[0], runs[1]), "two weight-gradient runs differ"

    def iohw(t):
        return t.view(torch.float32).double().cpu().view(c1, k, k, c2).permute(0, 3, 1, 2)
    n = N * H * W
    _check(f"tconv dW {cfg} {dtype}", iohw(runs[0]), c["dw"], 2 * n * U * c["dw_abs"])
    _check(f"tconv dW+ {cfg} {dtype}", iohw(runs[2]), c["dw"] + c["dw0"].double(), 2 * (n + 1) * U * (c["dw_abs"] + c["dw0"].double().abs()))


# ---------------------------------------------------------------------------------------------------------------------------
# depth-wise
# ---------------------------------------------------------------------------------------------------------------------------
def dw_case(cfg, dtype):
    key = ("dw", cfg, dtype)
    if key in _CACHE:
        return _CACHE[key]
    N, H, W, C, k = cfg
    p, op = FORMS[k]
    c = _common(dtype)
    tdt = c["tdt"]
    g = torch.Generator().manual_seed(6000 + 31 * DW.index(cfg))
    x = (torch.randn(N, C, H, W, generator=g) + 0.25).to(tdt)
    master = torch.randn(C, 1, k, k, generator=g) / ((k + 1) // 2)          # read by the kernels in f32, as it is
    bias = torch.randn(C, generator=g)
    dy = torch.randn(N, C, 2 * H, 2 * W, generator=g).to(tdt)
    dx0 = torch.randn(N, C, H, W, generator=g).to(tdt)
    dw0 = torch.randn(C, 1, k, k, generator=g)
    xd, wd, dyd, bd = x.double(), master.double(), dy.double(), bias.double()
    tk = dict(stride=2, padding=p, output_padding=op, groups=C)
    ck = dict(stride=2, padding=p, groups=C)
    c.update(N=N, H=H, W=W, C=C, k=k, p=p, op=op, x=x, master=master, bias=bias, dy=dy, dx0=dx0, dw0=dw0,
             y=F.conv_transpose2d(xd, wd, bd, **tk), y_abs=F.conv_transpose2d(xd.abs(), wd.abs(), bd.abs(), **tk),
             y_nb=F.conv_transpose2d(xd, wd, None, **tk),
             dx=F.conv2d(dyd, wd, **ck), dx_abs=F.conv2d(dyd.abs(), wd.abs(), **ck),
             dw=torch.nn.grad.conv2d_weight(dyd, wd.shape, xd, **ck), dw_abs=torch.nn.grad.conv2d_weight(dyd.abs(), wd.shape, xd.abs(), **ck))
    _CACHE[key] = c
    return c


def dw_forward(c, x=None, bias=True):
    L = _L()
    N, H, W, C, k = c["N"], c["H"], c["W"], c["C"], c["k"]
    npo = N * 4 * H * W
    xw = wide(c["x"] if x is None else x, c["tdt"], upper=True)
    yw = sentinel_like(npo * 2 * C, c["tdt"]).view(npo, 2 * C)
    wm, b = c["master"].view(C, k * k).contiguous().cuda(), c["bias"].cuda()
    L.call("ydl_dwtconv_fwd", c["dt"], half_ptr(xw, C, c["es"], True), 2 * C, _P(wm), _P(b) if bias else None, half_ptr(yw, C, c["es"], False),
           2 * C, N, H, W, C, k, c["p"], c["op"], _st())
    torch.cuda.synchronize()
    return yw


def dw_dgrad(c, accumulate, dy=None):
    L = _L()
    N, H, W, C, k = c["N"], c["H"], c["W"], c["C"], c["k"]
    dyw = wide(c["dy"] if dy is None else dy, c["tdt"], upper=True)
    dxw = wide(c["dx0"], c["tdt"], upper=False)
    wm = c["master"].view(C, k * k).contiguous().cuda()
    L.call("ydl_dwtconv_dgrad", c["dt"], half_ptr(dyw, C, c["es"], True), 2 * C, _P(wm), half_ptr(dxw, C, c["es"], False), 2 * C, accumulate,
           N, H, W, C, k, c["p"], c["op"], _st())
    torch.cuda.synchronize()
    return dxw


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", DW, ids=_ids(DW))
def test_depthwise_forward_with_fused_bias(cfg, dtype):
    c = dw_case(cfg, dtype)
    N, H, W, C, k = cfg
    K = ((k + 1) // 2) ** 2 + 1
    yw = dw_forward(c)
    assert _upper_intact(yw, C, c["tdt"]), "upper half of the wide output buffer written"
    _check(f"dwtconv fwd {cfg} {dtype}", to_nchw(yw[:, :C], N, 2 * H, 2 * W), c["y"], 2 * K * U * c["y_abs"] + c["eps"] * c["y"].abs())
    yw = dw_forward(c, bias=False)
    _check(f"dwtconv fwd nobias {cfg} {dtype}", to_nchw(yw[:, :C], N, 2 * H, 2 * W), c["y_nb"], 2 * K * U * c["y_abs"] + c["eps"] * c["y_nb"].abs())


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", DW, ids=_ids(DW))
def test_depthwise_input_gradient(cfg, dtype, accumulate):
    c = dw_case(cfg, dtype)
    N, H, W, C, k = cfg
    dxw = dw_dgrad(c, accumulate)
    assert _upper_intact(dxw, C, c["tdt"]), "upper half of the wide gradient buffer written"
    want = c["dx"] + (c["dx0"].double() if accumulate else 0.0)
    mag = c["dx_abs"] + (c["dx0"].double().abs() if accumulate else 0.0)
    _check(f"dwtconv dgrad {cfg} {dtype} acc={accumulate}", to_nchw(dxw[:, :C], N, H, W), want,
           2 * (k * k + accumulate) * U * mag + c["eps"] * want.abs())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", DW, ids=_ids(DW))
def test_depthwise_weight_gradient(cfg, dtype):
    L = _L()
    c = dw_case(cfg, dtype)
    N, H, W, C, k = cfg
    xw, dyw = wide(c["x"], c["tdt"], upper=True), wide(c["dy"], c["tdt"], upper=True)
    ndw = C * k * k
    d0 = c["dw0"].reshape(-1).contiguous().cuda()
    runs = []
    for start in (None, None, d0):
        wsi, ws, q = _guarded_ws(L.lib().ydl_dwtconv_wgrad_ws_bytes(C, k))
        dwi = _sentinel(ndw + MIB)
        dwi[:ndw] = 0 if start is None else start.view(torch.int32)
        L.call("ydl_dwtconv_wgrad", c["dt"], half_ptr(xw, C, c["es"], True), 2 * C, half_ptr(dyw, C, c["es"], True), 2 * C, _P(dwi), _P(ws),
               N, H, W, C, k, c["p"], c["op"], _st())
        torch.cuda.synchronize()
        assert _intact(wsi, q), "written beyond ydl_dwtconv_wgrad_ws_bytes"
        assert _intact(dwi, ndw), "written beyond dw"
        runs.append(dwi[:ndw].clone())
    assert torch.equal(runs[0], runs[1]), "two weight-gradient runs differ"

    def shaped(t):
        return t.view(torch.float32).double().cpu().view(C, 1, k, k)
    n = N * H * W
    _check(f"dwtconv dW {cfg} {dtype}", shaped(runs[0]), c["dw"], 2 * n * U * c["dw_abs"])
    _check(f"dwtconv dW+ {cfg} {dtype}", shaped(runs[2]), c["dw"] + c["dw0"].double(), 2 * (n + 1) * U * (c["dw_abs"] + c["dw0"].double().abs()))


# ---------------------------------------------------------------------------------------------------------------------------
# wrap tests
# ---------------------------------------------------------------------------------------------------------------------------
def _wrap(c, C_in, C_out, fwd, dgrad):
    N, H, W = c["N"], c["H"], c["W"]
    assert N > 1 and W > 2
    for axis in ("w", "h"):
        x, dy = torch.zeros_like(c["x"]), torch.zeros_like(c["dy"])
        if axis == "w":
            x[:, :, :, W - 1] = c["x"][:, :, :, W - 1]
            dy[:, :, :, 2 * W - 1] = c["dy"][:, :, :, 2 * W - 1]
            pick = lambda t: t[:, :, :, 0]
        else:
            x[0, :, H - 1, :] = c["x"][0, :, H - 1, :]
            dy[0, :, 2 * H - 1, :] = c["dy"][0, :, 2 * H - 1, :]
            pick = lambda t: t[1, :, 0, :]
        y = raw(fwd(x))[:, :C_out].reshape(N, 2 * H, 2 * W, C_out).permute(0, 3, 1, 2)
        assert bool((y != 0).any()), "the non-zero input reached nothing"
        assert bool((pick(y) == 0).all()), f"forward: a tap wrapped ({axis})"
        dx = raw(dgrad(dy))[:, :C_in].reshape(N, H, W, C_in).permute(0, 3, 1, 2)
        assert bool((dx != 0).any()), "the non-zero gradient reached nothing"
        assert bool((pick(dx) == 0).all()), f"input gradient: a tap wrapped ({axis})"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", DENSE[:3], ids=_ids(DENSE[:3]))
def test_dense_tap_does_not_wrap_into_the_next_row_or_sample(cfg, dtype):
    c = dense_case(cfg, dtype)
    w, wt = dense_weights(c)
    _wrap(c, c["c1"], c["c2"], lambda x: dense_forward(c, wt, x=x), lambda dy: dense_dgrad(c, w, 0, dy=dy))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", DW[:3], ids=_ids(DW[:3]))
def test_depthwise_tap_does_not_wrap_into_the_next_row_or_sample(cfg, dtype):
    c = dw_case(cfg, dtype)
    _wrap(c, c["C"], c["C"], lambda x: dw_forward(c, x=x, bias=False), lambda dy: dw_dgrad(c, 0, dy=dy))


def test_supported_answers_on_the_host_and_bad_arguments_are_refused():
    L = _L()
    lib = L.lib()
    for k, (p, op) in FORMS.items():
        assert lib.ydl_dwtconv_supported(16, k, 2, p, op) == 1
    # (C, k, s, p, op): 12 channels; stride 1; stride 3; k = 1; k = 5; the wrong padding; the wrong output padding
    for C, k, s, p, op in ((12, 4, 2, 1, 0), (16, 4, 1, 1, 0), (16, 4, 3, 1, 0), (16, 1, 2, 0, 0), (16, 5, 2, 2, 1), (16, 4, 2, 0, 0), (16, 3, 2, 1, 0)):
        assert lib.ydl_dwtconv_supported(C, k, s, p, op) == 0
    x = torch.zeros(4096, device="cuda")
    for C, k, p, op in ((12, 4, 1, 0), (16, 5, 2, 1), (16, 4, 0, 0), (16, 3, 1, 0)):
        for rc in (lib.ydl_dwtconv_fwd(L.YDL_F32, _P(x), 16, _P(x), None, _P(x), 16, 1, 2, 2, C, k, p, op, _st()),
                   lib.ydl_dwtconv_dgrad(L.YDL_F32, _P(x), 16, _P(x), _P(x), 16, 0, 1, 2, 2, C, k, p, op, _st()),
                   lib.ydl_dwtconv_wgrad(L.YDL_F32, _P(x), 16, _P(x), 16, _P(x), _P(x), 1, 2, 2, C, k, p, op, _st())):
            assert rc != 0 and lib.ydl_last_error()
    torch.cuda.synchronize()
