"""GPU: the squeeze-excitation kernels (csrc/se.hip) at their C ABI against the float64 formulas of tests/se_ref.py on the same rounded
operands, per element, f32 and bf16.

Every activation tensor is a channel slice in the UPPER half of a wider buffer (row stride 2 C + 8, first channel C + 8) whose other
channels and whose tail hold a NaN bit pattern no kernel produces; workspaces, saved rows and parameter-gradient rows have the same tail.
All of it must be intact afterwards.  The four parameters sit 4 bytes off a 16-byte boundary.  Shapes: (C, Cs) in {(8, 1), (24, 4),
(24, 6), (72, 8), (136, 28), (1152, 144)}, (N, HW) in {(1, 1), (2, 15), (1, 257), (3, 4099)}: 4099 pixels make 64 slices of 65 with a
ragged last one of 4; 1152 channels leave lanes of a CTA idle in bf16 (144 chunks) and take two chunk blocks in f32 (288).

Bounds are derived, not tuned, in the project's form  2 K 2^-24 S  (se_ref.bound) with S the kernel's expression on absolute values,
plus 2^-8 (1 + 2^-6) |ref| for a bf16 store.  Every stage is compared on the operands the kernel itself read -- its own stored pooled,
h, z, dz, dh -- so K is that stage's own chain:

pool        a lane adds its ceil(Lp / R) pixels in order (Lp pixels per slice, R = 256 / min(C / V, 256) pixel lanes), the CTA folds
            the R lanes in lane order: K = ceil(Lp / R) + R (+ 1 for the product of the dgate form), S = sum |x| (|x y|) of the
            slice.  Input: mean 100, std 1 -- the bound scales with sum |x|, so no cancellation hides in it.
pooled      the S slices in order and the division: K = S + 1, S = sum |part| / HW.
h           K = ceil(C / 64) + 7 (a lane's fused multiply-adds, six butterfly steps, the bias), S = |W1| |p| + |b1|.
z           K = Cs + 1 on S = |W2| |a| + |b2|, plus K_EXP = 4 on |W2| |a| for a = act(h) formed with expf.
gate        sigmoid: K_EXP on g; hardsigmoid: K = 3 on (|z| + 3) / 6.
dz          K = S - 1 + K_DEXP (6: expf and five operations) on sum_s |dgate_s| scale'(z): zero, hence equality, where a hardsigmoid
            is dead; at z = +-8 the sigmoid's derivative is 3.3e-4 and must carry full relative precision.
dh          K = ceil(C / 64) + 7 + K_DEXP on (|W2|^T |dz|) |act'(h)|: zero where a ReLU unit is dead.
dpooled     K = Cs on |W1|^T |dh|.
parameters  K = N + 1 (N products and additions in sample order, the addition into the destination; + K_EXP for dW2, which recomputes
            act(h)), S = the sum's absolute terms + |prior|.  Every sum runs twice into zeros with the same bits and once into twos.
scale_bwd   K = 4 (product, quotient, their sum, the prior), S = |dy| |g| + |dpooled| / HW + |prior|.

Where expf over- or underflows (a sigmoid or SiLU at |argument| > 87), f32 cannot hold the value to relative precision: those bounds
carry one more term, 2^-126 (the smallest normal f32) times the quantity the value multiplies.  A dead hardsigmoid or ReLU keeps a zero
bound; every other bound also carries K quanta of the subnormal range, 2^-149, since an f32 rounding below 2^-126 is absolute (a
saturated sigmoid's derivative times a gradient lands there).  The worst share of a bound is printed per kernel and dtype."""
import ctypes
import math

import pytest
import torch

from tests import se_ref as R
from tests.census import Floats, _P, _stream
from tests.test_gpu_convnext_kernels import Wide, _draw, _gen

pytestmark = pytest.mark.gpu

PAIRS = [(8, 1), (24, 4), (24, 6), (72, 8), (136, 28), (1152, 144)]
SHAPES = [(1, 1), (2, 15), (1, 257), (3, 4099)]
COMBOS = [("relu", "hardsigmoid"), ("silu", "sigmoid")]
WORST = {}


def _lib():
    from yolo_dual_amd import _lib as L
    return L


def _codes(L, act, gate):
    return (L.ACT_RELU if act == "relu" else L.ACT_SILU), (L.SE_GATE_HSIGMOID if gate == "hardsigmoid" else L.SE_GATE_SIGMOID)


def _note(kernel, dt, what, res):
    ratio, over = res
    key = (kernel, "bf16" if dt else "f32")
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert over == 0, (kernel, what, ratio, over)


def _nan(n):
    return Floats(n, "cuda", torch.full((n,), float("nan")))


class Off4:
    """n f32 values 4 bytes behind a 16-byte boundary, a sentinel guard behind them"""

    def __init__(self, data, init=None):
        self.n = data.numel() if init is None else data
        self.f = Floats(self.n + 1, "cuda", torch.zeros(self.n + 1))
        self.v = self.f.v[1:]
        self.v.copy_(data.flatten().float() if init is None else torch.full((self.n,), init))
        assert self.v.data_ptr() % 16 == 4

    @property
    def ptr(self):
        return ctypes.c_void_p(self.v.data_ptr())

    def check(self, what):
        self.f.check_guards(what)
        assert float(self.f.v[0]) == 0.0, what + ": written in front of the row"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [8, 24, 72, 136, 1152])
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_pool_partial_rows(dt, C, shape):
    N, hw = shape
    L = _lib()
    lib = L.lib()
    bf = dt == 1
    V = 8 if bf else 4
    gen = _gen(11, dt, C, N, hw)
    x = _draw(gen, (N * hw, C), bf, 1.0, 100.0)
    y = _draw(gen, (N * hw, C), bf)
    S = lib.ydl_se_pool_splits(N, hw)
    Lp = -(-hw // S)
    Rl = 256 // min(C // V, 256)
    K = -(-Lp // Rl) + Rl
    assert lib.ydl_se_pool_ws_bytes(N, hw, C) == N * S * C * 4
    if hw == 4099:
        assert (S, Lp, hw - (S - 1) * Lp) == (64, 65, 4)
    xb, yb = Wide(N * hw, C, dt, x), Wide(N * hw, C, dt, y)
    for dot in (False, True):
        ws = _nan(N * S * C)
        L.call("ydl_se_pool_fwd", dt, xb.ptr, xb.ld, yb.ptr if dot else None, yb.ld if dot else 0, _P(ws.raw), N, hw, C, _stream())
        torch.cuda.synchronize()
        ws.check_guards("ydl_se_pool_fwd: ws")
        xb.check("ydl_se_pool_fwd: x")
        yb.check("ydl_se_pool_fwd: y")
        got = ws.v.view(N, S, C).double().cpu()
        t = (x * y if dot else x).view(N, hw, C)
        pad = torch.zeros(N, S * Lp - hw, C, dtype=torch.float64)
        want = torch.cat([t, pad], 1).view(N, S, Lp, C).sum(2)
        Sabs = torch.cat([t.abs(), pad], 1).view(N, S, Lp, C).sum(2)
        _note("pool_dot" if dot else "pool", dt, "partial rows", R.compare(got, want, R.bound(K + (1 if dot else 0), Sabs)))
        ws2 = _nan(N * S * C)
        L.call("ydl_se_pool_fwd", dt, xb.ptr, xb.ld, yb.ptr if dot else None, yb.ld if dot else 0, _P(ws2.raw), N, hw, C, _stream())
        torch.cuda.synchronize()
        assert torch.equal(ws.raw, ws2.raw), "two runs differ"


def _excite_inputs(C, Cs, N, S, act, gate, seed):
    """partial rows, parameters and a gate gradient that reach every regime: the first eight channels have z = +-8 exactly (zero fc2
    rows, biases +-8), and with N > 1 sample 0's hidden units are all dead under ReLU (W1 >= 0, its pooled row negative)"""
    gen = _gen(12, C, Cs, N, S, seed)

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=torch.float64)
    part = (rn(N, S, C) + 1.0).abs()
    if N > 1:
        part[0] = -part[0]
    w1 = (rn(Cs, C).abs() * C ** -0.5).float().double()
    b1 = (rn(Cs) * 0.05).float().double()
    w2 = (rn(C, Cs) * 2.0 * Cs ** -0.5).float().double()
    b2 = (rn(C) * 2.0).float().double()
    w2[:8] = 0
    b2[:8] = torch.tensor([8.0, -8.0] * 4, dtype=torch.float64)
    dgate = rn(N, S, C).float().double()
    return part.float().double(), w1, b1, w2, b2, dgate


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_excite_forward_and_backward(combo, pair, shape):
    (act, gate), (C, Cs), (N, hw) = combo, pair, shape
    L = _lib()
    lib = L.lib()
    ac, gc = _codes(L, act, gate)
    S = lib.ydl_se_pool_splits(N, hw)
    part, w1, b1, w2, b2, dgate = _excite_inputs(C, Cs, N, S, act, gate, hw)
    P = [Off4(t) for t in (w1, b1, w2, b2)]
    pd = part.float().cuda()
    saved = {k: _nan(n) for k, n in (("pooled", N * C), ("h", N * Cs), ("z", N * C), ("gate", N * C))}
    L.call("ydl_se_excite_fwd", _P(pd), S, P[0].ptr, P[1].ptr, P[2].ptr, P[3].ptr, ac, gc, _P(saved["pooled"].raw), _P(saved["h"].raw),
           _P(saved["z"].raw), _P(saved["gate"].raw), N, hw, C, Cs, _stream())
    torch.cuda.synchronize()
    for k, f in saved.items():
        f.check_guards("ydl_se_excite_fwd: " + k)
    for p in P:
        p.check("ydl_se_excite_fwd: parameter")
    p_g, h_g = saved["pooled"].v.view(N, C).double().cpu(), saved["h"].v.view(N, Cs).double().cpu()
    z_g, g_g = saved["z"].v.view(N, C).double().cpu(), saved["gate"].v.view(N, C).double().cpu()
    _note("excite_fwd", 0, "pooled", R.compare(p_g, part.sum(1) / hw, R.bound(S + 1, part.abs().sum(1) / hw)))
    _note("excite_fwd", 0, "h", R.compare(h_g, p_g @ w1.T + b1, R.bound_h(p_g, w1, b1)))
    _note("excite_fwd", 0, "z", R.compare(z_g, R.act_fwd(h_g, act) @ w2.T + b2, R.bound_z(h_g, w2, b2, act)))
    _note("excite_fwd", 0, "gate", R.compare(g_g, R.gate_fwd(z_g, gate), R.bound_gate(z_g, gate)))
    assert torch.equal(z_g[:, :8], torch.tensor([8.0, -8.0] * 4, dtype=torch.float64).expand(N, 8))
    if gate == "hardsigmoid":
        assert torch.equal(g_g[:, :8], torch.tensor([1.0, 0.0] * 4, dtype=torch.float64).expand(N, 8))
    if act == "relu" and N > 1:
        assert bool((h_g[0] < 0).all()) and bool((h_g[1:] > 0).any())

    # backward: dz, dh (read back from the workspace) and dpooled, each from the kernel's own operands
    dd = dgate.float().cuda()
    nws = lib.ydl_se_excite_bwd_ws_bytes(N, C, Cs) // 4
    assert nws == N * (C + Cs)
    sizes = (Cs * C, Cs, C * Cs, C)

    def launch(init, skip=()):
        ws, dp = _nan(nws), _nan(N * C)
        grads = [None if i in skip else Off4(n, init) for i, n in enumerate(sizes)]
        L.call("ydl_se_excite_bwd", _P(dd), S, _P(saved["pooled"].raw), _P(saved["h"].raw), _P(saved["z"].raw), P[0].ptr, P[2].ptr, ac, gc,
               _P(dp.raw), *(g.ptr if g is not None else None for g in grads), _P(ws.raw), N, C, Cs, _stream())
        torch.cuda.synchronize()
        ws.check_guards("ydl_se_excite_bwd: ws")
        dp.check_guards("ydl_se_excite_bwd: dpooled")
        for g in grads:
            if g is not None:
                g.check("ydl_se_excite_bwd: parameter gradient")
        return ws, dp, grads
    ws, dp, g0 = launch(0.0)
    dz_g, dh_g = ws.v[:N * C].view(N, C).double().cpu(), ws.v[N * C:].view(N, Cs).double().cpu()
    dp_g = dp.v.view(N, C).double().cpu()
    _note("excite_bwd", 0, "dz", R.compare(dz_g, dgate.sum(1) * R.gate_grad(z_g, gate), R.bound_dz(dgate, z_g, gate)))
    _note("excite_bwd", 0, "dh", R.compare(dh_g, (dz_g @ w2) * R.act_grad(h_g, act), R.bound_dh(dz_g, h_g, w2, act)))
    _note("excite_bwd", 0, "dpooled", R.compare(dp_g, dh_g @ w1, R.bound_dpooled(dh_g, w1)))
    if gate == "hardsigmoid":
        assert bool((dz_g[:, :8] == 0).all())                  # beyond +-3: no gradient
    else:
        assert bool((dz_g[:, :8] != 0).all())                  # saturated at +-8: small, not lost
    if act == "relu" and N > 1:
        assert bool((dh_g[0] == 0).all()) and bool((dp_g[0] == 0).all())
    a_g = R.act_fwd(h_g, act)
    want = [dh_g.T @ p_g, dh_g.sum(0), dz_g.T @ a_g, dz_g.sum(0)]
    Sabs = [dh_g.abs().T @ p_g.abs(), dh_g.abs().sum(0), dz_g.abs().T @ a_g.abs(), dz_g.abs().sum(0)]
    under = [0.0, 0.0, R.TINY * (dz_g.abs().T @ h_g.abs()) if act == "silu" else 0.0, 0.0]
    extra = [0, 0, R.K_EXP, 0]
    _ws1, _dp1, g1 = launch(0.0)
    _ws2, _dp2, g2 = launch(2.0)
    for i, name in enumerate(("dw1", "db1", "dw2", "db2")):
        assert torch.equal(g0[i].f.raw, g1[i].f.raw), name + ": two runs differ"
        for g, prior in ((g0[i], 0.0), (g2[i], 2.0)):
            _note("excite_bwd", 0, name, R.compare(g.v.view(want[i].shape).double().cpu(), want[i] + prior,
                                                    R.bound_param(N, Sabs[i] + prior, extra[i]) + under[i]))
    # a frozen parameter: its pointer is NULL and the others come out the same
    _ws3, dp3, g3 = launch(0.0, skip=(0, 3))
    assert torch.equal(dp3.raw, dp.raw) and torch.equal(g3[1].f.raw, g0[1].f.raw) and torch.equal(g3[2].f.raw, g0[2].f.raw)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [8, 24, 72, 136, 1152])
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_scale_backward(dt, C, shape, accumulate):
    N, hw = shape
    L = _lib()
    bf = dt == 1
    gen = _gen(13, dt, C, N, hw, accumulate)
    dy = _draw(gen, (N * hw, C), bf)
    prior = _draw(gen, (N * hw, C), bf)
    g = torch.rand(N, C, generator=gen, dtype=torch.float64).float().double()
    dp = (torch.randn(N, C, generator=gen, dtype=torch.float64) * hw).float().double()       # dpooled / HW of the order of dy * g
    dyb, dxb = Wide(N * hw, C, dt, dy), Wide(N * hw, C, dt, prior)
    gd, dpd = g.float().cuda(), dp.float().cuda()
    L.call("ydl_se_scale_bwd", dt, dyb.ptr, dyb.ld, _P(gd), _P(dpd), dxb.ptr, dxb.ld, accumulate, N, hw, C, _stream())
    torch.cuda.synchronize()
    dyb.check("ydl_se_scale_bwd: dy")
    dxb.check("ydl_se_scale_bwd: dx")
    old = prior.view(N, hw, C) if accumulate else None
    want = R.scale_bwd(dy.view(N, hw, C), g, dp) + (old if accumulate else 0)
    tol = R.bound_scale_bwd(dy.view(N, hw, C), g, dp, old, bf)
    _note("scale_bwd", dt, f"acc={accumulate}", R.compare(dxb.logical().view(N, hw, C), want, tol))


def test_bad_arguments_are_refused_without_a_launch():
    L = _lib()
    lib = L.lib()
    x = torch.zeros(64, 16, device="cuda")
    f = torch.zeros(4096, device="cuda")
    st = _stream()
    bad = [("ydl_se_pool_fwd", (0, _P(x), 16, None, 0, _P(f), 2, 32, 12, st)),                     # C not a multiple of 8
           ("ydl_se_pool_fwd", (0, _P(x), 8, None, 0, _P(f), 2, 32, 16, st)),                      # stride below C
           ("ydl_se_pool_fwd", (0, ctypes.c_void_p(x.data_ptr() + 4), 16, None, 0, _P(f), 2, 32, 16, st)),    # misaligned x
           ("ydl_se_pool_fwd", (0, _P(x), 16, None, 0, None, 2, 32, 16, st)),                      # no workspace
           ("ydl_se_excite_fwd", (_P(f), 1, _P(f), _P(f), _P(f), _P(f), 0, 0, _P(f), _P(f), _P(f), _P(f), 2, 32, 16, 4, st)),    # act NONE
           ("ydl_se_excite_fwd", (_P(f), 1, _P(f), _P(f), _P(f), _P(f), 2, 2, _P(f), _P(f), _P(f), _P(f), 2, 32, 16, 4, st)),    # gate code
           ("ydl_se_excite_fwd", (_P(f), 1, _P(f), _P(f), _P(f), _P(f), 2, 1, _P(f), _P(f), _P(f), _P(f), 2, 32, 16, 513, st)),  # Cs
           ("ydl_se_excite_fwd", (_P(f), 65, _P(f), _P(f), _P(f), _P(f), 2, 1, _P(f), _P(f), _P(f), _P(f), 2, 32, 16, 4, st)),   # S
           ("ydl_se_excite_bwd", (_P(f), 1, _P(f), _P(f), _P(f), _P(f), _P(f), 1, 0, None, None, None, None, None, _P(f), 2, 16, 4, st)),
           ("ydl_se_scale_bwd", (1, _P(x), 16, _P(f), _P(f), _P(x), 12, 0, 2, 32, 16, st)),        # bf16 stride not whole chunks
           ("ydl_se_scale_bwd", (0, _P(x), 16, _P(f), None, _P(x), 16, 0, 2, 32, 16, st))]         # no dpooled
    for name, args in bad:
        assert getattr(lib, name)(*args) != 0, (name, args)
        assert name in lib.ydl_last_error().decode()
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0 and float(f.abs().sum()) == 0.0


def test_zz_print_the_worst_shares():
    for (kernel, dt), v in sorted(WORST.items()):
        print(f"[se kernels] {kernel:12s} {dt:5s} worst share of its bound {v:.3f}")
    assert all(math.isfinite(v) and v <= 1.0 for v in WORST.values())
