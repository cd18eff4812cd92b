"""GPU: the ConvNeXt kernels (csrc/convnext.hip) at their C ABI against the float64 formulas of tests/convnext_ref.py on the same
rounded operands, per element, f32 and bf16.

Every tensor is a channel slice in the UPPER half of a wider buffer (row stride 2 C + 8, first channel C + 8) whose other channels and
whose tail hold a NaN bit pattern no kernel produces; workspaces and parameter-gradient rows have the same tail.  All of it must be
intact afterwards.  Shapes: C in {8, 24, 136, 768} (1024 too for LayerNorm), npix in {1, 30 (N = 2, 3 x 5), 257}.

Bounds are derived, not tuned, in the project's form  2 K 2^-24 S  with S the kernel's expression on absolute values, plus
2^-8 (1 + 2^-6) |ref| for a bf16 store.  U = 2^-24 below; "chain" is the longest run of f32 additions a sum goes through.

LayerNorm forward, K = chain + 6 with chain = V ceil(C / 16 V) + 4 (a lane's chunks, then the four row steps):
    the sums carry chain roundings, so d = u - mu is off by K U A with A = max_c |u| + mean_c |u|; the variance, a mean of d^2, by
    2 sqrt(var) K U A, which moves r by r^2 K U A; hence  S = r |gamma| A (1 + |xh|) + |beta|.  With mean 100 and std 1 the bound is
    about 200 K U: the cancellation in u - mu is in S, and a one-pass variance (E u^2 - mu^2, error 10^4 K U) is far outside it.
    Stored mu: S = mean |u|; stored r: S = r (1 + r A).
LayerNorm backward, K = chain + 8, from the stored statistics as operands:
    E = r (max_c |u| + |mu|) bounds xh's own error per unit U; S = r (|g| + mean |g| + |xh| mean |g xh| + E (|m2| + |xh| mean |g|)).
    dgamma: S = sum_p |dy| (|xh| + E), dbeta: S = sum_p |dy|, with K = 20 (one pixel per lane here, sixteen rows folded in f32, then
    double); dpre_bias: the sum of dx's own bounds plus 2 * 20 U sum_p |dx|.
GELU, K = 8 (u, the argument, erff and expf to a few ulps, 1 + erf, two products):
    forward S = |u| (1 + |erf|) / 2 + 1.13 (|z| + |b|): the rounding of u meets |GELU'| <= 1.13;
    backward S = |dy| ((1 + |erf|) / 2 + |u| pdf (1 + u^2 / 2) + 0.8 (|z| + |b|)): expf's argument error is relative to u^2 / 2 and
    |(cdf + u pdf)'| = pdf |2 - u^2| <= 0.8.  dbias: the sum of dz's bounds plus 2 K_acc U sum_p |dz|, K_acc = 258: up to 256 pixel
    lanes of a CTA are folded in f32 in lane order, then double.
Layer-scaled residual, K = 3: S = |x| + |keep gamma y|;  dy: K = 2, S = |ref|;  dgamma: K_acc as above, S = sum |keep dout y|;
    dx = dout exactly (one more rounding when it accumulates).  A sample with keep = 0 gets x bit for bit.

Every parameter-gradient sum runs twice into zeros with the same bits and once more into a row of twos.  The worst share of a bound
is printed per kernel and dtype."""
import math

import pytest
import torch

from tests import convnext_ref as R
from tests.census import SENT, TAIL, Floats, _P, _stream, _tdt

pytestmark = pytest.mark.gpu

CS = [8, 24, 136, 768]
NPIX = {1: (1, 1), 30: (2, 15), 257: (1, 257)}          # npix -> (N, hw)
U, ST = R.U24, R.BF16_STORE
K_ACC = 258


def _lib():
    from yolo_dual_amd import _lib as L
    return L


class Wide:
    """[npix, C] values of the storage type in channels [C + 8, 2 C + 8) of rows of 2 C + 8 elements; everything else, and TAIL
    elements behind the last row, holds a NaN sentinel.  ``data`` None: an output, sentinel everywhere."""

    def __init__(self, npix, C, dt, data=None):
        self.npix, self.C, self.ld, self.c0, self.tdt = npix, C, 2 * C + 8, C + 8, _tdt(dt)
        self.it = torch.int16 if dt else torch.int32
        self.pat = 0x7FA5 if dt else SENT
        self.flat = torch.empty(npix * self.ld + TAIL, dtype=self.tdt, device="cuda")
        self.flat.view(self.it).fill_(self.pat)
        self.v = self.flat[:npix * self.ld].view(npix, self.ld)
        if data is not None:
            self.v[:, self.c0:self.c0 + C] = data.to(self.tdt).cuda()

    @property
    def ptr(self):
        import ctypes
        return ctypes.c_void_p(self.flat.data_ptr() + self.c0 * self.flat.element_size())

    def logical(self):
        return self.v[:, self.c0:self.c0 + self.C].double().cpu()

    def bits(self):
        return self.v[:, self.c0:self.c0 + self.C].contiguous().view(self.it).cpu()

    def check(self, what):
        g = self.flat.view(self.it)
        rows = g[:self.npix * self.ld].view(self.npix, self.ld)
        assert bool((g[self.npix * self.ld:] == self.pat).all()), what + ": written behind the last row"
        assert bool((rows[:, :self.c0] == self.pat).all()) and bool((rows[:, self.c0 + self.C:] == self.pat).all()), \
            what + ": written outside its channels"


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (1 << 31))


def _draw(gen, shape, bf16, scale=1.0, offset=0.0):
    return R.rnd(torch.randn(*shape, generator=gen, dtype=torch.float64) * scale + offset, bf16)


def _vec(gen, C, lo, hi):
    return (torch.rand(C, generator=gen, dtype=torch.float64) * (hi - lo) + lo).float().double()


def _ws(nbytes):
    return Floats(max(nbytes // 4, 4), "cuda", torch.full((max(nbytes // 4, 4),), float("nan")))


WORST = {}


def _note(kernel, dt, what, res):
    ratio, over = res
    key = (kernel, "bf16" if dt else "f32")
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert over == 0, (kernel, what, ratio, over)
    return ratio


def _sum_runs(launch, C, what):
    """``launch(rows)`` adds the parameter-gradient sums into ``rows`` (a list of Floats): twice into zeros with the same bits, once
    into twos -> (the sums, the sums + 2)"""
    runs = []
    for init in (0.0, 0.0, 2.0):
        rows = launch(lambda: Floats(C, "cuda", torch.full((C,), init)))
        torch.cuda.synchronize()
        for r in rows:
            if r is not None:
                r.check_guards(what + ": parameter gradient")
        runs.append(rows)
    for a, b in zip(runs[0], runs[1]):
        assert (a is None and b is None) or torch.equal(a.raw, b.raw), what + ": two runs differ"
    return runs[0], runs[2]


def _chain(C, dt):
    V = 8 if dt else 4
    return V * math.ceil(C / (16 * V)) + 4


@pytest.mark.parametrize("npix", sorted(NPIX))
@pytest.mark.parametrize("C", CS + [1024])
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_layer_norm(dt, C, npix):
    L = _lib()
    bf = dt == 1
    store = ST if bf else 0.0
    eps = 1e-6
    for case, (off, use_pb) in enumerate(((0.3, True), (100.0, False))):      # the second: mean 100, std 1, no pre_bias
        gen = _gen(1, dt, C, npix, case)
        x = _draw(gen, (npix, C), bf, 1.0, off)
        dy = _draw(gen, (npix, C), bf)
        prior = _draw(gen, (npix, C), bf)
        gamma, beta = _vec(gen, C, 0.5, 1.5), _vec(gen, C, -0.3, 0.3)
        pb = _vec(gen, C, -0.5, 0.5) if use_pb else None
        gd, bd = gamma.float().cuda(), beta.float().cuda()
        pd = pb.float().cuda() if use_pb else None
        xb = Wide(npix, C, dt, x)
        F = R.ln_fwd(x, pb, gamma, beta, eps)
        u = F["u"]
        A = u.abs().max(1, keepdim=True)[0] + u.abs().mean(1, keepdim=True)
        r = F["r"][:, None]
        Kf = _chain(C, dt) + 6
        tol_y = 2 * Kf * U * (r * gamma.abs() * A * (1 + F["xh"].abs()) + beta.abs()) + store * F["y"].abs()
        for with_stats in (True, False):
            yb = Wide(npix, C, dt)
            stats = Floats(2 * npix, "cuda", torch.full((2 * npix,), float("nan"))) if with_stats else None
            L.call("ydl_ln_fwd", dt, xb.ptr, xb.ld, _P(pd), _P(gd), _P(bd), eps, yb.ptr, yb.ld, _P(stats.raw) if stats else None, npix, C,
                   _stream())
            torch.cuda.synchronize()
            yb.check("ydl_ln_fwd: y")
            xb.check("ydl_ln_fwd: x")
            _note("ln_fwd", dt, "y", R.compare(yb.logical(), F["y"], tol_y))
            if stats:
                stats.check_guards("ydl_ln_fwd: stats")
                sv = stats.v.view(npix, 2).double().cpu()
                _note("ln_fwd", dt, "mu", R.compare(sv[:, 0], F["mu"], 2 * Kf * U * u.abs().mean(1)))
                _note("ln_fwd", dt, "r", R.compare(sv[:, 1], F["r"], 2 * Kf * U * (r * (1 + r * A))[:, 0]))
        # backward from the reference's statistics rounded to f32: operands of kernel and reference alike
        mu32, r32 = F["mu"].float().double(), F["r"].float().double()
        st = torch.stack([mu32, r32], 1).float().contiguous().cuda()
        B = R.ln_bwd(x, pb, gamma, mu32, r32, dy)
        rr = r32[:, None]
        E = rr * (u.abs().max(1, keepdim=True)[0] + mu32.abs()[:, None])
        gbar = B["g"].abs().mean(1, keepdim=True)
        Kb = _chain(C, dt) + 8
        S_dx = rr * (B["g"].abs() + gbar + B["xh"].abs() * (B["g"] * B["xh"]).abs().mean(1, keepdim=True)
                     + E * (B["m2"].abs() + B["xh"].abs() * gbar))
        tol_dx = 2 * Kb * U * S_dx
        dyb = Wide(npix, C, dt, dy)
        for acc in (0, 1):
            def launch(mk):
                dxb = Wide(npix, C, dt, prior if acc else None)
                rows = [mk(), mk(), mk() if use_pb else None]
                ws = _ws(L.lib().ydl_ln_bwd_ws_bytes(npix, C))
                L.call("ydl_ln_bwd", dt, xb.ptr, xb.ld, _P(pd), _P(gd), _P(st), dyb.ptr, dyb.ld, dxb.ptr, dxb.ld, acc, _P(rows[0].raw),
                       _P(rows[1].raw), _P(rows[2].raw) if use_pb else None, _P(ws.raw), npix, C, _stream())
                torch.cuda.synchronize()
                ws.check_guards("ydl_ln_bwd: workspace")
                dxb.check("ydl_ln_bwd: dx")
                launch.dx = dxb
                return rows
            zero, twos = _sum_runs(launch, C, "ydl_ln_bwd")
            want = B["dx"] + (prior if acc else 0.0)
            _note("ln_bwd", dt, "dx", R.compare(launch.dx.logical(), want, tol_dx + (U * (prior.abs() + B["dx"].abs()) if acc else 0.0)
                                                + store * want.abs()))
            t_g = 2 * 20 * U * (dy.abs() * (B["xh"].abs() + E)).sum(0)
            t_b = 2 * 20 * U * dy.abs().sum(0)
            t_p = tol_dx.sum(0) + 2 * 20 * U * B["dx"].abs().sum(0)
            for i, (name, t) in enumerate((("dgamma", t_g), ("dbeta", t_b), ("dpre_bias", t_p))):
                if zero[i] is None:
                    continue
                _note("ln_bwd", dt, name, R.compare(zero[i].v.cpu(), B[name], t + U * B[name].abs()))
                _note("ln_bwd", dt, name + "+2", R.compare(twos[i].v.cpu(), B[name] + 2.0, t + 2 * U * (2.0 + B[name].abs())))
    print("[convnext ln]", "bf16" if dt else "f32", C, npix, {k[0]: f"{v:.3f}" for k, v in WORST.items() if k[1] == ("bf16" if dt else "f32")
                                                              and k[0].startswith("ln")})


def test_layer_norm_served_set_and_refusals():
    L = _lib()
    lib = L.lib()
    assert [c for c in (0, 4, 8, 12, 16, 96, 1024, 1032, 2048) if lib.ydl_ln_supported(c)] == [8, 16, 96, 1024]
    x = Wide(4, 12, 0, torch.zeros(4, 12, dtype=torch.float64))
    y = Wide(4, 12, 0)
    g = torch.ones(16, device="cuda")
    with pytest.raises(L.YdlError, match="multiple of 8"):
        L.call("ydl_ln_fwd", 0, x.ptr, x.ld, None, _P(g), _P(g), 1e-6, y.ptr, y.ld, None, 4, 12, _stream())
    with pytest.raises(L.YdlError, match="strides"):
        L.call("ydl_ln_fwd", 0, x.ptr, 6, None, _P(g), _P(g), 1e-6, y.ptr, y.ld, None, 4, 8, _stream())
    with pytest.raises(L.YdlError, match="null"):
        L.call("ydl_ln_bwd", 0, x.ptr, x.ld, None, _P(g), None, x.ptr, x.ld, y.ptr, y.ld, 0, _P(g), _P(g), None, _P(g), 4, 8, _stream())
    torch.cuda.synchronize()
    y.check("refused")
    assert bool((y.v.view(torch.int32) == SENT).all())               # refused without a launch


SPECIAL = [0.0, 1e-3, -1e-3, 5.0, -5.0, 12.0, -12.0, 40.0, -40.0]


@pytest.mark.parametrize("npix", sorted(NPIX))
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_bias_gelu(dt, C, npix):
    L = _lib()
    bf = dt == 1
    store = ST if bf else 0.0
    gen = _gen(2, dt, C, npix)
    bias = _vec(gen, C, -0.5, 0.5)
    z = torch.randn(npix, C, generator=gen, dtype=torch.float64) * 2.0
    flat = z.view(-1)
    n = min(len(SPECIAL), flat.numel())
    flat[:n] = torch.tensor(SPECIAL[:n], dtype=torch.float64) - bias.repeat(npix)[:n]      # u = the special values (up to z's rounding)
    z = R.rnd(z, bf)
    dy = _draw(gen, (npix, C), bf)
    bd = bias.float().cuda()
    zb, yb = Wide(npix, C, dt, z), Wide(npix, C, dt)
    L.call("ydl_bias_gelu_fwd", dt, zb.ptr, zb.ld, _P(bd), yb.ptr, yb.ld, npix, C, _stream())
    torch.cuda.synchronize()
    yb.check("ydl_bias_gelu_fwd: y")
    u = z + bias
    erf = torch.erf(u / math.sqrt(2.0))
    ref = R.gelu_fwd(z, bias)
    arg = 1.13 * (z.abs() + bias.abs())
    assert bool(torch.isfinite(yb.logical()).all())
    _note("gelu_fwd", dt, "y", R.compare(yb.logical(), ref, 2 * 8 * U * (0.5 * u.abs() * (1 + erf.abs()) + arg) + store * ref.abs()))
    B = R.gelu_bwd(z, bias, dy)
    S_dz = dy.abs() * (0.5 * (1 + erf.abs()) + u.abs() * B["pdf"] * (1 + 0.5 * u * u) + 0.8 * (z.abs() + bias.abs()))
    tol_dz = 2 * 8 * U * S_dz
    for in_place in (False, True):
        def launch(mk):
            dyb = Wide(npix, C, dt, dy)
            dzb = dyb if in_place else Wide(npix, C, dt)
            rows = [mk()]
            ws = _ws(L.lib().ydl_bias_gelu_bwd_ws_bytes(npix, C))
            L.call("ydl_bias_gelu_bwd", dt, zb.ptr, zb.ld, _P(bd), dyb.ptr, dyb.ld, dzb.ptr, dzb.ld, _P(rows[0].raw), _P(ws.raw), npix, C,
                   _stream())
            torch.cuda.synchronize()
            ws.check_guards("ydl_bias_gelu_bwd: workspace")
            dzb.check("ydl_bias_gelu_bwd: dz")
            dyb.check("ydl_bias_gelu_bwd: dy")
            launch.dz = dzb
            return rows
        zero, twos = _sum_runs(launch, C, "ydl_bias_gelu_bwd")
        assert bool(torch.isfinite(launch.dz.logical()).all())
        _note("gelu_bwd", dt, "dz", R.compare(launch.dz.logical(), B["dz"], tol_dz + store * B["dz"].abs()))
        t = tol_dz.sum(0) + 2 * K_ACC * U * B["dz"].abs().sum(0)
        _note("gelu_bwd", dt, "dbias", R.compare(zero[0].v.cpu(), B["dbias"], t + U * B["dbias"].abs()))
        _note("gelu_bwd", dt, "dbias+2", R.compare(twos[0].v.cpu(), B["dbias"] + 2.0, t + 2 * U * (2.0 + B["dbias"].abs())))
    zb.check("ydl_bias_gelu: z")
    print("[convnext gelu]", "bf16" if dt else "f32", C, npix, {k[0]: f"{v:.3f}" for k, v in WORST.items() if k[1] == ("bf16" if dt else "f32")
                                                                and k[0].startswith("gelu")})


@pytest.mark.parametrize("npix", sorted(NPIX))
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_scale_residual(dt, C, npix):
    L = _lib()
    bf = dt == 1
    store = ST if bf else 0.0
    N, hw = NPIX[npix]
    for case, (gscale, keep) in enumerate(((1.0, None), (1e-6, None), (1.0, [0.0, 2.0][:N] if N > 1 else [0.0]), (1.0, [2.0, 0.5][:N]))):
        gen = _gen(3, dt, C, npix, case)
        x, y, dout, prior = (_draw(gen, (npix, C), bf) for _ in range(4))
        gamma = _vec(gen, C, 0.5, 1.5) * gscale
        gamma = gamma.float().double()
        kt = torch.tensor(keep, dtype=torch.float64) if keep is not None else None
        gd = gamma.float().cuda()
        kd = kt.float().cuda() if kt is not None else None
        xb, yb, ob = Wide(npix, C, dt, x), Wide(npix, C, dt, y), Wide(npix, C, dt)
        L.call("ydl_scale_res_fwd", dt, yb.ptr, yb.ld, _P(gd), _P(kd), xb.ptr, xb.ld, ob.ptr, ob.ld, N, hw, C, _stream())
        torch.cuda.synchronize()
        ob.check("ydl_scale_res_fwd: out")
        ref = R.scale_res_fwd(y, gamma, kt, x, hw)
        kr = R._keep_rows(kt, npix, hw)
        _note("scale_res_fwd", dt, "out", R.compare(ob.logical(), ref, 2 * 3 * U * (x.abs() + (kr * gamma * y).abs()) + store * ref.abs()))
        if kt is not None:
            for n in range(N):
                if keep[n] == 0.0:                                    # a dropped sample: x bit for bit
                    assert torch.equal(ob.bits()[n * hw:(n + 1) * hw], xb.bits()[n * hw:(n + 1) * hw])
        B = R.scale_res_bwd(dout, y, gamma, kt, hw)
        db = Wide(npix, C, dt, dout)
        for dx_mode in ("none", "store", "add"):
            def launch(mk):
                dyb = Wide(npix, C, dt)
                dxb = None if dx_mode == "none" else Wide(npix, C, dt, prior if dx_mode == "add" else None)
                rows = [mk()]
                ws = _ws(L.lib().ydl_scale_res_bwd_ws_bytes(N, hw, C))
                L.call("ydl_scale_res_bwd", dt, db.ptr, db.ld, yb.ptr, yb.ld, _P(gd), _P(kd), dyb.ptr, dyb.ld, dxb.ptr if dxb else None,
                       dxb.ld if dxb else 0, 1 if dx_mode == "add" else 0, _P(rows[0].raw), _P(ws.raw), N, hw, C, _stream())
                torch.cuda.synchronize()
                ws.check_guards("ydl_scale_res_bwd: workspace")
                dyb.check("ydl_scale_res_bwd: dy")
                if dxb:
                    dxb.check("ydl_scale_res_bwd: dx")
                launch.dy, launch.dx = dyb, dxb
                return rows
            zero, twos = _sum_runs(launch, C, "ydl_scale_res_bwd")
            _note("scale_res_bwd", dt, "dy", R.compare(launch.dy.logical(), B["dy"], 2 * 2 * U * B["dy"].abs() + store * B["dy"].abs()))
            if dx_mode == "store":
                assert torch.equal(launch.dx.bits(), db.bits())
            elif dx_mode == "add":
                want = dout + prior
                _note("scale_res_bwd", dt, "dx", R.compare(launch.dx.logical(), want, U * want.abs() + store * want.abs()))
            t = 2 * K_ACC * U * (kr * dout * y).abs().sum(0)
            _note("scale_res_bwd", dt, "dgamma", R.compare(zero[0].v.cpu(), B["dgamma"], t + U * B["dgamma"].abs()))
            _note("scale_res_bwd", dt, "dgamma+2", R.compare(twos[0].v.cpu(), B["dgamma"] + 2.0, t + 2 * U * (2.0 + B["dgamma"].abs())))
        for b in (xb, yb, db):
            b.check("ydl_scale_res: operand")
    print("[convnext scale_res]", "bf16" if dt else "f32", C, npix,
          {k[0]: f"{v:.3f}" for k, v in WORST.items() if k[1] == ("bf16" if dt else "f32") and k[0].startswith("scale")})


def test_worst_share_of_a_bound():
    """runs last in this file: the worst share of its bound per kernel and dtype over all the cases above"""
    print("[convnext kernels] worst share of a bound:", {f"{k[0]} {k[1]}": f"{v:.3f}" for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())
