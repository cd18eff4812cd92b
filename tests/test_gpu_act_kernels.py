"""GPU: the activation kernels at their C ABI against the float64 reference of tests/act_ref.py, per element, f32 and bf16.

Shapes (act_ref.SHAPES): 70 pixels x 24 channels at a row stride of 32, 70 x 20 with Cp = 24 (a channel tail), and 2046 x 16, which
needs more than one CTA in the reduce passes.  Every output has the guard rows of tests/census.py behind it.

Point-wise activations (YDL_ACT_LEAKY with slope 0.1 through the ``_p`` entry points, YDL_ACT_HSWISH and YDL_ACT_MISH through the
entry points without a parameter), all six streaming BatchNorm entry points.  The bounds have the form tests/census.py uses for SiLU:

  forward   L * 8 U24 (|y*scale| + |shift| + |res|)  +  8 U24 |ref|  +  the bf16 store term, L the activation's Lipschitz constant
            (1, 1.5, 1.1): the f32 argument error carried through the activation, and the activation's own evaluation;
  backward  check_bn_act_bwd's form with its dz term 16 U24 |dz| (1 + |z|) written out for an activation other than SiLU: the f32
            evaluation of act' costs a few ulps of |dz|, and the argument error of z meets act'' -- so the term is
            16 U24 (|dz| + A2 |dout| |z|) with A2 the largest |act''| act_ref computes in float64 (0, 1/3, 0.64).  For SiLU
            (A2 = 1/2, act' of order 1) this is the census's own term.

Elements whose z lies within the forward argument error of a kink (0 for LeakyReLU, +-3 for Hardswish) are left out, at most 1 % per
case (tests/test_act_ref_cpu.py checks that the operands meet this on their own); the worst ratios are printed.

AconC: the output, dz and the three per-channel sums, the sums with an ``acc_bound`` over the pixel count; two runs are bit-identical.
Max merge: exact ties planted; forward and both gradients exact to the bit in f32 and within one bf16 rounding in bf16."""
import pytest
import torch

from tests import act_ref as R
from tests.census import BN_BWD_TOL, CANARY, Floats, Rows, _P, _stream, _tdt

pytestmark = pytest.mark.gpu

CODES = [(R.ACT_LEAKY, R.SLOPE), (R.ACT_HSWISH, 0.0), (R.ACT_MISH, 0.0)]
RES_NONE, RES_AFTER = 0, 1
A2 = {}


def _a2(code):
    if code not in A2:
        A2[code] = R.max_d2(code)
    return A2[code]


def _lib():
    from yolo_dual_amd import _lib as L
    return L


def _rows(data, ld, dt, fill=True):
    """census Rows holding ``data`` [npix, C] (None: an output, canary everywhere)"""
    gen = torch.Generator("cuda").manual_seed(1)
    npix, C = data.shape
    r = Rows(npix, ld, C, _tdt(dt), gen, fill=False)
    if fill:
        r.v[:, :C] = data.cuda().to(_tdt(dt))
    return r


def _call(L, name, code, slope, k, *args):
    """the entry point, or its ``_p`` sibling with the slope behind the activation code (argument k) for YDL_ACT_LEAKY"""
    if code == R.ACT_LEAKY:
        L.call(name + "_p", *args[:k + 1], slope, *args[k + 1:])
    else:
        L.call(name, *args)


def _vec(t, Cp):
    return torch.cat([t.float(), torch.zeros(Cp - t.numel())]).cuda()


@pytest.mark.parametrize("shape", sorted(R.SHAPES))
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("code,slope", CODES, ids=["leaky", "hswish", "mish"])
def test_pointwise_forward(shape, dt, code, slope):
    L = _lib()
    npix, C, Cp, ld = R.SHAPES[shape]
    c = R.bn_case(shape, code, dt == 1)
    y, res = _rows(c["y"], ld, dt), _rows(c["res"], ld, dt)
    scale, shift = _vec(c["scale"], Cp), _vec(c["shift"], Cp)
    store = R.BF16_STORE if dt == 1 else 0.0
    worst = {}
    for mode in (RES_NONE, RES_AFTER):
        out = _rows(c["y"], ld, dt, fill=False)
        _call(L, "ydl_bn_act_fwd", code, slope, 8, dt, _P(y.flat), ld, _P(scale), _P(shift), _P(res.flat) if mode else None, ld if mode else 0,
              mode, code, _P(out.flat), ld, npix, Cp, _stream())
        torch.cuda.synchronize()
        ref, z, dz, tol = R.bn_fwd_ref(c, code, slope, bool(mode))
        skip = R.near_kink(z, code, dz)
        ratio, over, left = R.compare(out.logical().cpu(), ref, tol + store * ref.abs(), skip)
        out.check_guards("ydl_bn_act_fwd: out")
        assert left <= 0.01
        worst["fwd res%d" % mode] = (ratio, over)
    # the statistics form: one launch derives the coefficients from replica sums; its output is held to the coefficients it stored
    sums = Floats(8 * 2 * Cp, "cuda")
    sv = sums.v.view(8, 2, Cp)
    sv[0, 0, :C] = c["y"].sum(0).float().cuda()
    sv[0, 1, :C] = (c["y"] * c["y"]).sum(0).float().cuda()
    gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.rand(C, device="cuda") * 0.6 - 0.3
    co = [Floats(Cp, "cuda", torch.full((Cp,), CANARY)) for _ in range(4)]
    out = _rows(c["y"], ld, dt, fill=False)
    _call(L, "ydl_bn_act_fwd_sums", code, slope, 20, dt, _P(y.flat), ld, _P(sums.raw), Cp, npix, _P(gamma), _P(beta), 1e-3, 0.03, None, None,
          _P(co[0].raw), _P(co[1].raw), _P(co[2].raw), _P(co[3].raw), 1, None, 0, RES_NONE, code, _P(out.flat), ld, npix, C, Cp, _stream())
    torch.cuda.synchronize()
    c2 = dict(c, scale=co[2].v[:C].double().cpu(), shift=co[3].v[:C].double().cpu())
    ref, z, dz, tol = R.bn_fwd_ref(c2, code, slope, False)
    ratio, over, left = R.compare(out.logical().cpu(), ref, tol + store * ref.abs(), R.near_kink(z, code, dz))
    out.check_guards("ydl_bn_act_fwd_sums: out")
    for f in co:
        f.check_guards("ydl_bn_act_fwd_sums: coefficients")
    assert left <= 0.01
    worst["fwd_sums"] = (ratio, over)
    print("[act fwd]", shape, "bf16" if dt else "f32", code, {k: f"{v[0]:.3f}" for k, v in worst.items()})
    assert all(v[1] == 0 for v in worst.values()), worst


def _check_bwd(c, code, slope, dt, dy, dres, dgamma, dbeta, entry):
    B = R.bn_bwd_ref(c, code, slope)
    n = float(c["y"].shape[0])
    s = c["scale"].abs()
    t_b, t_g = BN_BWD_TOL * B["sq_b"], BN_BWD_TOL * B["sq_g"]
    store = R.BF16_STORE if dt == 1 else 0.0
    fwd_dz = 8.0 * R.U24 * ((c["y"] * c["scale"]).abs() + c["shift"].abs())
    skip = R.near_kink(B["z"], code, fwd_dz)
    e_dz = 16.0 * R.U24 * (B["dz"].abs() + _a2(code) * c["dout"].abs() * B["z"].abs())
    e_f32 = s * (e_dz + 16.0 * R.U24 * (B["kb"].abs() + (B["xhat"] * B["kg"]).abs()))
    # an element left out still enters the sums, its derivative on either side of the kink: the jump of act' times |dout|
    jump = {R.ACT_LEAKY: 1.0 - slope, R.ACT_HSWISH: 0.5, R.ACT_MISH: 0.0}[code]
    slack_b = (skip.double() * c["dout"].abs() * jump).sum(0)
    slack_g = (skip.double() * (c["dout"] * B["xhat"]).abs() * jump).sum(0)
    tol = store * B["dy"].abs() + s * (t_b + slack_b + B["xhat"].abs() * (t_g + slack_g)) / n + e_f32
    parts = {"dy": R.compare(dy.logical().cpu(), B["dy"], tol, skip)}
    dy.check_guards(entry + ": dy")
    if dres is not None:                       # joined after the activation: dout itself
        parts["dres"] = R.compare(dres.logical().cpu(), c["dout"], store * c["dout"].abs())
        dres.check_guards(entry + ": dres")
    for name, buf, ref, t, sl in (("dgamma", dgamma, B["dgamma"], t_g, slack_g), ("dbeta", dbeta, B["dbeta"], t_b, slack_b)):
        parts[name] = R.compare(buf.v.cpu(), ref, t + 4.0 * R.U24 * ref.abs() + sl)
        buf.check_guards(entry + ": " + name)
    assert all(p[2] <= 0.01 for p in parts.values())
    return parts


@pytest.mark.parametrize("shape", sorted(R.SHAPES))
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("code,slope", CODES, ids=["leaky", "hswish", "mish"])
def test_pointwise_backward(shape, dt, code, slope):
    L = _lib()
    npix, C, Cp, ld = R.SHAPES[shape]
    c = R.bn_case(shape, code, dt == 1)
    y, dout = _rows(c["y"], ld, dt), _rows(c["dout"], ld, dt)
    mean, invstd, scale, shift = (_vec(c[k], Cp) for k in ("mean", "invstd", "scale", "shift"))
    report = {}

    def outputs():
        return (_rows(c["y"], ld, dt, fill=False), _rows(c["y"], ld, dt, fill=False), Floats(C, "cuda"), Floats(C, "cuda"))

    # the two-phase form
    dy, dres, dg, db = outputs()
    ws = Floats(max(L.lib().ydl_bn_bwd_ws_bytes(npix, Cp) // 4, 4), "cuda")
    _call(L, "ydl_bn_act_bwd", code, slope, 13, dt, _P(y.flat), ld, _P(dout.flat), ld, None, 0, None, _P(mean), _P(invstd), _P(scale), _P(shift),
          RES_AFTER, code, _P(dy.flat), ld, _P(dres.flat), ld, _P(dg.raw), _P(db.raw), 0, _P(ws.raw), npix, C, Cp, _stream())
    torch.cuda.synchronize()
    ws.check_guards("ydl_bn_act_bwd: workspace")
    report["bwd"] = _check_bwd(c, code, slope, dt, dy, dres, dg, db, "ydl_bn_act_bwd")
    # replica sums, reduce and apply in one call
    dy, dres, dg, db = outputs()
    sums = Floats(8 * 2 * Cp, "cuda")
    _call(L, "ydl_bn_act_bwd_sums", code, slope, 12, dt, _P(y.flat), ld, _P(dout.flat), ld, None, 0, _P(mean), _P(invstd), _P(scale), _P(shift),
          RES_AFTER, code, _P(dy.flat), ld, _P(dres.flat), ld, _P(dg.raw), _P(db.raw), 0, _P(sums.raw), npix, C, Cp, _stream())
    torch.cuda.synchronize()
    sums.check_guards("ydl_bn_act_bwd_sums: sums")
    report["bwd_sums"] = _check_bwd(c, code, slope, dt, dy, dres, dg, db, "ydl_bn_act_bwd_sums")
    # the reduce pass alone (it writes the residual gradient), then the apply pass alone
    dy, dres, dg, db = outputs()
    sums = Floats(8 * 2 * Cp, "cuda")
    _call(L, "ydl_bn_act_bwd_reduce_sums", code, slope, 12, dt, _P(y.flat), ld, _P(dout.flat), ld, None, 0, _P(mean), _P(invstd), _P(scale),
          _P(shift), RES_AFTER, code, _P(dres.flat), ld, _P(sums.raw), npix, C, Cp, _stream())
    _call(L, "ydl_bn_act_bwd_apply_sums", code, slope, 12, dt, _P(y.flat), ld, _P(dout.flat), ld, None, 0, _P(mean), _P(invstd), _P(scale),
          _P(shift), RES_NONE, code, _P(dy.flat), ld, None, 0, _P(dg.raw), _P(db.raw), 0, _P(sums.raw), npix, C, Cp, _stream())
    torch.cuda.synchronize()
    sums.check_guards("ydl_bn_act_bwd_reduce_sums: sums")
    report["reduce+apply"] = _check_bwd(c, code, slope, dt, dy, dres, dg, db, "ydl_bn_act_bwd_reduce_sums + _apply_sums")
    print("[act bwd]", shape, "bf16" if dt else "f32", code, {e: {k: f"{v[0]:.3f}" for k, v in p.items()} for e, p in report.items()})
    bad = {(e, k): v for e, p in report.items() for k, v in p.items() if v[1]}
    assert not bad, bad


def test_leaky_needs_the_parameter_and_a_residual_before_it_is_refused():
    L = _lib()
    npix, C, Cp, ld = R.SHAPES["70x24_ld32"]
    c = R.bn_case("70x24_ld32", R.ACT_LEAKY, False)
    y, out = _rows(c["y"], ld, 0), _rows(c["y"], ld, 0, fill=False)
    scale, shift = _vec(c["scale"], Cp), _vec(c["shift"], Cp)
    with pytest.raises(L.YdlError, match="ydl_bn_act_fwd_p"):
        L.call("ydl_bn_act_fwd", 0, _P(y.flat), ld, _P(scale), _P(shift), None, 0, 0, R.ACT_LEAKY, _P(out.flat), ld, npix, Cp, _stream())
    with pytest.raises(L.YdlError, match="slope"):
        L.call("ydl_bn_act_fwd_p", 0, _P(y.flat), ld, _P(scale), _P(shift), None, 0, 0, R.ACT_LEAKY, 1.5, _P(out.flat), ld, npix, Cp, _stream())
    ws = Floats(max(L.lib().ydl_bn_bwd_ws_bytes(npix, Cp) // 4, 4), "cuda")
    for code in (R.ACT_HSWISH, R.ACT_MISH):
        with pytest.raises(L.YdlError, match="before the activation"):
            L.call("ydl_bn_act_bwd", 0, _P(y.flat), ld, _P(y.flat), ld, None, 0, None, _P(scale), _P(scale), _P(scale), _P(shift), 2, code,
                   _P(out.flat), ld, _P(out.flat), ld, None, None, 0, _P(ws.raw), npix, C, Cp, _stream())
    torch.cuda.synchronize()
    assert bool((out.v[:, :C].float() == CANARY).all())          # refused without a launch


@pytest.mark.parametrize("shape", sorted(R.SHAPES))
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_acon(shape, dt):
    L = _lib()
    npix, C, Cp, ld = R.SHAPES[shape]
    c = R.acon_case(shape, dt == 1)
    z, dout = _rows(c["z"], ld, dt), _rows(c["dout"], ld, dt)
    p1, p2, beta = (c[k].float().cuda() for k in ("p1", "p2", "beta"))
    store = R.BF16_STORE if dt == 1 else 0.0
    out = _rows(c["z"], ld, dt, fill=False)
    hw = npix // 2
    L.call("ydl_acon_fwd", dt, _P(z.flat), ld, _P(p1), _P(p2), _P(beta), 0, _P(out.flat), ld, npix, hw, C, Cp, _stream())
    torch.cuda.synchronize()
    ref = R.acon_fwd(c["z"], c["p1"], c["p2"], c["beta"])
    d = (c["p1"] - c["p2"]) * c["z"]
    # d, beta*d, the fast sigmoid (a few ulps; its argument error meets |(d sigmoid(beta d))'| <= 1.1 (1 + |beta d|)), two products, a sum
    tol_f = 16.0 * R.U24 * (d.abs() * (1.0 + (c["beta"] * d).abs()) + (c["p2"] * c["z"]).abs()) + store * ref.abs()
    parts = {"out": R.compare(out.logical().cpu(), ref, tol_f)}
    out.check_guards("ydl_acon_fwd: out")
    if Cp > C:
        assert bool((out.v[:, C:Cp].float() == 0).all())
    B = R.acon_bwd(c["z"], c["dout"], c["p1"], c["p2"], c["beta"])
    runs = []
    for _ in range(2):
        dz = _rows(c["z"], ld, dt, fill=False)
        g = [Floats(C, "cuda") for _ in range(3)]
        ws = Floats(max(L.lib().ydl_acon_bwd_ws_bytes(npix, hw, 0, Cp) // 4, 4), "cuda")
        L.call("ydl_acon_bwd", dt, _P(z.flat), ld, _P(dout.flat), ld, _P(p1), _P(p2), _P(beta), 0, _P(dz.flat), ld, 0, _P(g[0].raw), _P(g[1].raw),
               _P(g[2].raw), 0, _P(ws.raw), npix, hw, C, Cp, _stream())
        torch.cuda.synchronize()
        dz.check_guards("ydl_acon_bwd: dz")
        ws.check_guards("ydl_acon_bwd: workspace")
        for f in g:
            f.check_guards("ydl_acon_bwd: parameter gradient")
        runs.append((dz, g))
    dz, g = runs[0]
    assert torch.equal(dz.flat.view(torch.int16 if dt else torch.int32), runs[1][0].flat.view(torch.int16 if dt else torch.int32))
    assert all(torch.equal(a.raw, b.raw) for a, b in zip(g, runs[1][1]))           # no atomics: the same bits
    # g = s (1 + beta d (1 - s)) is bounded by 1.1 in magnitude and its derivative in beta*d by 1/2
    bd = (c["beta"] * d).abs()
    e_g = 16.0 * R.U24 * (1.0 + bd)
    tol_dz = c["dout"].abs() * (16.0 * R.U24 * ((c["p1"] - c["p2"]).abs() * B["g"].abs() + c["p2"].abs())
                                + (c["p1"] - c["p2"]).abs() * e_g) + store * B["dz"].abs()
    parts["dz"] = R.compare(dz.logical().cpu(), B["dz"], tol_dz)
    # a summand's f32 evaluation: dout * z * g and dout * z * (1 - g) carry g's error e_g and a few roundings of factors bounded by
    # 1.1; dout * d^2 * s (1 - s) has s (1 - s) <= 1/4 with a derivative below 0.1, so e_g covers it; then the f32 accumulation
    dzv = (c["dout"] * c["z"]).abs()
    e_sum = {"1": (dzv * (e_g + 8.0 * R.U24 * 1.1)).sum(0), "2": (dzv * (e_g + 8.0 * R.U24 * 1.1)).sum(0),
             "b": (c["dout"].abs() * d * d * e_g).sum(0)}
    for name, buf, k in (("dp1", g[0], "1"), ("dp2", g[1], "2"), ("dbeta", g[2], "b")):
        refv = B[name]
        parts[name] = R.compare(buf.v.cpu(), refv, R.acc_bound(npix, B["q" + k], B["a" + k]) + e_sum[k] + 2.0 * R.U24 * refv.abs())
    print("[acon]", shape, "bf16" if dt else "f32", {k: f"{v[0]:.3f}" for k, v in parts.items()})
    bad = {k: v for k, v in parts.items() if v[1]}
    assert not bad, bad


def test_acon_adds_into_dz_and_into_the_parameter_rows():
    L = _lib()
    npix, C, Cp, ld = R.SHAPES["70x20_cp24"]
    c = R.acon_case("70x20_cp24", False)
    z, dout = _rows(c["z"], ld, 0), _rows(c["dout"], ld, 0)
    p1, p2, beta = (c[k].float().cuda() for k in ("p1", "p2", "beta"))
    prior = _rows(c["dout"] * 0.5, ld, 0)
    g = [Floats(C, "cuda", torch.full((C,), 2.0)) for _ in range(3)]
    ws = Floats(L.lib().ydl_acon_bwd_ws_bytes(npix, npix, 0, Cp) // 4, "cuda")
    L.call("ydl_acon_bwd", 0, _P(z.flat), ld, _P(dout.flat), ld, _P(p1), _P(p2), _P(beta), 0, _P(prior.flat), ld, 1, _P(g[0].raw), _P(g[1].raw),
           _P(g[2].raw), 1, _P(ws.raw), npix, npix, C, Cp, _stream())
    torch.cuda.synchronize()
    B = R.acon_bwd(c["z"], c["dout"], c["p1"], c["p2"], c["beta"])
    want = B["dz"] + (c["dout"] * 0.5).float().double()
    assert R.compare(prior.logical().cpu(), want, 64.0 * R.U24 * (want.abs() + B["dz"].abs() + c["dout"].abs()))[1] == 0
    for buf, k in zip(g, ("dp1", "dp2", "dbeta")):
        assert R.compare(buf.v.cpu(), B[k] + 2.0, 1e-5 * (1.0 + B[k].abs()))[1] == 0


@pytest.mark.parametrize("shape", sorted(R.SHAPES))
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_max_merge_with_planted_ties(shape, dt):
    L = _lib()
    npix, C, Cp, ld = R.SHAPES[shape]
    c = R.max2_case(shape, dt == 1)
    a, b, dout = _rows(c["a"], ld, dt), _rows(c["b"], ld, dt), _rows(c["dout"], ld, dt)
    out, da, db = (_rows(c["a"], ld, dt, fill=False) for _ in range(3))
    L.call("ydl_max2_fwd", dt, _P(a.flat), ld, _P(b.flat), ld, _P(out.flat), ld, npix, Cp, _stream())
    L.call("ydl_max2_bwd", dt, _P(a.flat), ld, _P(b.flat), ld, _P(dout.flat), ld, _P(da.flat), ld, 0, _P(db.flat), ld, 0, npix, Cp, _stream())
    torch.cuda.synchronize()
    for r, what in ((out, "out"), (da, "da"), (db, "db")):
        r.check_guards("ydl_max2: " + what)
    ra, rb = R.max2_bwd(c["a"], c["b"], c["dout"])
    assert torch.equal(out.logical().cpu(), R.max2_fwd(c["a"], c["b"]))                 # a maximum of stored values is a stored value
    store = R.BF16_STORE if dt == 1 else 0.0                                            # half of a bf16 value may need one rounding
    assert R.compare(da.logical().cpu(), ra, store * ra.abs())[1] == 0
    assert R.compare(db.logical().cpu(), rb, store * rb.abs())[1] == 0
    assert int(c["tie"].sum()) > 0 and bool((da.logical().cpu()[c["tie"]] == db.logical().cpu()[c["tie"]]).all())
    # accumulate: the sum is formed in f32 and rounded once
    L.call("ydl_max2_bwd", dt, _P(a.flat), ld, _P(b.flat), ld, _P(dout.flat), ld, _P(da.flat), ld, 1, None, 0, 0, npix, Cp, _stream())
    torch.cuda.synchronize()
    prev = ra.to(_tdt(dt)).double()
    want = (prev + ra)
    assert R.compare(da.logical().cpu(), want, (store + (0.0 if dt else R.U24)) * want.abs())[1] == 0
