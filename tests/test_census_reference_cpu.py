"""The float64 reference routines and the comparison function of tests/census.py, held to torch's own float64 convolution (forward,
input gradient, weight gradient) and to float64 autograd of act(batch_norm(y)) with a residual, on the CPU: the launch census
(tests/test_gpu_launch_census.py) judges every kernel by these routines, so they must be right on their own.

The last test is the census' sensitivity, kept where no kernel has to misbehave: a bf16-rounded copy of the float64 reference passes
the per-element bound; the same copy with one element moved by 2^-7 |ref|, with one K-slice of 64 channels left out of the sum, or with
one 8-pixel strip shifted by one pixel fails it — and a relative-L2 check at 2e-2 passes all three."""
import pytest
import torch
import torch.nn.functional as F

from tests import census as Z

RTOL = 1e-12


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _operands(g, seed, ldw_block=False):
    """strided NHWC buffers with a canary outside the logical channels, and the same tensors in NCHW float64"""
    gen = torch.Generator().manual_seed(seed)
    kk, cip, cop = g.k * g.k, Z.r8(g.Cin), Z.r8(g.Cout)
    xb = torch.full((g.N * g.Hi * g.Wi, g.ldx), Z.CANARY, dtype=torch.float64)
    xb[:, :g.Cin] = torch.randn(g.N * g.Hi * g.Wi, g.Cin, generator=gen, dtype=torch.float64)
    xb[:, g.Cin:cip] = 0
    dyb = torch.full((g.N * g.Ho * g.Wo, g.ldy), Z.CANARY, dtype=torch.float64)
    dyb[:, :g.Cout] = torch.randn(g.N * g.Ho * g.Wo, g.Cout, generator=gen, dtype=torch.float64)
    dyb[:, g.Cout:cop] = 0
    w = torch.randn(g.Cout, g.Cin, g.k, g.k, generator=gen, dtype=torch.float64)
    wk = torch.zeros(g.Cout, kk, cip, dtype=torch.float64)
    wk[..., :g.Cin] = w.permute(0, 2, 3, 1).reshape(g.Cout, kk, g.Cin)
    wt = torch.zeros(g.Cin, kk, cop, dtype=torch.float64)
    wt[..., :g.Cout] = w.permute(1, 2, 3, 0).reshape(g.Cin, kk, g.Cout)
    x = xb.view(g.N, g.Hi, g.Wi, g.ldx)[..., :g.Cin].permute(0, 3, 1, 2)
    dy = dyb.view(g.N, g.Ho, g.Wo, g.ldy)[..., :g.Cout].permute(0, 3, 1, 2)
    return xb, dyb, wk, wt, x, dy, w


def _geom(N, H, W, Cin, Cout, k, s, p, ldx, ldy, ldw=0):
    return Z.Geom(N, H, W, Cin, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, Cout, k, s, p, ldx, ldy, ldw)


# small ragged shapes: row strides wider than the channel count, channel counts that are not multiples of 8, strides 1 and 2
GEOMS = [_geom(2, 9, 11, 12, 20, 3, 1, 1, 24, 40), _geom(3, 13, 10, 16, 10, 3, 2, 1, 16, 24), _geom(2, 7, 9, 5, 8, 1, 1, 0, 16, 8),
         _geom(1, 12, 9, 8, 16, 1, 2, 0, 8, 32), _geom(2, 17, 15, 3, 8, 7, 2, 3, 8, 8), _geom(1, 10, 14, 24, 12, 6, 2, 2, 40, 16)]


@pytest.mark.parametrize("g", GEOMS, ids=lambda g: f"k{g.k}s{g.s}_{g.Cin}to{g.Cout}")
def test_im2col_references_match_torch_float64(g):
    xb, dyb, wk, wt, x, dy, w = _operands(g, 3)
    ref_y = F.conv2d(x, w, stride=g.s, padding=g.p)
    _own, y, _q, _a = Z.conv_fwd_ref(g, xb, wk)
    assert _rel(y, ref_y.permute(0, 2, 3, 1).reshape(-1, g.Cout)) < RTOL
    ref_dx = torch.nn.grad.conv2d_input((g.N, g.Cin, g.Hi, g.Wi), w, dy, stride=g.s, padding=g.p)
    _own, dx, _q, _a = Z.conv_dgrad_ref(g, dyb, wt)
    assert _rel(dx, ref_dx.permute(0, 2, 3, 1).reshape(-1, g.Cin)) < RTOL
    ref_dw = torch.nn.grad.conv2d_weight(x, (g.Cout, g.Cin, g.k, g.k), dy, stride=g.s, padding=g.p)
    _own, dw, _q, _a = Z.conv_wgrad_ref(g, xb, dyb)
    dw = dw.view(g.Cout, g.k * g.k, Z.r8(g.Cin))
    assert _rel(dw[..., :g.Cin], ref_dw.permute(0, 2, 3, 1).reshape(g.Cout, g.k * g.k, g.Cin)) < RTOL
    assert float(dw[..., g.Cin:].abs().max()) == 0.0 if g.Cin % 8 else True


def test_prior_contents_and_error_measures():
    g = GEOMS[0]
    xb, dyb, wk, wt, x, dy, w = _operands(g, 5)
    prior = torch.randn(g.N * g.Ho * g.Wo, g.Cout, dtype=torch.float64)
    own, y, Q, A = Z.conv_fwd_ref(g, xb, wk, prior=prior)
    ref = F.conv2d(x, w, stride=g.s, padding=g.p).permute(0, 2, 3, 1).reshape(-1, g.Cout)
    assert _rel(own, ref) < RTOL and _rel(y, ref + prior) < RTOL
    q2 = F.conv2d(x * x, w * w, stride=g.s, padding=g.p).permute(0, 2, 3, 1).reshape(-1, g.Cout) + prior * prior
    ab = F.conv2d(x.abs(), w.abs(), stride=g.s, padding=g.p).permute(0, 2, 3, 1).reshape(-1, g.Cout) + prior.abs()
    assert _rel(Q, q2.sqrt()) < RTOL and _rel(A, ab) < RTOL
    assert bool((Q <= A * (1 + 1e-12)).all()) and bool((y.abs() <= A * (1 + 1e-12)).all())


def test_column_block_of_a_wider_weight_matrix():
    """ldw != 0: the launch's weights are columns [col0, col0 + Cin_p) of a wider 1x1 matrix; the forward reads them there, the weight
    gradient of the block equals the dense one"""
    g = _geom(2, 7, 9, 16, 24, 1, 1, 0, 24, 24, ldw=72)
    xb, dyb, wk, wt, x, dy, w = _operands(g, 7)
    wide = torch.full((g.Cout, g.ldw), Z.CANARY, dtype=torch.float64)
    wide[:, 40:56] = wk.view(g.Cout, 16)
    _own, y, _q, _a = Z.conv_fwd_ref(g, xb, wide, col0=40)
    ref = F.conv2d(x, w).permute(0, 2, 3, 1).reshape(-1, g.Cout)
    assert _rel(y, ref) < RTOL
    _own, dw, _q, _a = Z.conv_wgrad_ref(g, xb, dyb)
    assert _rel(dw, torch.nn.grad.conv2d_weight(x, w.shape, dy).reshape(g.Cout, g.Cin)) < RTOL


def test_dgrad_term_count_is_the_tap_count_of_the_parity_class():
    g = _geom(1, 8, 10, 8, 16, 3, 2, 1, 8, 16)
    K = Z.dgrad_terms(g, "cpu").view(g.Hi, g.Wi)
    # 3x3 / stride 2 / pad 1: even rows and columns see one tap per axis, odd ones two
    assert K[0, 0] == 1 * 16 and K[1, 0] == 2 * 16 and K[1, 1] == 4 * 16 and K[0, 3] == 2 * 16
    g1 = _geom(1, 8, 10, 8, 16, 3, 1, 1, 8, 16)
    assert bool((Z.dgrad_terms(g1, "cpu") == 9 * 16).all())
    g2 = _geom(1, 8, 10, 8, 16, 1, 2, 0, 8, 16)          # 1x1 / stride 2: the odd positions receive nothing
    K2 = Z.dgrad_terms(g2, "cpu").view(8, 10)
    assert K2[0, 0] == 16 and K2[1, 0] == 0 and K2[0, 1] == 0


ACTS = [(Z.ACT_NONE, lambda z: z), (Z.ACT_SILU, F.silu), (Z.ACT_RELU, torch.relu)]


@pytest.mark.parametrize("res_mode", [Z.RES_NONE, Z.RES_AFTER_ACT, Z.RES_BEFORE_ACT])
@pytest.mark.parametrize("act,fn", ACTS, ids=["none", "silu", "relu"])
def test_batchnorm_restatements_match_float64_autograd(act, fn, res_mode):
    gen = torch.Generator().manual_seed(11 + act + 3 * res_mode)
    n, C, eps, mom, rep = 301, 13, 1e-3, 0.1, 1
    y = (torch.randn(n, C, generator=gen, dtype=torch.float64) * 1.5 + 0.5).requires_grad_(True)
    gamma = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (torch.rand(C, generator=gen, dtype=torch.float64) - 0.5).requires_grad_(True)
    res = torch.randn(n, C, generator=gen, dtype=torch.float64).requires_grad_(True)
    dout = torch.randn(n, C, generator=gen, dtype=torch.float64)
    rm0, rv0 = torch.randn(C, generator=gen, dtype=torch.float64), torch.rand(C, generator=gen, dtype=torch.float64) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    bn = F.batch_norm(y, rm, rv, gamma, beta, training=True, momentum=mom, eps=eps)
    if res_mode == Z.RES_BEFORE_ACT:
        out = fn(bn + res)
    elif res_mode == Z.RES_AFTER_ACT:
        out = fn(bn) + res
    else:
        out = fn(bn)
    (out * dout).sum().backward()
    # forward: replica rows of the column sums (here in float64: the routine sums the rows it is given)
    yd = y.detach()
    frac = torch.rand(8, C, generator=gen, dtype=torch.float64) + 0.25
    frac = frac / frac.sum(0)
    R = Z.bn_coeffs_ref(frac * yd.sum(0), frac * (yd * yd).sum(0), n, gamma.detach(), beta.detach(), eps, mom, rm0, rv0, rep)
    assert _rel(R["rm"], rm) < 1e-11 and _rel(R["rv"], rv) < 1e-11
    o = Z.bn_apply_ref(yd, R["scale"], R["shift"], act, res_mode, res.detach())
    assert _rel(o, out.detach()) < 1e-11
    # backward
    B = Z.bn_bwd_ref(yd, dout, R["mean"], R["invstd"], R["scale"], R["shift"], act, res_mode, out=o, res=res.detach())
    assert _rel(B["dy"], y.grad) < 1e-9
    assert _rel(B["dgamma"], gamma.grad) < 1e-9 and _rel(B["dbeta"], beta.grad) < 1e-9
    if res_mode != Z.RES_NONE:
        assert _rel(B["dres"], res.grad) < 1e-9
        prior = torch.randn(n, C, generator=gen, dtype=torch.float64)
        B2 = Z.bn_bwd_ref(yd, dout, R["mean"], R["invstd"], R["scale"], R["shift"], act, res_mode | Z.RES_GRAD_ACCUMULATE, out=o,
                          res=res.detach(), dres_prior=prior)
        assert _rel(B2["dres"], res.grad + prior) < 1e-9
    else:
        assert B["dres"] is None
    # the apply pass alone takes the two sums from outside
    B3 = Z.bn_bwd_ref(yd, dout, R["mean"], R["invstd"], R["scale"], R["shift"], act, res_mode, out=o, res=res.detach(),
                      sums=(B["dbeta"], B["dgamma"]))
    assert _rel(B3["dy"], B["dy"]) < 1e-14


def test_running_variance_of_a_replicated_tensor():
    """replication r: the logical tensor is the stored one repeated r times; only the unbiased factor changes"""
    gen = torch.Generator().manual_seed(2)
    y = torch.randn(50, 4, generator=gen, dtype=torch.float64)
    one, zero = torch.ones(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    R = Z.bn_coeffs_ref(y.sum(0)[None], (y * y).sum(0)[None], 50, one, zero, 1e-3, 0.1, zero, one, 4)
    big = y.repeat(4, 1)
    assert _rel(R["unb"], big.var(0, unbiased=True)) < 1e-12 and _rel(R["var"], big.var(0, unbiased=False)) < 1e-12


def _l2(a, b):
    return float((a - b).norm() / b.norm())


def test_per_element_bound_sees_what_relative_l2_does_not():
    g = _geom(4, 96, 128, 128, 32, 3, 1, 1, 128, 32)          # 49 152 pixels: an eighth of the benchmark's largest maps
    gen = torch.Generator().manual_seed(9)
    kk = 9
    xb = torch.randn(g.N * g.Hi * g.Wi, 128, generator=gen).bfloat16()
    wk = (torch.randn(32, kk, 128, generator=gen) / (kk * 128) ** 0.5).bfloat16()
    _own, ref, Q, A = Z.conv_fwd_ref(g, xb, wk)
    tol = Z.stored_bound(ref, Z.acc_bound(kk * g.Cin, Q, A), True)
    good = ref.float().bfloat16().double()                       # one round-to-nearest of the exact result (through f32)
    ratio, over, _i = Z.worst(good, ref, tol)
    assert over == 0 and ratio <= 1.0, ratio
    # (a) one element moved by 2^-7 |ref|
    i = int(ref.abs().reshape(-1).argmax())
    bad = good.clone()
    bad.view(-1)[i] = ref.view(-1)[i] * (1 + 2.0 ** -7)
    assert Z.worst(bad, ref, tol)[1] >= 1 and _l2(bad, ref) < 2e-2
    # (b) one K-slice of 64 channels left out of the sum, for one tile of 128 pixels
    wk2 = wk.clone()
    wk2[:, 4, 64:] = 0
    _o, part, _q, _a = Z.conv_fwd_ref(g, xb, wk2)
    bad = good.clone()
    bad[256:384] = part[256:384].float().bfloat16().double()
    assert Z.worst(bad, ref, tol)[1] > 1000 and _l2(bad, ref) < 2e-2
    # (c) one 8-pixel strip shifted by one pixel
    bad = good.clone()
    bad[801:809] = good[800:808]
    assert Z.worst(bad, ref, tol)[1] > 64 and _l2(bad, ref) < 2e-2
    # a non-finite value and a value that must be exact
    bad = good.clone()
    bad[0, 0] = float("nan")
    assert Z.worst(bad, ref, tol)[1] == 1
    zero = torch.zeros(3, dtype=torch.float64)
    assert Z.worst(zero, zero, zero)[1] == 0 and Z.worst(zero + 1e-30, zero, zero)[1] == 3


def test_recorded_arguments_reduce_to_distinct_cases():
    """pointer values are not part of a case; every integer, flag and NULL-ness is"""
    import ctypes
    g = Z.Geom(2, 8, 8, 16, 8, 8, 32, 1, 1, 0, 16, 32, 0)
    P = ctypes.c_void_p
    cen = Z.Census()
    cen._settle = lambda: None                      # (no library here: kernel names are not read)
    cen.add("ydl_conv_fwd_sums", (g, 1, P(4096), P(8192), P(12288), P(64), 0, P(0)))
    cen.add("ydl_conv_fwd_sums", (g, 1, P(1 << 20), P(2 << 20), P(3 << 20), P(128), 0, P(0)))
    cen.add("ydl_conv_fwd", (g, 1, P(4096), P(8192), P(12288), None, 1, P(0)))
    cen.add("ydl_conv_fwd", (g._replace(ldy=64), 1, P(4096), P(8192), P(12288), P(0), 1, P(0)))
    cen.add("ydl_fill_zero", (P(4096), 64, P(0)))
    cen.add("ydl_conv_dgrad_bnred", (g, 1, P(1), P(2), P(3), 0, None, P(0)))
    assert [s["count"] for s in cen.cases.values()] == [2, 1, 1, 1]
    assert cen.total["conv"] == 5 and cen.total["bn"] == 0
    unknown = list(cen.cases.values())[-1]["case"]
    with pytest.raises(Z.CensusFailure, match="ydl_conv_dgrad_bnred"):
        Z.check_case(unknown)
