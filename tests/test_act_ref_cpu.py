"""CPU: tests/act_ref.py, the float64 reference the activation kernels are held to (tests/test_gpu_act_kernels.py), is pinned to torch
autograd in float64: the three point-wise activations with their first and second derivatives, AconC forward and backward, and the max
merge with torch's tie rule.  The comparison helper is shown to reject a wrong slope, a swapped tie rule and a dropped p2 * z term,
and the operands the GPU cases draw are shown to meet the kink condition on their own: at most 1 % of the elements of a case lie
within the f32 argument error of a kink of the activation.  The Mish form of the kernels, n / (n + 2) with n = w (w + 2) and
w = exp(min(z, 20)), is evaluated in f32 on the CPU against float64 over [-30, 30]."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import act_ref as R

CODES = [(R.ACT_LEAKY, 0.1), (R.ACT_HSWISH, 0.0), (R.ACT_MISH, 0.0)]


def _torch_act(code, slope):
    return {R.ACT_LEAKY: nn.LeakyReLU(slope), R.ACT_HSWISH: nn.Hardswish(), R.ACT_MISH: nn.Mish()}[code]


def _grid():
    gen = torch.Generator().manual_seed(5)
    z = torch.cat([torch.linspace(-30, 30, 4001, dtype=torch.float64), torch.randn(4000, generator=gen, dtype=torch.float64) * 3])
    return z[(z.abs() > 1e-9) & ((z.abs() - 3.0).abs() > 1e-9)]


@pytest.mark.parametrize("code,slope", CODES)
def test_pointwise_value_and_derivatives_equal_autograd(code, slope):
    z = _grid().requires_grad_(True)
    out = _torch_act(code, slope)(z)
    (g,) = torch.autograd.grad(out.sum(), z, create_graph=True)
    assert R.compare(R.act(z.detach(), code, slope), out.detach(), 1e-13 * (1 + out.detach().abs()))[1] == 0
    assert R.compare(R.dact(z.detach(), code, slope), g.detach(), 1e-12 * (1 + g.detach().abs()))[1] == 0
    if code != R.ACT_HSWISH:        # torch's hardswish backward is not differentiable a second time
        (g2,) = torch.autograd.grad(g.sum(), z)
        assert R.compare(R.d2act(z.detach(), code, slope), g2, 1e-11 * (1 + g2.abs()))[1] == 0
    else:
        h = 1e-6
        fd = (R.dact(z.detach() + h, code) - R.dact(z.detach() - h, code)) / (2 * h)
        keep = ((z.detach().abs() - 3.0).abs() > 1e-3)
        assert R.compare(R.d2act(z.detach(), code)[keep], fd[keep], 1e-6)[1] == 0
    assert float(R.dact(_grid(), code, slope).abs().max()) <= R.LIPSCHITZ[code]


def test_largest_second_derivatives():
    assert R.max_d2(R.ACT_LEAKY) == 0.0 and abs(R.max_d2(R.ACT_HSWISH) - 1.0 / 3.0) < 1e-15
    assert 0.5 < R.max_d2(R.ACT_MISH) < 0.7


def test_mish_form_of_the_kernels_in_f32():
    zf = torch.linspace(-30, 30, 200001, dtype=torch.float64).float()
    z = zf.double()                   # the reference at the very arguments the f32 form sees
    w = torch.exp(torch.clamp(zf, max=20.0))
    n = w * (w + 2.0)
    t = n / (n + 2.0)
    ref = torch.tanh(F.softplus(z))
    rel = ((t.double() - ref).abs() / ref.abs().clamp_min(1e-300)).max()
    assert float(rel) < 3e-7, float(rel)
    dt = 4.0 * (w / (n + 2.0)) * ((w + 1.0) / (n + 2.0))             # = sigmoid(z) * 4 (n + 1) / (n + 2)^2
    dref = R.dact(z, R.ACT_MISH)
    got = t.double() + z * dt.double()
    assert float((got - dref).abs().max()) < 1e-6


def test_acon_equals_autograd():
    c = R.acon_case("70x20_cp24", False)
    z, p1, p2, beta = (c[k].clone().requires_grad_(True) for k in ("z", "p1", "p2", "beta"))
    d = (p1 - p2) * z
    out = d * torch.sigmoid(beta * d) + p2 * z
    out.backward(c["dout"])
    assert R.compare(R.acon_fwd(c["z"], c["p1"], c["p2"], c["beta"]), out.detach(), 1e-13 * (1 + out.detach().abs()))[1] == 0
    B = R.acon_bwd(c["z"], c["dout"], c["p1"], c["p2"], c["beta"])
    for k, t in (("dz", z), ("dp1", p1), ("dp2", p2), ("dbeta", beta)):
        assert R.compare(B[k], t.grad, 1e-11 * (1 + t.grad.abs()))[1] == 0, k


def test_max_merge_equals_autograd_with_ties():
    c = R.max2_case("70x24_ld32", True)
    assert int(c["tie"].sum()) > 100 and bool((c["a"][c["tie"]] == c["b"][c["tie"]]).all())
    a, b = c["a"].clone().requires_grad_(True), c["b"].clone().requires_grad_(True)
    out = torch.max(a, b)
    out.backward(c["dout"])
    assert torch.equal(R.max2_fwd(c["a"], c["b"]), out.detach())
    da, db = R.max2_bwd(c["a"], c["b"], c["dout"])
    assert torch.equal(da, a.grad) and torch.equal(db, b.grad)
    assert bool((da[c["tie"]] == 0.5 * c["dout"][c["tie"]]).all())


def test_the_comparison_rejects_wrong_kernels():
    c = R.bn_case("70x24_ld32", R.ACT_LEAKY, False)
    out, z, dz, tol = R.bn_fwd_ref(c, R.ACT_LEAKY, 0.1, False)
    skip = R.near_kink(z, R.ACT_LEAKY, dz)
    assert R.compare(out.float(), out, tol, skip)[1] == 0                           # one f32 rounding passes
    assert R.compare(R.act(z, R.ACT_LEAKY, 0.01).float(), out, tol, skip)[1] > 0    # a wrong slope does not
    B = R.bn_bwd_ref(c, R.ACT_LEAKY, 0.1)
    wrong = c["dout"] * R.dact(z, R.ACT_LEAKY, 0.2)
    assert R.compare(wrong.float(), B["dz"], 16 * R.U24 * B["dz"].abs())[1] > 0
    m = R.max2_case("70x24_ld32", False)
    da, db = R.max2_bwd(m["a"], m["b"], m["dout"])
    da_swapped, _ = R.max2_bwd(m["a"], m["b"], m["dout"], tie=1.0)                    # all of a tie to the first operand
    assert R.compare(da, da, 0.0)[1] == 0 and R.compare(da_swapped, da, 0.0)[1] > 0
    a = R.acon_case("70x20_cp24", False)
    ref = R.acon_fwd(a["z"], a["p1"], a["p2"], a["beta"])
    d = (a["p1"] - a["p2"]) * a["z"]
    dropped = d * torch.sigmoid(a["beta"] * d)                                       # without p2 * z
    atol = 16 * R.U24 * (d.abs() + (a["p2"] * a["z"]).abs())
    assert R.compare(ref.float(), ref, atol)[1] == 0 and R.compare(dropped.float(), ref, atol)[1] > 0
    assert R.compare(torch.full_like(ref, float("nan")), ref, atol)[1] == ref.numel()


@pytest.mark.parametrize("shape", sorted(R.SHAPES))
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("code,slope", CODES)
def test_the_kernel_cases_meet_the_kink_condition(shape, bf16, code, slope):
    c = R.bn_case(shape, code, bf16)
    for with_res in (False, True):
        _out, z, dz, _tol = R.bn_fwd_ref(c, code, slope, with_res)
        frac = float(R.near_kink(z, code, dz).double().mean())
        assert frac <= 0.01, (shape, bf16, code, frac)
