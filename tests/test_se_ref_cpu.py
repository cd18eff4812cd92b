"""CPU: the closed formulas of tests/se_ref.py, which the squeeze-excitation kernel tests compare against, pinned to autograd through
``nn.Conv2d(1x1)``, ``F.adaptive_avg_pool2d``, ``F.hardsigmoid`` / ``torch.sigmoid`` and ``F.relu`` / ``F.silu``; and the comparison
helpers shown to reject three wrong answers under the bounds the kernel tests use: a sigmoid derivative taken from the f32-rounded gate
where it saturates, a hardsigmoid that is live at |z| = 3, and a dropped ``dpooled / HW`` term."""
import pytest
import torch
import torch.nn.functional as F

from tests import se_ref as R


def _draw(N, HW, C, Cs, seed, zshift=0.0):
    gen = torch.Generator().manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=torch.float64)
    x, dout = rn(N, HW, C) + 0.5, rn(N, HW, C)
    w1, b1, w2, b2 = rn(Cs, C) * C ** -0.5, rn(Cs) * 0.3, rn(C, Cs) * Cs ** -0.5, rn(C) + zshift
    return x, dout, w1, b1, w2, b2


@pytest.mark.parametrize("act,gate", [("relu", "hardsigmoid"), ("silu", "sigmoid")])
def test_the_closed_formulas_equal_autograd(act, gate):
    N, H, W, C, Cs = 3, 4, 5, 16, 6
    x, dout, w1, b1, w2, b2 = _draw(N, H * W, C, Cs, 1)
    f = R.se_all(x, dout, w1, b1, w2, b2, act, gate)
    xi = x.view(N, H, W, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    ps = [t.clone().requires_grad_(True) for t in (w1.view(Cs, C, 1, 1), b1, w2.view(C, Cs, 1, 1), b2)]
    s = F.conv2d(F.adaptive_avg_pool2d(xi, 1), ps[0], ps[1])
    s = F.conv2d(F.relu(s) if act == "relu" else F.silu(s), ps[2], ps[3])
    out = xi * (F.hardsigmoid(s) if gate == "hardsigmoid" else torch.sigmoid(s))
    out.backward(dout.view(N, H, W, C).permute(0, 3, 1, 2))
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(N, H * W, C)
    # autograd's hardsigmoid slope is the float32 value of 1/6 (see the corner test): 2^-24 relative on everything behind the gate
    rtol, atol = (1e-11, 1e-13) if gate == "sigmoid" else (2e-7, 1e-8)
    assert torch.allclose(rows(out.detach()), f["out"], rtol=1e-12, atol=1e-13)
    assert torch.allclose(rows(xi.grad), f["dx"], rtol=rtol, atol=atol)
    for got, k in zip(ps, ("dw1", "db1", "dw2", "db2")):
        assert torch.allclose(got.grad.reshape(f[k].shape), f[k], rtol=rtol, atol=atol), k
    if act == "relu":
        assert bool((f["h"] < 0).any()) and bool((f["h"] > 0).any())              # both branches of the activation were taken


def test_hardsigmoid_gradient_follows_atens_rule_at_the_corners():
    z = torch.tensor([-3.5, -3.0, -2.999, 0.0, 2.999, 3.0, 3.5], dtype=torch.float64, requires_grad=True)
    F.hardsigmoid(z).sum().backward()
    want = R.gate_grad(z.detach(), "hardsigmoid")
    assert want.tolist() == [0.0, 0.0, 1 / 6, 1 / 6, 1 / 6, 0.0, 0.0]
    # ATen multiplies by the float32 value of 1/6 in every dtype: the same zeros, the live slope equal to 2^-24 relative
    assert torch.equal(z.grad == 0, want == 0) and torch.allclose(z.grad, want, rtol=2.0 ** -24, atol=0)


def test_a_sigmoid_derivative_from_the_rounded_gate_is_rejected():
    N, S, C = 2, 1, 8
    gen = torch.Generator().manual_seed(2)
    z = torch.tensor([8.0, -8.0]).double().repeat(N, C // 2)
    dgate = torch.randn(N, S, C, generator=gen, dtype=torch.float64)
    want = dgate.sum(1) * R.gate_grad(z, "sigmoid")
    tol = R.bound_dz(dgate, z, "sigmoid")
    good = R.rnd(want, False)                                                     # the right answer, stored in f32
    assert R.compare(good, want, tol)[1] == 0
    g32 = R.rnd(torch.sigmoid(z), False)
    wrong = dgate.sum(1) * R.gate_grad(z, "sigmoid", from_gate=g32)
    share, over = R.compare(wrong, want, tol)
    assert over > 0 and share > 10.0, share                    # 1 - g has lost its low bits where the gate saturates at 0.9997


def test_a_hardsigmoid_live_at_three_is_rejected():
    z = torch.tensor([[3.0, -3.0, 1.0, 5.0, -5.0, 0.0, 2.0, -2.0]], dtype=torch.float64)
    dgate = torch.ones(1, 1, 8, dtype=torch.float64)
    want = dgate.sum(1) * R.gate_grad(z, "hardsigmoid")
    tol = R.bound_dz(dgate, z, "hardsigmoid")
    assert float(tol[0, 0]) == 0.0 and float(tol[0, 3]) == 0.0                    # a dead gate demands an exact zero
    assert R.compare(R.rnd(want, False), want, tol)[1] == 0
    wrong = dgate.sum(1) * R.gate_grad(z, "hardsigmoid", live_at_3=True)
    assert R.compare(wrong, want, tol)[1] == 2


@pytest.mark.parametrize("bf16", [False, True])
def test_a_dropped_pooled_term_is_rejected(bf16):
    x, dout, w1, b1, w2, b2 = _draw(2, 15, 8, 4, 3)
    f = R.se_all(x, dout, w1, b1, w2, b2, "silu", "sigmoid")
    dy = R.rnd(dout, bf16)
    want = R.scale_bwd(dy, f["g"], f["dpooled"])
    tol = R.bound_scale_bwd(dy, f["g"], f["dpooled"], None, bf16)
    assert R.compare(R.rnd(want, bf16), want, tol)[1] == 0
    share, over = R.compare(R.rnd(R.scale_bwd(dy, f["g"], f["dpooled"], drop_pooled=True), bf16), want, tol)
    assert over > 0 and share > 10.0, share


def test_compare_counts_non_finite_values_and_demands_equality_at_a_zero_bound():
    ref = torch.zeros(4, dtype=torch.float64)
    assert R.compare(torch.tensor([0.0, float("nan"), 0.0, 1e-30]).double(), ref, torch.zeros(4))[1] == 2
