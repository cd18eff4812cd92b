"""CPU: the float64 reference of the ConvNeXt pieces (tests/convnext_ref.py) equals torch's own nn.LayerNorm / nn.GELU autograd in
float64, its modules equal the composition of torch's layers, and the comparison the GPU tests use rejects the wrong answers a kernel
could give, each evaluated in f32 and held to the f32 bound of tests/test_gpu_convnext_kernels.py: the variance over C - 1, eps = 1e-5,
the tanh-approximate GELU, a dropped pre_bias, a missing keep factor, and dgamma without the keep factor."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import convnext_ref as R

U = R.U24


def _data(npix=30, C=24, seed=0, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(npix, C, generator=gen, dtype=torch.float64) * scale).float().double()
    dy = torch.randn(npix, C, generator=gen, dtype=torch.float64).float().double()
    gamma = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double()
    beta = (torch.rand(C, generator=gen, dtype=torch.float64) * 0.6 - 0.3).float().double()
    pb = (torch.rand(C, generator=gen, dtype=torch.float64) - 0.5).float().double()
    return x, dy, gamma, beta, pb


def test_layer_norm_formulas_equal_torch_autograd():
    x, dy, gamma, beta, pb = _data()
    xr, gr, br, pr = (t.clone().requires_grad_(True) for t in (x, gamma, beta, pb))
    ln = F.layer_norm(xr + pr, (x.shape[1],), gr, br, 1e-6)
    ln.backward(dy)
    Fw = R.ln_fwd(x, pb, gamma, beta, 1e-6)
    B = R.ln_bwd(x, pb, gamma, Fw["mu"], Fw["r"], dy)
    assert torch.allclose(Fw["y"], ln.detach(), rtol=1e-12, atol=1e-12)
    for got, want in ((B["dx"], xr.grad), (B["dgamma"], gr.grad), (B["dbeta"], br.grad), (B["dpre_bias"], pr.grad)):
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-11)
    mod = nn.LayerNorm(24, eps=1e-6).double()
    with torch.no_grad():
        mod.weight.copy_(gamma); mod.bias.copy_(beta)
    assert torch.allclose(R.ln_fwd(x, None, gamma, beta, 1e-6)["y"], mod(x), rtol=1e-12, atol=1e-12)


def test_gelu_formulas_equal_torch_autograd():
    x, dy, _g, _b, pb = _data(scale=2.0)
    zr, br = x.clone().requires_grad_(True), pb.clone().requires_grad_(True)
    y = nn.GELU()(zr + br)
    y.backward(dy)
    B = R.gelu_bwd(x, pb, dy)
    assert torch.allclose(R.gelu_fwd(x, pb), y.detach(), rtol=1e-12, atol=1e-14)
    assert torch.allclose(B["dz"], zr.grad, rtol=1e-11, atol=1e-13) and torch.allclose(B["dbias"], br.grad, rtol=1e-11, atol=1e-12)


def test_scale_residual_formulas_equal_torch_autograd():
    x, dout, gamma, _b, _pb = _data()
    y = _data(seed=1)[0]
    keep = torch.tensor([0.0, 2.0], dtype=torch.float64)
    xr, yr, gr = (t.clone().requires_grad_(True) for t in (x, y, gamma))
    out = xr + keep.repeat_interleave(15)[:, None] * gr * yr
    out.backward(dout)
    B = R.scale_res_bwd(dout, y, gamma, keep, 15)
    assert torch.equal(R.scale_res_fwd(y, gamma, keep, x, 15), out.detach())
    assert torch.equal(R.scale_res_fwd(y, gamma, keep, x, 15)[:15], x[:15])
    assert torch.allclose(B["dy"], yr.grad) and torch.allclose(B["dgamma"], gr.grad) and torch.equal(B["dx"], xr.grad)


def test_modules_equal_the_composition_of_torch_layers():
    torch.manual_seed(0)
    blk = R.CNBlock(16, 1.0, 0.0).double()
    with torch.no_grad():
        blk.layer_scale.uniform_(0.5, 1.5)
    x = torch.randn(2, 16, 6, 10, dtype=torch.float64)
    t = blk.block[0](x).permute(0, 2, 3, 1)
    t = blk.block[5](blk.block[4](blk.block[3](blk.block[2](t)))).permute(0, 3, 1, 2)
    assert torch.allclose(blk(x), x + blk.layer_scale * t, rtol=1e-12, atol=1e-12)
    blk.fixed_keep = torch.tensor([0.0, 2.0], dtype=torch.float64)
    out = blk(x)
    assert torch.equal(out[0], x[0]) and torch.allclose(out[1], x[1] + 2.0 * blk.layer_scale * t[1], rtol=1e-12, atol=1e-12)
    ln = R.LayerNorm2d(16).double()
    assert torch.allclose(ln(x), F.layer_norm(x.permute(0, 2, 3, 1), (16,), ln.weight, ln.bias, 1e-6).permute(0, 3, 1, 2))
    assert R.stem(3, 16)(torch.randn(2, 3, 12, 20)).shape == (2, 16, 3, 5) and R.down(16, 32)(torch.randn(2, 16, 6, 10)).shape == (2, 32, 3, 5)
    # the bf16-storage variant differs from the exact one by bf16-sized errors only, and really rounds
    r = R.CNBlock(16, 1.0, 0.0, store=True).double()
    r.load_state_dict(blk.state_dict())
    want = (x + blk.layer_scale * t).detach()
    err = float((r(x).detach() - want).abs().max() / want.abs().max())
    assert 2.0 ** -12 < err < 2.0 ** -5


def test_rows_have_the_sizes_of_convnext_tiny():
    rows = [R.convnext_tiny1(), R.convnext_tiny2(), R.convnext_tiny3()]
    assert [sum(p.numel() for p in r.parameters()) for r in rows] == [1235040, 11112960, 15470592]
    ps = [m.p for r in rows for m in r.modules() if isinstance(m, R.CNBlock)]
    assert len(ps) == 18 and all(abs(p - 0.1 * j / 17) < 1e-12 for j, p in enumerate(ps))
    rows[0].eval()
    assert rows[0](torch.randn(1, 3, 32, 32)).shape == (1, 192, 4, 4)


def _f32_bounds_ln(x, pb, gamma, beta, eps, C):
    """the f32 forward bound of tests/test_gpu_convnext_kernels.py for these operands"""
    Fw = R.ln_fwd(x, pb, gamma, beta, eps)
    u = Fw["u"]
    A = u.abs().max(1, keepdim=True)[0] + u.abs().mean(1, keepdim=True)
    K = 4 * math.ceil(C / 64) + 4 + 6
    return Fw, 2 * K * U * (Fw["r"][:, None] * gamma.abs() * A * (1 + Fw["xh"].abs()) + beta.abs())


def test_the_comparison_rejects_wrong_layer_norms():
    x, dy, gamma, beta, pb = _data(npix=30, C=24, scale=0.01)          # a small variance: eps matters
    Fw, tol = _f32_bounds_ln(x, pb, gamma, beta, 1e-6, 24)
    assert R.compare(Fw["y"].float(), Fw["y"], tol)[1] == 0                                           # the right answer in f32 passes
    assert R.compare(R.ln_fwd(x, pb, gamma, beta, 1e-6, ddof=1)["y"].float(), Fw["y"], tol)[1] > 0    # variance over C - 1
    assert R.compare(R.ln_fwd(x, pb, gamma, beta, 1e-5)["y"].float(), Fw["y"], tol)[1] > 0            # eps = 1e-5
    assert R.compare(R.ln_fwd(x, None, gamma, beta, 1e-6)["y"].float(), Fw["y"], tol)[1] > 0          # pre_bias dropped
    # at C = 1024 the C - 1 variance is 5e-4 off: still outside the f32 bound
    x, dy, gamma, beta, pb = _data(npix=4, C=1024)
    Fw, tol = _f32_bounds_ln(x, pb, gamma, beta, 1e-6, 1024)
    assert R.compare(Fw["y"].float(), Fw["y"], tol)[1] == 0
    assert R.compare(R.ln_fwd(x, pb, gamma, beta, 1e-6, ddof=1)["y"].float(), Fw["y"], tol)[1] > 0
    # backward: a dropped pre_bias moves dx and dgamma
    B = R.ln_bwd(x, pb, gamma, Fw["mu"], Fw["r"], dy)
    Bw = R.ln_bwd(x, None, gamma, Fw["mu"], Fw["r"], dy)
    assert R.compare(Bw["dgamma"].float(), B["dgamma"], 2 * 20 * U * (dy.abs() * (B["xh"].abs() + 10.0)).sum(0))[1] > 0


def test_the_comparison_rejects_the_tanh_gelu():
    x, dy, _g, _b, pb = _data(scale=2.0)
    u = x + pb
    ref = R.gelu_fwd(x, pb)
    tol = 2 * 8 * U * (0.5 * u.abs() * (1 + torch.erf(u / math.sqrt(2.0)).abs()) + 1.13 * (x.abs() + pb.abs()))
    assert R.compare(ref.float(), ref, tol)[1] == 0
    assert R.compare(R.gelu_fwd(x, pb, approximate="tanh").float(), ref, tol)[1] > 0
    assert R.compare(F.gelu(u, approximate="tanh").float(), ref, tol)[1] > 0


def test_the_comparison_rejects_missing_keep_factors():
    x, dout, gamma, _b, _pb = _data()
    y = _data(seed=1)[0]
    keep = torch.tensor([0.0, 2.0], dtype=torch.float64)
    ref = R.scale_res_fwd(y, gamma, keep, x, 15)
    kr = R._keep_rows(keep, 30, 15)
    tol = 2 * 3 * U * (x.abs() + (kr * gamma * y).abs())
    assert R.compare(ref.float(), ref, tol)[1] == 0
    assert R.compare(R.scale_res_fwd(y, gamma, None, x, 15).float(), ref, tol)[1] > 0               # keep ignored
    B = R.scale_res_bwd(dout, y, gamma, keep, 15)
    t = 2 * 258 * U * (kr * dout * y).abs().sum(0) + U * B["dgamma"].abs()
    assert R.compare(B["dgamma"].float(), B["dgamma"], t)[1] == 0
    assert R.compare(R.scale_res_bwd(dout, y, gamma, keep, 15, keep_in_dgamma=False)["dgamma"].float(), B["dgamma"], t)[1] > 0
    assert R.compare(R.scale_res_bwd(dout, y, gamma, None, 15)["dy"].float(), B["dy"], 4 * U * B["dy"].abs())[1] > 0
