"""GPU: the SPP pyramid blocks (SPP, C3SPP, SPPCSPC through Tape.spp_pools; SimSPPF, SimCSPSPPF through Tape.sppf_pools).
* f32 mode against the fixtures recorded from the reference's own classes in float64 (tools/make_spp_golden.py): the output, the
  gradient of x and of every parameter, and the running statistics after the step, 1e-4 relative to each tensor's max (the
  project's bound for module fixtures); the eval-mode forward runs and leaves the state alone;
* bf16 mode against the same fixtures, at twice the errors measured on an MI355X (BF16_TOL below);
* the small yaml model of tests/test_builders_spp_cpu.py (one row of each block) takes a full eager training step in bf16 and in
  f32, every parameter touched and moved;
* in deterministic f32 mode five steps replayed from the launch list leave the same losses and state as the eager steps, bit for
  bit (tests/block_harness.py): the new entry points are in the replay table."""
import os

import pytest
import torch

from tests.block_harness import (check_bf16_against_tol, check_f32_fixture, check_replay_equals_eager, eager_step_checks, rel_max_err,
                                 train_setup)
from tests.test_builders_spp_cpu import FILES, YAML, build

pytestmark = pytest.mark.gpu

# bf16 mode, worst error over the five fixtures relative to each tensor's max, measured on an MI355X against the float64 fixtures
# (the same figures in three runs): output 1.54e-2 (SimCSPSPPF), gradients (x and parameters) 2.71e-1, running statistics 3.24e-3
# (SimCSPSPPF, cv5's running mean); the bounds are twice that.  The gradient figure is SPPCSPC's (the BatchNorm bias of cv1; its
# grad_x 2.6e-1, SimCSPSPPF's grad_x 2.3e-1): seven Conv + BN layers deep with the pools in the middle.  SPP alone is at 7.7e-2
# (grad_x), C3SPP at 8.6e-2, SimSPPF with its two ReLU layers at 1.5e-1; the same steps in f32 mode are within 3.1e-6 everywhere.
BF16_TOL = {"out": 3.1e-2, "grad": 5.4e-1, "run": 6.5e-3}


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_modules_match_the_reference_fixtures(path):
    check_f32_fixture(path, build)


def test_bf16_mode_against_the_fixtures():
    check_bf16_against_tol(FILES, build, BF16_TOL, "spp")


def test_a_plane_too_large_for_lds_takes_one_pool_per_window():
    """SPP on a 44 x 44 plane in f32 mode (1936 pixels: ydl_spp_pool_supported says 0, Tape.spp_pools issues three max-pool launches
    each way) against the same layers in torch float64 on the module's own parameters: output, grad_x and cv1's weight gradient,
    1e-4 of each tensor's max as for the fixtures"""
    import torch.nn.functional as F
    import yolo_dual_amd as ydl
    from yolo_dual_amd import _lib as L
    assert L.lib().ydl_spp_pool_supported(L.YDL_F32, 44, 44, 8, 5, 9, 13) == 0
    ydl.set_compute_dtype("f32")
    try:
        torch.manual_seed(5)
        mod = ydl.SPP(16, 16).cuda().train()
        x = torch.randn(1, 16, 44, 44, device="cuda", requires_grad=True)
        g = torch.randn(1, 16, 44, 44, device="cuda")
        out = mod(x)
        out.backward(g)
        torch.cuda.synchronize()

        def conv(c, t, w):
            t = F.conv2d(t, w, None, c.conv.stride, c.conv.padding)
            return F.silu(F.batch_norm(t, None, None, c.bn.weight.detach().double(), c.bn.bias.detach().double(), True, 0.0, c.bn.eps))
        xr = x.detach().double().requires_grad_(True)
        w1 = mod.cv1.conv.weight.detach().double().requires_grad_(True)
        y = conv(mod.cv1, xr, w1)
        ref = conv(mod.cv2, torch.cat([y] + [F.max_pool2d(y, k, 1, k // 2) for k in mod.k], 1), mod.cv2.conv.weight.detach().double())
        ref.backward(g.double())
        errs = {"out": rel_max_err(out, ref.detach().cpu()), "grad_x": rel_max_err(x.grad, xr.grad.cpu()),
                "g.cv1.conv.weight": rel_max_err(mod.cv1.conv.weight.grad, w1.grad.cpu())}
        print("[spp 44x44]", {k: f"{v:.1e}" for k, v in errs.items()})
        assert all(v < 1e-4 for v in errs.values()), errs
    finally:
        ydl.set_compute_dtype("bf16")


def _setup(mode):
    return train_setup(YAML, mode, 8)


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_yaml_model_takes_a_full_eager_step(mode):
    import yolo_dual_amd as ydl
    try:
        m, opt, crit, xs, ts = _setup(mode)
        params, before, after = eager_step_checks(m, opt, crit, xs, ts, (2, 12, 8, 8))
        for k in params:                                   # the fused optimizer step moved every parameter
            assert not torch.equal(before[k], after[k]), k
        w = m.model[3].cv5.conv.weight
        assert w.data_ptr() >= opt.params_arena.data_ptr() and w.grad.data_ptr() >= opt.grads_arena.data_ptr()
    finally:
        ydl.set_compute_dtype("bf16")


def test_replayed_step_equals_the_eager_step_bit_for_bit():
    check_replay_equals_eager(_setup, "spp")
