"""GPU: the Ghost blocks (DWConv, GhostConv, GhostBottleneck, C3Ghost).
* f32 mode against the fixtures recorded from the reference's own classes in float64 (tools/make_ghost_golden.py): the output, the
  gradient of x and of every parameter, and the running statistics after the step, 1e-4 relative to each tensor's max (the
  project's bound for module fixtures); the eval-mode forward runs and leaves the state alone;
* bf16 mode against the same fixtures, at twice the errors measured on an MI355X (BF16_TOL below);
* GhostConv with a half width of 4 channels (the concat fallback) against the same layer in f32 mode;
* the small yaml model of tests/test_builders_ghost_cpu.py takes a full eager training step in bf16 and in f32, every parameter
  touched and moved;
* in deterministic f32 mode five steps replayed from the launch list leave the same losses and state as the eager steps, bit for
  bit (tests/block_harness.py)."""
import os

import pytest
import torch

from tests.block_harness import (check_bf16_against_tol, check_f32_fixture, check_replay_equals_eager, eager_step_checks, kind, rel_max_err,
                                 train_setup)
from tests.test_builders_ghost_cpu import FILES, YAML, build

pytestmark = pytest.mark.gpu

# bf16 mode, worst error over the six fixtures relative to each tensor's max, measured on an MI355X: output 8.8e-3, gradients (x and
# parameters) 4.5e-2 (a BatchNorm bias gradient of C3Ghost's inner 4-channel GhostConv; every other gradient is below 2.2e-2),
# running statistics 7.9e-3; the bounds are twice that.  The c_ = 4 layer against its f32 run: 6.0e-3 / 6.2e-3.
BF16_TOL = {"out": 1.8e-2, "grad": 9.0e-2, "run": 1.6e-2}


# a BatchNorm bias gradient below this fraction of its layer's weight gradient counts as exactly zero (DWConv(act=False) inside
# GhostBottleneck, in front of a linear layer and another train-mode BatchNorm: float64 leaves ~1e-17) and is measured against that
# weight gradient
ZERO_BIAS_REL = 1e-9


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_modules_match_the_reference_fixtures(path):
    check_f32_fixture(path, build, zero_bias_rel=ZERO_BIAS_REL)


def test_bf16_mode_against_the_fixtures():
    check_bf16_against_tol(FILES, build, BF16_TOL, "ghost", zero_bias_rel=ZERO_BIAS_REL)


def test_ghostconv_unaligned_half_width_takes_the_concat_path():
    """c_ = 4 is half a bf16 chunk: both halves go through Tape.concat.  Same layer, same inputs, f32 mode (whose arithmetic the
    GhostBottleneck fixtures pin: their first GhostConv has c_ = 4) as the reference."""
    import yolo_dual_amd as ydl
    torch.manual_seed(5)
    mod = ydl.GhostConv(16, 8, 1, 1).cuda().train()
    assert mod.c_ == 4
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    x0 = torch.randn(2, 16, 6, 6, device="cuda")
    g0 = torch.randn(2, 8, 6, 6, device="cuda")
    res = {}
    try:
        for mode in ("f32", "bf16"):
            ydl.set_compute_dtype(mode)
            for p in mod.parameters():
                p.grad = None
            x = x0.clone().requires_grad_(True)
            out = mod(x)
            out.backward(g0)
            torch.cuda.synchronize()
            res[mode] = dict(out=out.detach().clone(), grad_x=x.grad.clone(), **{"g." + k: p.grad.clone() for k, p in mod.named_parameters()})
    finally:
        ydl.set_compute_dtype("bf16")
    errs = {k: rel_max_err(res["bf16"][k], res["f32"][k].double().cpu()) for k in res["f32"]}
    print("[ghost c_=4 bf16 vs f32]", {k: f"{v:.1e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < BF16_TOL[kind(k)], (k, v)


def _setup(mode):
    return train_setup(YAML, mode, 4)


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_yaml_model_takes_a_full_eager_step(mode):
    import yolo_dual_amd as ydl
    try:
        m, opt, crit, xs, ts = _setup(mode)
        params, before, after = eager_step_checks(m, opt, crit, xs, ts, (2, 12, 4, 4))
        for k in params:                                   # the fused optimizer step moved every parameter
            assert not torch.equal(before[k], after[k]), k
        dw = m.model[4].conv.weight
        assert dw.data_ptr() >= opt.params_arena.data_ptr() and dw.grad.data_ptr() >= opt.grads_arena.data_ptr()
    finally:
        ydl.set_compute_dtype("bf16")


def test_replayed_step_equals_the_eager_step_bit_for_bit():
    check_replay_equals_eager(_setup, "ghost")
