"""GPU: the dilated blocks (Conv with d > 1, BasicConv, ASPP, RFB) through Tape.dilated_conv.
* f32 mode against the fixtures recorded from the reference's own classes in float64 (tools/make_dilated_golden.py): the output, the
  gradient of x and of every parameter, and the running statistics after the step, 1e-4 relative to each tensor's max (the
  project's bound for module fixtures); the eval-mode forward runs and leaves the state alone;
* bf16 mode against the same fixtures, at twice the errors measured on an MI355X (BF16_TOL below);
* the small yaml model of tests/test_builders_dilated_cpu.py (an RFB row with inter-plane widths 4, 6 and 8, a dilated Conv, two
  ASPP rows) takes a full eager training step in bf16 and in f32, every parameter touched and moved;
* in deterministic f32 mode five steps replayed from the launch list leave the same losses and state as the eager steps, bit for
  bit (tests/block_harness.py)."""
import os

import pytest
import torch

from tests.block_harness import check_bf16_against_tol, check_f32_fixture, check_replay_equals_eager, eager_step_checks, train_setup
from tests.test_builders_dilated_cpu import FILES, YAML, build

pytestmark = pytest.mark.gpu

# bf16 mode, worst error over the four fixtures relative to each tensor's max, measured on an MI355X: output 6.8e-3 (ASPP), gradients
# (x and parameters) 2.9e-1, running statistics 3.5e-3; the bounds are twice that.  The gradient figure is RFB's (a BatchNorm bias
# gradient in branch2; its grad_x 1.7e-1, its other gradients 2e-3 ... 1.3e-1): five ReLUs over 128 pixels per channel, where a
# bf16 rounding that flips one mask entry moves a 128-term sum by several percent.  Every gradient of the other three fixtures is
# below 5.1e-3, and the same RFB step in f32 mode is within 9e-7 everywhere.
BF16_TOL = {"out": 1.4e-2, "grad": 5.8e-1, "run": 7.0e-3}


# a BatchNorm bias gradient below this fraction of its layer's weight gradient counts as exactly zero (the relu=False 1x1 BasicConv that
# opens every RFB branch, in front of a linear layer and another train-mode BatchNorm) and is measured against that weight gradient
ZERO_BIAS_REL = 1e-6


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_modules_match_the_reference_fixtures(path):
    # ASPP holds no BatchNorm
    check_f32_fixture(path, build, expect_running_stats=os.path.basename(path) != "dil_aspp_16_8.npz", zero_bias_rel=ZERO_BIAS_REL)


def test_bf16_mode_against_the_fixtures():
    check_bf16_against_tol(FILES, build, BF16_TOL, "dilated", zero_bias_rel=ZERO_BIAS_REL)


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
        dw = m.model[4].atrous_block12.weight
        assert dw.data_ptr() >= opt.params_arena.data_ptr() and dw.grad.data_ptr() >= opt.grads_arena.data_ptr()
    finally:
        ydl.set_compute_dtype("bf16")


def test_replayed_step_equals_the_eager_step_bit_for_bit():
    check_replay_equals_eager(_setup, "dilated")
