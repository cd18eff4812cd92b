"""GPU: grouped convolution at module level — ``Conv(g > 1)`` and ``SPPCSPC_group`` through Tape.gconv_bn_act.
* f32 mode against the fixtures recorded from the reference's own classes in float64 (tools/make_gconv_golden.py): the output, the
  gradient of x and of every parameter, and the running statistics after the step, 1e-4 relative to each tensor's max (the
  project's bound for module fixtures); the eval-mode forward runs and leaves the state alone;
* bf16 mode against the same fixtures, at twice the errors measured on an MI355X (BF16_TOL below);
* the small yaml model of tests/test_builders_gconv_cpu.py (SPPCSPC_group, then a C3 whose Bottleneck has a 3x3 with g = 2 and a
  residual) takes a full eager training step in bf16 and in f32, every parameter touched and moved;
* in deterministic f32 mode five steps replayed from the launch list leave the same losses and state as the eager steps, bit for
  bit (tests/block_harness.py): the new entry points are in the replay table."""
import os

import pytest
import torch

from tests.block_harness import check_bf16_against_tol, check_f32_fixture, check_replay_equals_eager, eager_step_checks, train_setup
from tests.test_builders_gconv_cpu import FILES, YAML, build

pytestmark = pytest.mark.gpu

# bf16 mode, worst error over the two fixtures relative to each tensor's max, measured on an MI355X against the float64 fixtures
# (the same figures in three runs): output 4.94e-2, gradients (x and parameters) 3.26e-1 (cv3's BatchNorm weight), running statistics
# 7.54e-3 (cv6's running mean), all three SPPCSPC_group's: seven Conv + BN layers deep with the pools in the middle (the dense
# CSP pool blocks of tests/test_gpu_spp_blocks.py, the same depth at 16 channels, are at 1.5e-2 / 2.7e-1 / 3.2e-3).  The single Conv(32, 96, 3, g=2) is at 3.7e-3 / 4.6e-3 / 4.2e-3.  The bounds are twice the figures; the same steps in f32
# mode are within 1.7e-5 everywhere.
BF16_TOL = {"out": 9.9e-2, "grad": 6.5e-1, "run": 1.5e-2}


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_modules_match_the_reference_fixtures(path):
    check_f32_fixture(path, build)


def test_bf16_mode_against_the_fixtures():
    check_bf16_against_tol(FILES, build, BF16_TOL, "gconv")


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
        for w in (m.model[2].cv5.conv.weight, m.model[3].m[0].cv2.conv.weight):
            assert w.data_ptr() >= opt.params_arena.data_ptr() and w.grad.data_ptr() >= opt.grads_arena.data_ptr()
    finally:
        ydl.set_compute_dtype("bf16")


def test_replayed_step_equals_the_eager_step_bit_for_bit():
    check_replay_equals_eager(_setup, "gconv", ("ydl_gconv_fwd",))
