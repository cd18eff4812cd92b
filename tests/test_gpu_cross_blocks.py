"""GPU: cross convolutions at module level — ``Conv`` with a (1, k) / (k, 1) kernel, ``CrossConv`` and ``C3x`` through Tape.xconv_bn_act.
* f32 mode against the five fixtures recorded from the reference's own classes in float64 (tools/make_cross_golden.py): the output,
  the gradient of x and of every parameter, and the running statistics after the step, 1e-4 relative to each tensor's max (the
  project's bound for module fixtures); the eval-mode forward runs and leaves the state alone;
* bf16 mode against the same fixtures: per fixture and kind (output / gradients / running statistics) the bound is FLOOR_FACTOR times
  the bf16 floor the fixture records — the reference's own error on the same data when its input, convolution weights, convolution
  outputs, Conv outputs and their incoming gradients pass through bf16.  The factor is a margin over that emulation: the kernels sum in
  another order and round at other points, and single draws on 100-pixel tensors scatter by a small multiple;
* the small yaml model of tests/test_builders_cross_cpu.py (a CrossConv down-sampler, then a C3x with two CrossConvs and shortcuts)
  takes a full eager training step in bf16 and in f32 at a 32^2 input, every parameter touched and moved;
* in deterministic f32 mode five steps replayed from the launch list leave the same losses and state as the eager steps, bit for
  bit (tests/block_harness.py): the new entry points are in the replay table."""
import os

import pytest
import torch

from tests.block_harness import check_bf16_against_floor, check_f32_fixture, check_replay_equals_eager, eager_step_checks, train_setup
from tests.test_builders_cross_cpu import FILES, YAML, build

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 4.0


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_modules_match_the_reference_fixtures(path):
    check_f32_fixture(path, build)


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_bf16_mode_against_the_fixtures(path):
    check_bf16_against_floor(path, build, FLOOR_FACTOR, ("out", "grad", "run"), "cross")


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
        for w in (m.model[1].cv1.conv.weight, m.model[2].m[1].cv2.conv.weight):
            assert w.data_ptr() >= opt.params_arena.data_ptr() and w.grad.data_ptr() >= opt.grads_arena.data_ptr()
            assert w.permute(0, 2, 3, 1).is_contiguous() and w.grad.permute(0, 2, 3, 1).is_contiguous()
    finally:
        ydl.set_compute_dtype("bf16")


def test_replayed_step_equals_the_eager_step_bit_for_bit():
    check_replay_equals_eager(_setup, "cross", ("ydl_xconv_fwd", "ydl_xconv_dgrad", "ydl_xconv_wgrad"))
