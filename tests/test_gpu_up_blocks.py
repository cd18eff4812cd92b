"""GPU: the decoder up-samplers at module level — ``ConvTranspose2d`` through Tape.conv_transpose (the implicit-GEMM entry points on the
mirrored geometry), ``DWConvTranspose2d`` through Tape.dw_conv_transpose (csrc/tconv.hip) and ``Upsample(mode='bicubic')`` through
Tape.resize (ydl_bicubic_fwd / ydl_bicubic_bwd).  The scaffold is tests/block_harness.py.
* f32 mode against the seven fixtures of tools/make_up_golden.py (torch / the reference's own DWConvTranspose2d in float64): the output,
  the gradient of x and of every parameter, 1e-4 relative to each tensor's max (the project's bound for module fixtures); the eval-mode forward runs and leaves the state alone;
* bf16 mode against the same fixtures: per fixture and kind (output / gradients) the bound is FLOOR_FACTOR = 4 times the bf16 floor the
  fixture records — the module's own error on the same data when its input, weight, output and incoming gradient pass through bf16.  The
  same factor and reasoning as the cross blocks: the kernels sum in another order and round at other points (the dense forward stores
  the convolution and then the biased sum: two roundings), and single draws on small tensors scatter by a small multiple;
* the small yaml model of tests/test_builders_up_cpu.py (both transposed rows, two Concats with earlier layers, a bicubic Upsample)
  takes a full eager training step in bf16 and in f32 at a 32^2 input, every parameter touched and moved;
* in deterministic f32 mode five steps replayed from the launch list leave the same losses and state as the eager steps, bit for bit:
  the new entry points are in the replay table;
* a frozen ``ConvTranspose2d.weight`` gets no gradient and is not marked touched; its bias and its input still get theirs."""
import os

import pytest
import torch

from tests.block_harness import check_bf16_against_floor, check_f32_fixture, check_replay_equals_eager, eager_step_checks, train_setup
from tests.test_builders_up_cpu import FILES, YAML, build

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 4.0


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_modules_match_the_fixtures(path):
    check_f32_fixture(path, build, expect_running_stats=False)


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_bf16_mode_against_the_fixtures(path):
    check_bf16_against_floor(path, build, FLOOR_FACTOR, ("out", "grad"), "up")


def _setup(mode):
    return train_setup(YAML, mode, 32)


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_yaml_model_takes_a_full_eager_step(mode):
    import yolo_dual_amd as ydl
    try:
        m, opt, crit, xs, ts = _setup(mode)
        params, before, after = eager_step_checks(m, opt, crit, xs, ts, (2, 12, 32, 32))
        for k in params:                                   # the fused optimizer step moved every parameter
            assert not torch.equal(before[k], after[k]), k
        for w in (m.model[4].weight, m.model[6].weight):
            assert w.data_ptr() >= opt.params_arena.data_ptr() and w.grad.data_ptr() >= opt.grads_arena.data_ptr()
            assert w.permute(0, 2, 3, 1).is_contiguous() and w.grad.permute(0, 2, 3, 1).is_contiguous()
    finally:
        ydl.set_compute_dtype("bf16")


def test_replayed_step_equals_the_eager_step_bit_for_bit():
    check_replay_equals_eager(_setup, "up", ("ydl_dwtconv_fwd", "ydl_dwtconv_dgrad", "ydl_dwtconv_wgrad", "ydl_bicubic_fwd", "ydl_bicubic_bwd",
                                             "ydl_conv_wgrad_det"))


def test_a_frozen_weight_gets_no_gradient_and_is_not_marked_touched():
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    try:
        torch.manual_seed(2)
        m = ydl.ConvTranspose2d(16, 24, 4, 2, 1).cuda().train()
        m.weight.requires_grad_(False)
        x = torch.randn(2, 16, 5, 7, device="cuda", requires_grad=True)
        out = m(x)
        out.backward(torch.randn_like(out))
        torch.cuda.synchronize()
        assert m.weight.grad is None and not getattr(m.weight, "_ydl_touched", False)
        assert m.bias.grad is not None and bool((m.bias.grad != 0).any()) and getattr(m.bias, "_ydl_touched", False)
        assert x.grad is not None and bool((x.grad != 0).any())
    finally:
        ydl.set_compute_dtype("bf16")
