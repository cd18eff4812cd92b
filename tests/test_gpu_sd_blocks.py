"""GPU: the space / depth layers, the bare BatchNorm2d row and BottleneckCSP at module level — ``Focus``, ``Contract`` and ``Expand``
through Tape.space_to_depth / depth_to_space (csrc/s2d.hip), ``BatchNorm2d`` through Tape.bn_act, ``BottleneckCSP`` with the two halves of
its BatchNorm riding on the convolutions that produce them.  The scaffold is tests/block_harness.py.
* f32 mode against the nine fixtures of tools/make_sd_golden.py (the reference's own classes in float64): the output, the gradient of x
  and of every parameter, 1e-4 relative to each tensor's max (the project's bound for module fixtures); the running statistics equal the
  fixture's and every ``num_batches_tracked`` has advanced by exactly one (a BottleneckCSP whose halves each counted a step, or each
  updated the other's running channels, fails here); the eval-mode forward runs and leaves the state alone;
* bf16 mode against the same fixtures: per fixture and kind the bound is FLOOR_FACTOR = 4 times the bf16 floor the fixture records — the
  module's own error on the same data when its tensors pass through bf16 where a bf16 implementation stores them.  The same factor and
  reasoning as the cross blocks: the kernels sum in another order and round at other points, and single draws on small tensors scatter
  by a small multiple.  Contract and Expand move bytes: in bf16 mode their output is the bf16-rounded input, permuted, to the bit;
* the small yaml model of tests/test_builders_sd_cpu.py takes a full eager training step in bf16 and in f32 at a 32^2 input, every
  parameter touched and moved, the prediction (2, 12, 32, 32);
* in deterministic f32 mode five steps replayed from the launch list leave the same losses and state as the eager steps, bit for bit:
  ydl_space_to_depth, ydl_depth_to_space and ydl_bn_stats are in the replay table;
* a frozen ``BottleneckCSP.cv2.weight`` gets no gradient and is not marked touched; ``bn``'s parameters and the input still get theirs."""
import json
import os

import numpy as np
import pytest
import torch

from tests.block_harness import (check_bf16_against_floor, check_f32_fixture, check_replay_equals_eager, eager_step_checks, load_module,
                                 train_setup)
from tests.sd_ref import depth_to_space_ref, space_to_depth_ref
from tests.test_builders_sd_cpu import FILES, YAML, build, has_running_stats

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 4.0
IDS = [os.path.basename(f)[:-4] for f in FILES]
MOVERS = [f for f in FILES if os.path.basename(f).startswith(("sd_contract", "sd_expand"))]


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_modules_match_the_fixtures(path):
    z = np.load(path)

    def after_eval(mod, _x, _out, _out_eval):
        # the state after the ONE train-mode step (the eval-mode forward has just run and must not have moved it)
        sd = mod.state_dict()
        for k in sd:
            if k.endswith("num_batches_tracked"):
                assert int(sd[k]) == int(z["p." + k]) + 1, k
    check_f32_fixture(path, build, expect_running_stats=has_running_stats(path), after_eval=after_eval)


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_bf16_mode_against_the_fixtures(path):
    check_bf16_against_floor(path, build, FLOOR_FACTOR, ("out", "grad", "run") if has_running_stats(path) else ("out", "grad"), "sd")


@pytest.mark.parametrize("path", MOVERS, ids=[os.path.basename(f)[:-4] for f in MOVERS])
def test_contract_and_expand_move_bf16_bits(path):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("bf16")
    z = np.load(path)
    s = json.loads(str(z["args"]))[0]
    fwd, bwd = (space_to_depth_ref, depth_to_space_ref) if str(z["cls"]) == "Contract" else (depth_to_space_ref, space_to_depth_ref)
    mod = load_module(z, build)
    x = torch.from_numpy(z["x"]).float().cuda().requires_grad_(True)
    gout = torch.from_numpy(z["grad_out"]).float()
    out = mod(x)
    out.backward(gout.cuda())
    torch.cuda.synchronize()
    assert torch.equal(out.detach().cpu(), fwd(torch.from_numpy(z["x"]).float().bfloat16(), s, 0).float())
    assert torch.equal(x.grad.cpu(), bwd(gout.bfloat16(), s, 0).float())


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
        csp, bn = m.model[1], m.model[5]
        for p in (csp.cv2.weight, csp.cv3.weight, csp.bn.weight, csp.bn.bias, bn.weight, bn.bias):     # in the flat arenas like every layer's
            assert opt.params_arena.data_ptr() <= p.data_ptr() < opt.params_arena.data_ptr() + opt.params_arena.numel() * 4
            assert opt.grads_arena.data_ptr() <= p.grad.data_ptr() < opt.grads_arena.data_ptr() + opt.grads_arena.numel() * 4
        sd = m.state_dict()
        assert int(sd["model.1.bn.num_batches_tracked"]) == 1 and int(sd["model.5.num_batches_tracked"]) == 1
        assert not torch.equal(after["model.1.bn.running_mean"][:16], before["model.1.bn.running_mean"][:16])
        assert not torch.equal(after["model.1.bn.running_mean"][16:], before["model.1.bn.running_mean"][16:])
    finally:
        ydl.set_compute_dtype("bf16")


def test_replayed_step_equals_the_eager_step_bit_for_bit():
    check_replay_equals_eager(_setup, "sd", ("ydl_space_to_depth", "ydl_depth_to_space", "ydl_bn_stats"))


def test_checkpoint_round_trips_the_new_layers(tmp_path):
    import yolo_dual_amd as ydl
    try:
        m, opt, _crit, _xs, _ts = _setup("f32")
        path = str(tmp_path / "sd.pt")
        ydl.save_checkpoint(path, m.state_dict(), opt, epoch=0)
        fresh = ydl.SegYoloModel(YAML)
        ydl.load_weights(fresh, path)
        want = m.state_dict()
        for k, v in fresh.state_dict().items():
            assert torch.equal(v.cpu(), want[k].cpu()), k
    finally:
        ydl.set_compute_dtype("bf16")


def test_a_frozen_cv2_weight_gets_no_gradient_and_is_not_marked_touched():
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    try:
        torch.manual_seed(2)
        m = ydl.BottleneckCSP(16, 32, 1).cuda().train()
        m.cv2.weight.requires_grad_(False)
        x = torch.randn(2, 16, 8, 8, device="cuda", requires_grad=True)
        out = m(x)
        out.backward(torch.randn_like(out))
        torch.cuda.synchronize()
        assert m.cv2.weight.grad is None and not getattr(m.cv2.weight, "_ydl_touched", False)
        assert m.cv3.weight.grad is not None and bool((m.cv3.weight.grad != 0).any()) and getattr(m.cv3.weight, "_ydl_touched", False)
        for p in (m.bn.weight, m.bn.bias):
            assert p.grad is not None and bool((p.grad[:16] != 0).any()) and bool((p.grad[16:] != 0).any()) and getattr(p, "_ydl_touched", False)
        assert x.grad is not None and bool((x.grad != 0).any())
    finally:
        ydl.set_compute_dtype("bf16")
