"""GPU: the Conv activations at module level -- LeakyReLU / Hardswish / Mish inside the streaming BatchNorm kernels of every conv family
they are recorded for (dense, depth-wise, a C3 whose shortcut joins after the activation), AconC through ydl_acon_fwd / _bwd and FReLU
through Tape.dw_bn_act and ydl_max2_fwd / _bwd.
* f32 mode against the eight fixtures recorded from the reference's own classes in float64 (tools/make_act_golden.py): the output, the
  gradient of x and of every parameter, and the running statistics after the step, 1e-4 relative to each tensor's max (the project's
  bound for module fixtures); eval mode, and ``fuse()`` then eval, run and leave the state alone;
* bf16 mode against the same fixtures: per fixture and kind (output / gradients / running statistics) the bound is FLOOR_FACTOR times
  the bf16 floor the fixture records (the project's factor);
* a small yaml model under ``activation: nn.Mish()`` with one AconC and one FReLU Conv swapped in takes a full eager training step in
  bf16 and in f32 at a 32^2 input, every parameter touched and moved, p1 / p2 / beta included;
* in deterministic f32 mode five steps replayed from the launch list leave the same losses and state as the eager steps, bit for bit;
* the recorded launch list of the headline model (the step tests/test_gpu_replay.py records) names none of the new entry points."""
import os

import pytest
import torch

from tests.block_harness import (check_bf16_against_floor, check_f32_fixture, check_replay_equals_eager, eager_step_checks, rel_max_err,
                                 train_setup)
from tests.test_builders_act_cpu import FILES, YAML, build

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 4.0
NEW_ENTRIES = ("ydl_bn_act_fwd_p", "ydl_bn_act_bwd_p", "ydl_bn_act_fwd_sums_p", "ydl_bn_act_bwd_sums_p", "ydl_bn_act_bwd_apply_sums_p",
               "ydl_bn_act_bwd_reduce_sums_p", "ydl_acon_fwd", "ydl_acon_bwd", "ydl_max2_fwd", "ydl_max2_bwd")


def _fuse_then_eval(mod, x, out, out_eval):
    """fuse(): every dense Conv folds its own BatchNorm; AconC / FReLU run behind the folded conv, FReLU's inner BatchNorm stays"""
    import yolo_dual_amd as ydl
    fused = 0
    for m in mod.modules():
        if isinstance(m, ydl.Conv) and not m.depthwise:
            m.fuse()
            fused += 1
    if fused:
        with torch.no_grad():
            out_fused = mod(x.detach())
        torch.cuda.synchronize()
        assert rel_max_err(out_fused, out_eval.cpu()) < 1e-4


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_modules_match_the_reference_fixtures(path):
    check_f32_fixture(path, build, after_eval=_fuse_then_eval)


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_bf16_mode_against_the_fixtures(path):
    check_bf16_against_floor(path, build, FLOOR_FACTOR, ("out", "grad", "run"), "act")


def _swap_in_acon_and_frelu(m):
    import yolo_dual_amd as ydl
    with ydl.default_activation("nn.Mish()"):
        down = ydl.Conv(16, 32, 3, 2, act=ydl.AconC(32))                    # the down-sampler, under AconC
        down.i, down.f, down.type, down.np = m.model[1].i, m.model[1].f, m.model[1].type, m.model[1].np
        m.model[1] = down
        m.model[2].cv3 = ydl.Conv(32, 32, 1, 1, act=ydl.FReLU(32))          # the C3's output convolution, under FReLU


def _setup(mode):
    return train_setup(dict(YAML, activation="nn.Mish()"), mode, 8, patch=_swap_in_acon_and_frelu)


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_yaml_model_takes_a_full_eager_step(mode):
    import yolo_dual_amd as ydl
    try:
        m, opt, crit, xs, ts = _setup(mode)
        assert sum(isinstance(c.act, torch.nn.Mish) for c in m.modules() if isinstance(c, ydl.Conv)) == 8
        params, before, after = eager_step_checks(m, opt, crit, xs, ts, (2, 12, 8, 8))
        for k in ("model.1.act.p1", "model.1.act.p2", "model.1.act.beta", "model.2.cv3.act.conv.weight", "model.2.cv3.act.bn.weight"):
            assert k in params, k
        for k in params:                                   # the fused optimizer step moved every parameter
            assert not torch.equal(before[k], after[k]), k
    finally:
        ydl.set_compute_dtype("bf16")


def test_replayed_step_equals_the_eager_step_bit_for_bit():
    check_replay_equals_eager(_setup, "act", NEW_ENTRIES)


class _Names:
    """recorder for ``_lib.set_recorder``: the names of the entry points a step calls"""

    def __init__(self):
        self.names = []

    def add(self, name, args):
        self.names.append(name)

    def edge(self, src, dst):
        pass


def test_the_headline_model_launches_no_new_entry_point():
    import yolo_dual_amd as ydl
    from yolo_dual_amd import _lib as L
    from tests.test_gpu_replay import _setup as headline
    try:
        m, opt, crit, xs, ts = headline("bf16")
        for _ in range(2):
            opt.zero_grad()
            crit(m(xs[0]), ts[0])[0].backward()
            opt.step()
        rec = _Names()
        L.set_recorder(rec)
        try:
            opt.zero_grad()
            crit(m(xs[1]), ts[1])[0].backward()
        finally:
            L.set_recorder(None)
        torch.cuda.synchronize()
        assert len(rec.names) > 50 and any(n.startswith("ydl_bn_act_") for n in rec.names)
        assert not set(rec.names) & set(NEW_ENTRIES), sorted(set(rec.names) & set(NEW_ENTRIES))
    finally:
        ydl.set_compute_dtype("bf16")
