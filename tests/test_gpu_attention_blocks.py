"""GPU: the AttentionConv / AttentionStem modules.
* f32 mode against the fixtures recorded from the reference's own classes (tools/make_attn_golden.py): the output, the gradient of x
  and of every parameter, 1e-4 relative to each tensor's max;
* the eval-mode forward equals the train-mode forward;
* the small yaml model of tests/test_builders_attention_cpu.py takes a full eager training step in bf16 and in f32;
* in deterministic f32 mode the step replayed from the launch list leaves the same losses and the same state as the eager step, bit
  for bit (tests/block_harness.py).
(The projections run as separate GEMM launches, so there is no row-concatenated form to compare.)"""
import glob
import os

import numpy as np
import pytest
import torch

from tests.block_harness import F32_TOL, check_replay_equals_eager, eager_step_checks, fixture_step, train_setup
from tests.test_builders_attention_cpu import YAML

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "attn_*.npz")))


def build(z):
    import yolo_dual_amd as ydl
    c1, c2, ks, s, p, g, m = (int(v) for v in z["args"])
    return ydl.AttentionStem(c1, c2, ks, s, p, g, m) if m else ydl.AttentionConv(c1, c2, ks, s, p, g)


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_modules_match_the_reference_fixtures(path):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    try:
        # an all-zero gradient (the mixing table of m = 1 is constant) is measured absolutely
        mod, x, out, errs = fixture_step(np.load(path), build)
        print(os.path.basename(path), {k: f"{v:.1e}" for k, v in errs.items()})
        assert all(v < F32_TOL for v in errs.values()), errs
        # eval mode: the same forward, nothing recorded
        mod.eval()
        with torch.no_grad():
            out_eval = mod(x.detach())
        assert torch.equal(out_eval, out.detach())
    finally:
        ydl.set_compute_dtype("bf16")


def _setup(mode):
    return train_setup(YAML, mode, 16)


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_yaml_model_takes_a_full_eager_step(mode):
    import yolo_dual_amd as ydl
    try:
        m, opt, crit, xs, ts = _setup(mode)
        params, before, after = eager_step_checks(m, opt, crit, xs, ts, (2, 12, 16, 16))
        ac, st = m.model[1], m.model[2]
        # the fused optimizer step moved every new parameter
        for k in ("model.1.rel_h", "model.1.rel_w", "model.1.query_conv.weight", "model.1.key_conv.weight", "model.1.value_conv.weight",
                  "model.2.emb_a", "model.2.emb_b", "model.2.emb_mix", "model.2.query_conv.weight", "model.2.key_conv.weight",
                  "model.2.value_conv.0.weight", "model.2.value_conv.3.weight"):
            assert not torch.equal(before[k], after[k]), k
        assert ac.rel_h.data_ptr() >= opt.params_arena.data_ptr() and st.emb_mix.grad.data_ptr() >= opt.grads_arena.data_ptr()
    finally:
        ydl.set_compute_dtype("bf16")


def test_replayed_step_equals_the_eager_step_bit_for_bit():
    check_replay_equals_eager(_setup, "attention")
