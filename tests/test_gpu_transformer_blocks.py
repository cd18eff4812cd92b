"""GPU: the TransformerLayer / TransformerBlock / C3TR modules (the scaffold is tests/block_harness.py).
* f32 mode against the fixtures recorded from the reference's own classes (tools/make_transformer_golden.py): the output, the
  gradient of x and of every parameter, 1e-4 relative to each tensor's max (a gradient that is analytically zero, out_proj.bias in
  front of C3TR's train-mode BatchNorm, absolutely);
* the eval-mode forward equals the train-mode forward for the fixtures without BatchNorm;
* the small yaml model of tests/test_builders_transformer_cpu.py takes a full eager training step in bf16 and in f32;
* in deterministic f32 mode the step replayed from the launch list leaves the same losses and the same state as the eager step, bit
  for bit (tests/block_harness.py)."""
import glob
import os

import numpy as np
import pytest
import torch

from tests.block_harness import F32_TOL, check_replay_equals_eager, eager_step_checks, load_module, rel_max_err, train_setup
from tests.test_builders_transformer_cpu import YAML

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "tr_*.npz")))


def _err(got, want):
    """an analytically zero gradient (1e-14 of rounding noise in the fixture) is measured absolutely"""
    scale = float(np.abs(want).max())
    return rel_max_err(got, want, scale if scale > 1e-10 else 1.0)


def build(z):
    import yolo_dual_amd as ydl
    return getattr(ydl, str(z["cls"]))(*(int(a) for a in z["args"]))


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_modules_match_the_reference_fixtures(path):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    try:
        z = np.load(path)
        mod = load_module(z, build)
        x = torch.from_numpy(z["x"]).float().cuda().requires_grad_(True)
        out = mod(x)
        out.backward(torch.from_numpy(z["grad_out"]).float().cuda())
        torch.cuda.synchronize()
        errs = {"out": _err(out, z["out"]), "grad_x": _err(x.grad, z["grad_x"])}
        for k, p in mod.named_parameters():
            assert p.grad is not None, k
            errs["g." + k] = _err(p.grad, z["g." + k])
        print(os.path.basename(path), {k: f"{v:.1e}" for k, v in errs.items()})
        assert all(v < F32_TOL for v in errs.values()), errs
        if not any("running_mean" in str(k) for k in z["keys"]):
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
        blk = m.model[1].m
        # the fused optimizer step moved every new parameter
        names = ("linear.bias", "tr.0.q.weight", "tr.0.ma.in_proj_weight", "tr.0.ma.in_proj_bias", "tr.0.ma.out_proj.bias", "tr.0.fc2.weight")
        lo, hi = opt.grads_arena.data_ptr(), opt.grads_arena.data_ptr() + 4 * opt.grads_arena.numel()
        for k in names:
            assert not torch.equal(before["model.1.m." + k], after["model.1.m." + k]), k
            g = blk.get_parameter(k).grad
            assert lo <= g.data_ptr() and g.data_ptr() + 4 * g.numel() <= hi, k
    finally:
        ydl.set_compute_dtype("bf16")


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_every_parameter_is_reported_once_per_step_after_its_last_writer(mode):
    """``config.mark_touched`` is what the data-parallel reducer counts down on (parallel.GradReducer._on_grad): a parameter whose
    gradient is written by several launches (the three row blocks of ``ma.in_proj_weight`` / ``ma.in_proj_bias``) must be reported
    exactly once, and only when the whole gradient is there"""
    import yolo_dual_amd as ydl
    from yolo_dual_amd import config
    try:
        m, opt, crit, xs, ts = _setup(mode)
        names = {id(p): k for k, p in m.named_parameters()}
        seen, at_hook = [], {}
        t0 = m.model[1].m.tr[0]
        watched = {id(t0.ma.in_proj_weight), id(t0.ma.in_proj_bias)}

        def hook(p):
            seen.append(names[id(p)])
            if id(p) in watched:        # what the gradient holds when the hook fires: nothing may write it afterwards
                torch.cuda.synchronize()
                at_hook[names[id(p)]] = p.grad.detach().clone()
        config.add_grad_hook(hook)
        try:
            for step in range(2):
                del seen[:]
                at_hook.clear()
                opt.zero_grad()
                total, _items = crit(m(xs[step]), ts[step])
                total.backward()
                torch.cuda.synchronize()
                assert sorted(seen) == sorted(names.values()), sorted(set(k for k in seen if seen.count(k) != 1) | (set(names.values()) - set(seen)))
                for k, p in (("model.1.m.tr.0.ma.in_proj_weight", t0.ma.in_proj_weight), ("model.1.m.tr.0.ma.in_proj_bias", t0.ma.in_proj_bias)):
                    assert torch.equal(at_hook[k], p.grad), k
                    c = p.shape[0] // 3
                    assert all(bool(p.grad[i * c:(i + 1) * c].abs().max() > 0) for i in (0, 2)), k       # Q and V blocks were written
                opt.step()
        finally:
            config.remove_grad_hook(hook)
    finally:
        ydl.set_compute_dtype("bf16")


def test_replayed_step_equals_the_eager_step_bit_for_bit():
    check_replay_equals_eager(_setup, "transformer")
