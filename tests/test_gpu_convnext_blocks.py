"""GPU: the ConvNeXt modules at module level -- ``CNBlock`` (depth-wise 7x7, LayerNorm with the convolution's bias, the fc1 GEMM, bias +
erf GELU, the fc2 GEMM, the layer-scaled residual with keep factors), the stem and a down-sampling layer (patchify convolution +
``LayerNorm2d`` either way round), and the three rows.  The scaffold is tests/block_harness.py.
* f32 mode against the four fixtures of tools/make_convnext_golden.py (plain torch in float64, tests/convnext_ref.py): the output, the
  gradient of x and of every parameter within 1e-4 of each tensor's max.  All of them carry layer_scale of order 1; one more case runs
  at the initial 1e-6, where the branch does not show in the output, and checks ``layer_scale.grad`` alone, which does not vanish;
* bf16 mode against the same fixtures: the bound is FLOOR_FACTOR = 4 times the bf16 floor the fixture records, the reference's own
  error under bf16 storage.  4 is the factor of the newest merged family (the space / depth layers) with its reasoning: the kernels
  sum in another order and round at other points, and single draws on small tensors scatter by a small multiple.
  Measured on an MI355X (worst error / floor): cnblock_16 out 1.00 grad 1.00, cnblock_24_keep out 1.07 grad 1.00, down_16_32
  out 1.38 grad 1.00, stem_3_16 out 1.22 grad 1.00 -- the reference rounds where these kernels store, so the two nearly coincide;
  the factor stays at the family's 4;
* ``convnext_tiny1`` on 2 x 3 x 32 x 32 with seeded weights (layer_scale of order 1) against the reference computed at test time, f32:
  1e-4;
* the three rows + SPPF + a short head ending in a 12-channel 1x1 take a full eager training step in bf16 and f32 with every parameter
  touched, and at stochastic_depth_prob = 0 five replayed steps equal the eager ones bit for bit with the six new entry points in the
  replay table; a recorded step with stochastic depth is refused by name;
* one eager step of a CNBlock at p = 0.5 with a seeded generator: finite, every parameter touched, a dropped sample's output equal to
  its input."""
import os

import numpy as np
import pytest
import torch

from tests import convnext_ref as R
from tests.block_harness import (F32_TOL, check_bf16_against_floor, check_f32_fixture, check_replay_equals_eager, eager_step_checks,
                                 rel_max_err, train_setup)
from tests.test_builders_convnext_cpu import FILES, YAML, build

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 4.0
IDS = [os.path.basename(f)[:-4] for f in FILES]
ENTRIES = ("ydl_ln_fwd", "ydl_ln_bwd", "ydl_bias_gelu_fwd", "ydl_bias_gelu_bwd", "ydl_scale_res_fwd", "ydl_scale_res_bwd")


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_modules_match_the_fixtures(path):
    def after_eval(mod, x, out, out_eval):
        if "keep" not in np.load(path).files:          # no stochastic depth: eval computes what the train-mode step did
            assert rel_max_err(out_eval, out.detach().cpu()) < 1e-6
    check_f32_fixture(path, build, expect_running_stats=False, after_eval=after_eval)


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_bf16_mode_against_the_fixtures(path):
    check_bf16_against_floor(path, build, FLOOR_FACTOR, ("out", "grad"), "convnext")


def _seeded(mod, seed):
    """weights ~ N(0, 1/fan_in), LayerNorm weights and layer_scale uniform in [0.5, 1.5], biases uniform in [-0.3, 0.3], through f32"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if k.endswith("layer_scale") or (k.endswith("weight") and p.dim() == 1):
                v = torch.rand(p.shape, generator=gen, dtype=torch.float64) + 0.5
            elif k.endswith("bias"):
                v = torch.rand(p.shape, generator=gen, dtype=torch.float64) * 0.6 - 0.3
            else:
                v = torch.randn(p.shape, generator=gen, dtype=torch.float64) * p[0].numel() ** -0.5
            p.copy_(v.float())
    return mod


def _step(mod, x, gout):
    x = x.clone().requires_grad_(True)
    out = mod(x)
    out.backward(gout)
    return out.detach(), x.grad, {k: p.grad for k, p in mod.named_parameters()}


def test_layer_scale_gradient_at_the_initial_value():
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    try:
        ref = _seeded(R.CNBlock(16), 5).double().train()
        with torch.no_grad():
            ref.layer_scale.fill_(1e-6)
        mod = ydl.CNBlock(16)
        mod.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
        mod = mod.cuda().train()
        gen = torch.Generator().manual_seed(6)
        x, gout = (torch.randn(2, 16, 6, 10, generator=gen, dtype=torch.float64).float() for _ in range(2))
        _o, _gx, want = _step(ref, x.double(), gout.double())
        _o2, _gx2, got = _step(mod, x.cuda(), gout.cuda())
        torch.cuda.synchronize()
        assert float(want["layer_scale"].abs().max()) > 1e-2                  # of order 1 although the branch is scaled by 1e-6
        err = rel_max_err(got["layer_scale"], want["layer_scale"])
        print("[convnext] layer_scale.grad at 1e-6:", f"{err:.1e}")
        assert err < F32_TOL
    finally:
        ydl.set_compute_dtype("bf16")


def test_convnext_tiny1_matches_the_reference_computed_here():
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    try:
        ref = _seeded(R.convnext_tiny1(stochastic_depth_prob=0.0), 7).double().train()
        mod = ydl.convnext_tiny1(192, stochastic_depth_prob=0.0)
        mod.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
        mod = mod.cuda().train()
        gen = torch.Generator().manual_seed(8)
        x = torch.randn(2, 3, 32, 32, generator=gen, dtype=torch.float64).float()
        gout = torch.randn(2, 192, 4, 4, generator=gen, dtype=torch.float64).float()
        out_r, gx_r, g_r = _step(ref, x.double(), gout.double())
        out, gx, g = _step(mod, x.cuda(), gout.cuda())
        torch.cuda.synchronize()
        assert out.shape == (2, 192, 4, 4)
        errs = {"out": rel_max_err(out, out_r), "grad_x": rel_max_err(gx, gx_r)}
        errs.update(("g." + k, rel_max_err(g[k], g_r[k])) for k in g_r)
        worst = max(errs.items(), key=lambda e: e[1])
        print("[convnext] convnext_tiny1 f32: out", f"{errs['out']:.1e}", "grad_x", f"{errs['grad_x']:.1e}", "worst", worst)
        assert all(v < F32_TOL for v in errs.values()), {k: v for k, v in errs.items() if not v < F32_TOL}
    finally:
        ydl.set_compute_dtype("bf16")


def _no_sd(m):
    for sub in m.modules():
        if type(sub).__name__ == "CNBlock":
            sub.stochastic_depth_prob = 0.0


def _setup(mode, patch=None):
    return train_setup(YAML, mode, 2, patch)


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_yaml_model_takes_a_full_eager_step(mode):
    import yolo_dual_amd as ydl
    try:
        m, opt, crit, xs, ts = _setup(mode)                       # stochastic depth at the rows' default 0.1
        params, before, after = eager_step_checks(m, opt, crit, xs, ts, (2, 12, 2, 2))
        for k in ("model.0.model.0.0.weight", "model.1.model.1.4.block.3.weight", "model.2.model.1.2.block.2.bias"):
            assert not torch.equal(before[k], after[k]), k
        blk = m.model[1].model[1][0]
        for p in (blk.layer_scale, blk.block[0].bias, blk.block[2].weight, m.model[0].model[0][0].weight):      # in the flat arenas
            assert opt.params_arena.data_ptr() <= p.data_ptr() < opt.params_arena.data_ptr() + opt.params_arena.numel() * 4
            assert opt.grads_arena.data_ptr() <= p.grad.data_ptr() < opt.grads_arena.data_ptr() + opt.grads_arena.numel() * 4
    finally:
        ydl.set_compute_dtype("bf16")


def test_replayed_step_equals_the_eager_step_bit_for_bit():
    check_replay_equals_eager(lambda mode: _setup(mode, _no_sd), "convnext", ENTRIES)


def test_a_recorded_step_with_stochastic_depth_is_refused():
    import yolo_dual_amd as ydl
    from yolo_dual_amd.replay import ReplayedTrainStep
    try:
        m, opt, crit, xs, ts = _setup("f32")
        with pytest.raises(NotImplementedError, match="stochastic depth"):
            ReplayedTrainStep(m, crit, opt, xs[0], ts[0], warmup=1)
    finally:
        ydl.set_compute_dtype("bf16")


def test_an_eager_step_with_stochastic_depth_drops_whole_samples():
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    try:
        mod = _seeded(ydl.CNBlock(16, 1.0, 0.5), 9).cuda().train()
        mod.generator = torch.Generator("cuda").manual_seed(10)
        twin = torch.Generator("cuda").manual_seed(10)
        keep = torch.empty(8, device="cuda").bernoulli_(0.5, generator=twin) / 0.5
        assert 0 < int((keep == 0).sum()) < 8
        x = torch.randn(8, 16, 6, 10, device="cuda", requires_grad=True)
        out = mod(x)
        out.backward(torch.randn_like(out))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x.grad).all())
        for k, p in mod.named_parameters():
            assert getattr(p, "_ydl_touched", False) and p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        for n in range(8):
            same = torch.equal(out[n].detach(), x[n].detach())
            assert same == (float(keep[n]) == 0.0), n
        mod.eval()
        with torch.no_grad():
            assert not torch.equal(mod(x.detach())[int((keep == 0).nonzero()[0])], x.detach()[int((keep == 0).nonzero()[0])])
    finally:
        ydl.set_compute_dtype("bf16")
