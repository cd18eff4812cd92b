"""GPU: the squeeze-excitation modules at module level -- ``SqueezeExcitation`` (pool, the one-launch excitation, the gated product and
their backward), ``InvertedResidual`` and ``MBConv`` on it, and the six backbone rows.  The scaffold is tests/block_harness.py.
* f32 mode against the six fixtures of tools/make_se_golden.py (plain torch in float64, tests/se_ref.py): the output, the gradient of x
  and of every parameter and the running statistics within 1e-4 of each tensor's max;
* bf16 mode against the same fixtures: the bound is FLOOR_FACTOR = 4 times the bf16 floor the fixture records, the reference's own
  error under bf16 storage.  4 is the family factor in use since the space / depth layers, with its reasoning: the kernels sum in
  another order and round at other points, and single draws on small tensors scatter by a small multiple.  The measured worst ratios
  are in DESIGN.md, "Squeeze-excitation blocks";
* ``MobileNetV3s1`` and ``efficientnet_b01`` on 2 x 3 x 32 x 32 with seeded weights against the reference computed at test time, f32;
* each yaml's three rows + SPPF + a short 12-class head take a full eager training step in bf16 and f32 with every parameter touched,
  and at stochastic_depth_prob = 0 five replayed steps equal the eager ones bit for bit with the new entry points in the replay table;
  a recorded step with stochastic depth is refused by name;
* an MBConv sample with keep 0 equals its input bit for bit."""
import os

import numpy as np
import pytest
import torch

from tests import se_ref as R
from tests.block_harness import (F32_TOL, check_bf16_against_floor, check_f32_fixture, check_replay_equals_eager, eager_step_checks,
                                 rel_max_err, train_setup)
from tests.test_builders_se_cpu import FILES, YAML_EFF, YAML_MNV3, build

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 4.0
IDS = [os.path.basename(f)[:-4] for f in FILES]
ENTRIES = ("ydl_se_pool_fwd", "ydl_se_excite_fwd", "ydl_se_excite_bwd", "ydl_se_scale_bwd")
YAMLS = {"mobilenet_v3_small": YAML_MNV3, "efficientnet_b0": YAML_EFF}


def _has_bn(path):
    return "gate" not in os.path.basename(path)


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_modules_match_the_fixtures(path):
    check_f32_fixture(path, build, expect_running_stats=_has_bn(path))


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_bf16_mode_against_the_fixtures(path):
    check_bf16_against_floor(path, build, FLOOR_FACTOR, ("out", "grad", "run") if _has_bn(path) else ("out", "grad"), "se")


def _seeded(mod, seed):
    """weights ~ N(0, 1/fan_in) (SE weights twice that), BatchNorm weights uniform in [0.5, 1.5], biases ~ N(0, 0.3^2) (fc2: N(0, 1)),
    through f32"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if k.endswith("weight") and p.dim() == 1:
                v = torch.rand(p.shape, generator=gen, dtype=torch.float64) + 0.5
            elif k.endswith("bias"):
                v = torch.randn(p.shape, generator=gen, dtype=torch.float64) * (1.0 if k.endswith("fc2.bias") else 0.3)
            else:
                v = torch.randn(p.shape, generator=gen, dtype=torch.float64) * p[0].numel() ** -0.5 * (2.0 if ".fc" in k else 1.0)
            p.copy_(v.float())
    return mod


def _grad_scale(g_r, k):
    """the harness's rule for a BatchNorm bias in front of a linear layer and another train-mode BatchNorm (block_harness.
    zero_bias_scale, here under torchvision's names): the projection's ``1.bias`` feeds the next block's 1x1 convolution and its
    BatchNorm, so its exact gradient is zero and float64 leaves round-off with no scale of its own.  Where the reference's gradient is
    below 1e-6 of the same BatchNorm's weight gradient (a sum over the same dz), that weight gradient's max is the scale."""
    if not k.endswith(".1.bias"):
        return None
    gw = float(g_r[k[:-4] + "weight"].abs().max())
    return gw if float(g_r[k].abs().max()) < 1e-6 * gw else None


def _step(mod, x, gout):
    x = x.clone().requires_grad_(True)
    out = mod(x)
    out.backward(gout)
    return out.detach(), x.grad, {k: p.grad for k, p in mod.named_parameters()}


@pytest.mark.parametrize("name,cout", [("MobileNetV3s1", 24), ("efficientnet_b01", 40)])
def test_first_rows_match_the_reference_computed_here(name, cout):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    try:
        kw = {} if name == "MobileNetV3s1" else {"stochastic_depth_prob": 0.0}
        ref = _seeded(getattr(R, name)(**kw), 7).double().train()
        mod = getattr(ydl, name)(cout, **kw)
        mod.load_state_dict({k: v.float() if v.dtype.is_floating_point else v for k, v in ref.state_dict().items()})
        mod = mod.cuda().train()
        gen = torch.Generator().manual_seed(8)
        x = torch.randn(2, 3, 32, 32, generator=gen, dtype=torch.float64).float()
        gout = torch.randn(2, cout, 4, 4, generator=gen, dtype=torch.float64).float()
        out_r, gx_r, g_r = _step(ref, x.double(), gout.double())
        out, gx, g = _step(mod, x.cuda(), gout.cuda())
        torch.cuda.synchronize()
        assert out.shape == (2, cout, 4, 4)
        errs = {"out": rel_max_err(out, out_r), "grad_x": rel_max_err(gx, gx_r)}
        errs.update(("g." + k, rel_max_err(g[k], g_r[k], _grad_scale(g_r, k))) for k in g_r)
        sd, sd_r = mod.state_dict(), ref.state_dict()
        errs.update(("run." + k, rel_max_err(sd[k], sd_r[k])) for k in sd_r if k.endswith(("running_mean", "running_var")))
        worst = max(errs.items(), key=lambda e: e[1])
        print(f"[se] {name} f32: out", f"{errs['out']:.1e}", "grad_x", f"{errs['grad_x']:.1e}", "worst", worst)
        assert all(v < F32_TOL for v in errs.values()), {k: v for k, v in errs.items() if not v < F32_TOL}
    finally:
        ydl.set_compute_dtype("bf16")


def _no_sd(m):
    for sub in m.modules():
        if type(sub).__name__ == "MBConv":
            sub.stochastic_depth_prob = 0.0


def _setup(family, mode, patch=None):
    return train_setup(YAMLS[family], mode, 2, patch)


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("family", sorted(YAMLS))
def test_yaml_model_takes_a_full_eager_step(family, mode):
    import yolo_dual_amd as ydl
    try:
        m, opt, crit, xs, ts = _setup(family, mode)                # EfficientNet: stochastic depth at the rows' default 0.2
        params, before, after = eager_step_checks(m, opt, crit, xs, ts, (2, 12, 2, 2))
        se = [s for s in m.modules() if type(s).__name__ == "SqueezeExcitation"]
        assert len(se) == (9 if family == "mobilenet_v3_small" else 16)
        names = {id(p): k for k, p in params.items()}
        for s in (se[0], se[-1]):
            for p in (s.fc1.weight, s.fc1.bias, s.fc2.weight, s.fc2.bias):              # in the flat arenas, and moved by the step
                assert opt.params_arena.data_ptr() <= p.data_ptr() < opt.params_arena.data_ptr() + opt.params_arena.numel() * 4
                assert opt.grads_arena.data_ptr() <= p.grad.data_ptr() < opt.grads_arena.data_ptr() + opt.grads_arena.numel() * 4
                assert not torch.equal(before[names[id(p)]], after[names[id(p)]]), names[id(p)]
    finally:
        ydl.set_compute_dtype("bf16")


@pytest.mark.parametrize("family", sorted(YAMLS))
def test_replayed_step_equals_the_eager_step_bit_for_bit(family):
    check_replay_equals_eager(lambda mode: _setup(family, mode, _no_sd), "se " + family, ENTRIES)


def test_a_recorded_step_with_stochastic_depth_is_refused():
    import yolo_dual_amd as ydl
    from yolo_dual_amd.replay import ReplayedTrainStep
    try:
        m, opt, crit, xs, ts = _setup("efficientnet_b0", "f32")
        with pytest.raises(NotImplementedError, match="stochastic depth.*MBConv"):
            ReplayedTrainStep(m, crit, opt, xs[0], ts[0], warmup=1)
    finally:
        ydl.set_compute_dtype("bf16")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_an_mbconv_sample_with_keep_zero_equals_its_input(mode):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype(mode)
    try:
        mod = _seeded(ydl.MBConv(6, 3, 1, 24, 24, 0.5), 9).cuda().train()
        mod.generator = torch.Generator("cuda").manual_seed(10)
        twin = torch.Generator("cuda").manual_seed(10)
        keep = torch.empty(8, device="cuda").bernoulli_(0.5, generator=twin) / 0.5
        assert 0 < int((keep == 0).sum()) < 8
        x = torch.randn(8, 24, 6, 10, device="cuda")
        if mode == "bf16":
            x = x.bfloat16().float()                                # values the bf16 path stores exactly
        x.requires_grad_(True)
        out = mod(x)
        out.backward(torch.randn_like(out))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x.grad).all())
        for k, p in mod.named_parameters():
            assert getattr(p, "_ydl_touched", False) and p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        for n in range(8):
            assert torch.equal(out[n].detach(), x[n].detach()) == (float(keep[n]) == 0.0), n
        mod.eval()
        with torch.no_grad():
            i = int((keep == 0).nonzero()[0])
            assert not torch.equal(mod(x.detach())[i], x.detach()[i])
    finally:
        ydl.set_compute_dtype("bf16")
