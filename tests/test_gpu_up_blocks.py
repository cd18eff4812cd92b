"""GPU: the decoder up-samplers at module level — ``ConvTranspose2d`` through Tape.conv_transpose (the implicit-GEMM entry points on the
mirrored geometry), ``DWConvTranspose2d`` through Tape.dw_conv_transpose (csrc/tconv.hip) and ``Upsample(mode='bicubic')`` through
Tape.resize (ydl_bicubic_fwd / ydl_bicubic_bwd).  The pattern of tests/test_gpu_cross_blocks.py.
* f32 mode against the seven fixtures of tools/make_up_golden.py (torch / the reference's own DWConvTranspose2d in float64): the output,
  the gradient of x and of every parameter, 1e-4 relative to each tensor's max (the project's bound for module fixtures);
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

import numpy as np
import pytest
import torch

from tests.test_builders_up_cpu import FILES, YAML, build

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 4.0


def _err(got, want):
    want = torch.as_tensor(want).double()
    scale = float(want.abs().max())
    return float((got.detach().double().cpu() - want).abs().max()) / (scale if scale > 0 else 1.0)


def _step(z):
    """one train-mode forward + backward of the fixture's module -> errors by tensor"""
    mod = build(z)
    sd = mod.state_dict()
    mod.load_state_dict({str(k): torch.from_numpy(z["p." + str(k)]).to(sd[str(k)].dtype) for k in z["keys"]})
    mod = mod.cuda().train()
    x = torch.from_numpy(z["x"]).float().cuda().requires_grad_(True)
    out = mod(x)
    assert tuple(out.shape) == tuple(z["out"].shape)
    out.backward(torch.from_numpy(z["grad_out"]).float().cuda())
    torch.cuda.synchronize()
    errs = {"out": _err(out, z["out"]), "grad_x": _err(x.grad, z["grad_x"])}
    for k, p in mod.named_parameters():
        assert p.grad is not None, k
        errs["g." + k] = _err(p.grad, z["g." + k])
    return errs


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_modules_match_the_fixtures(path):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    try:
        errs = _step(np.load(path))
        print(os.path.basename(path), {k: f"{v:.1e}" for k, v in errs.items()})
        assert all(v < 1e-4 for v in errs.values()), {k: v for k, v in errs.items() if not v < 1e-4}
    finally:
        ydl.set_compute_dtype("bf16")


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_bf16_mode_against_the_fixtures(path):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("bf16")
    z = np.load(path)
    name = os.path.basename(path)[:-4]
    floor = {k: float(z["floor." + k]) for k in ("out", "grad")}
    errs = _step(z)
    kind = lambda k: "out" if k == "out" else "grad"
    worst = {"out": (0.0, ""), "grad": (0.0, "")}
    for k, v in errs.items():
        worst[kind(k)] = max(worst[kind(k)], (v, k))
    print("[up bf16]", name, {k: f"{v:.2e} ({w}) floor {floor[k]:.2e} ratio {v / floor[k]:.2f}" for k, (v, w) in worst.items()})
    bad = {k: (v, FLOOR_FACTOR * floor[kind(k)]) for k, v in errs.items() if not v < FLOOR_FACTOR * floor[kind(k)]}
    assert not bad, bad


def _setup(mode):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype(mode)
    torch.manual_seed(11)
    m = ydl.SegYoloModel(YAML).cuda().train()
    opt = ydl.smart_optimizer(m, "SGD", lr=0.01, momentum=0.937, decay=5e-4)
    crit = ydl.SegmentationLoss(12, 0.0, torch.ones(12), "dice", sync=False)
    gen = torch.Generator("cuda").manual_seed(3)
    xs = [torch.rand(2, 3, 32, 32, device="cuda", generator=gen) for _ in range(2)]
    ts = [torch.randint(0, 12, (2, 32, 32), device="cuda", generator=gen) for _ in range(2)]
    return m, opt, crit, xs, ts


def _state(m, opt):
    out = {k: v.detach().clone() for k, v in m.state_dict().items()}
    out["__momentum"] = opt.mom_arena.detach().clone()
    out["__ema"] = opt.ema_arena.detach().clone()
    return out


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_yaml_model_takes_a_full_eager_step(mode):
    import yolo_dual_amd as ydl
    try:
        m, opt, crit, xs, ts = _setup(mode)
        before = _state(m, opt)
        opt.zero_grad()
        out = m(xs[0])
        assert out.shape == (2, 12, 32, 32)
        total, items = crit(out, ts[0])
        total.backward()
        params = dict(m.named_parameters())
        assert all(getattr(p, "_ydl_touched", False) for p in params.values()), [k for k, p in params.items() if not p._ydl_touched]
        opt.step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(total)) and bool(torch.isfinite(opt.params_arena).all())
        after = _state(m, opt)
        for k in params:                                   # the fused optimizer step moved every parameter
            assert not torch.equal(before[k], after[k]), k
        for w in (m.model[4].weight, m.model[6].weight):
            assert w.data_ptr() >= opt.params_arena.data_ptr() and w.grad.data_ptr() >= opt.grads_arena.data_ptr()
            assert w.permute(0, 2, 3, 1).is_contiguous() and w.grad.permute(0, 2, 3, 1).is_contiguous()
    finally:
        ydl.set_compute_dtype("bf16")


def test_replayed_step_equals_the_eager_step_bit_for_bit():
    import yolo_dual_amd as ydl
    from yolo_dual_amd import config
    from yolo_dual_amd.replay import ReplayedTrainStep
    config.set_deterministic(True)
    try:
        res = {}
        for how in ("eager", "replay"):
            m, opt, crit, xs, ts = _setup("f32")
            x, t = xs[0].clone(), ts[0].clone()
            losses = []
            if how == "eager":
                for st in range(5):
                    x.copy_(xs[st % 2]); t.copy_(ts[st % 2])
                    opt.zero_grad()
                    total, items = crit(m(x), t)
                    total.backward()
                    opt.step()
                    losses.append(float(items[0]))
            else:
                step_no = [0]

                def pre(_mod, _inp):
                    i = step_no[0]
                    x.copy_(xs[i % 2]); t.copy_(ts[i % 2])
                    step_no[0] += 1
                h = m.register_forward_pre_hook(pre)
                r = ReplayedTrainStep(m, crit, opt, x, t, warmup=2)
                h.remove()
                assert step_no[0] == 3
                for fn in ("ydl_dwtconv_fwd", "ydl_dwtconv_dgrad", "ydl_dwtconv_wgrad", "ydl_bicubic_fwd", "ydl_bicubic_bwd", "ydl_conv_wgrad_det"):
                    assert r.rec.fn.get(fn) is not None, fn
                losses = [None, None, float(r.loss_items[0])]
                r.poison()
                for st in range(3, 5):
                    x.copy_(xs[st % 2]); t.copy_(ts[st % 2])
                    losses.append(float(r.step()[0]))
            torch.cuda.synchronize()
            res[how] = (losses, _state(m, opt))
        le, lr_ = res["eager"][0], res["replay"][0]
        print("[up replay] losses", le, lr_)
        assert le[2:] == lr_[2:], (le, lr_)
        for k, v in res["eager"][1].items():
            assert torch.equal(v, res["replay"][1][k]), k
    finally:
        config.set_deterministic(None)
        ydl.set_compute_dtype("bf16")


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
