"""GPU: the TransformerLayer / TransformerBlock / C3TR modules (the pattern of tests/test_gpu_attention_blocks.py).
* f32 mode against the fixtures recorded from the reference's own classes (tools/make_transformer_golden.py): the output, the
  gradient of x and of every parameter, 1e-4 relative to each tensor's max (a gradient that is analytically zero, out_proj.bias in
  front of C3TR's train-mode BatchNorm, absolutely);
* the eval-mode forward equals the train-mode forward for the fixtures without BatchNorm;
* the small yaml model of tests/test_builders_transformer_cpu.py takes a full eager training step in bf16 and in f32;
* in deterministic f32 mode the step replayed from the launch list leaves the same losses and the same state as the eager step, bit
  for bit (the pattern of tests/test_gpu_replay.py)."""
import glob
import os

import numpy as np
import pytest
import torch

from tests.test_builders_transformer_cpu import YAML

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "tr_*.npz")))


def _err(got, want):
    want = torch.as_tensor(want)
    scale = float(want.abs().max())             # an analytically zero gradient (1e-14 of rounding noise in the fixture): absolute error
    return float((got.detach().double().cpu() - want).abs().max()) / (scale if scale > 1e-10 else 1.0)


def _module(z):
    import yolo_dual_amd as ydl
    mod = getattr(ydl, str(z["cls"]))(*(int(a) for a in z["args"]))
    mod.load_state_dict({str(k): torch.from_numpy(z["p." + str(k)]) for k in z["keys"]})
    return mod.cuda().train()


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_modules_match_the_reference_fixtures(path):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    try:
        z = np.load(path)
        mod = _module(z)
        x = torch.from_numpy(z["x"]).float().cuda().requires_grad_(True)
        out = mod(x)
        out.backward(torch.from_numpy(z["grad_out"]).float().cuda())
        torch.cuda.synchronize()
        errs = {"out": _err(out, z["out"]), "grad_x": _err(x.grad, z["grad_x"])}
        for k, p in mod.named_parameters():
            assert p.grad is not None, k
            errs["g." + k] = _err(p.grad, z["g." + k])
        print(os.path.basename(path), {k: f"{v:.1e}" for k, v in errs.items()})
        assert all(v < 1e-4 for v in errs.values()), errs
        if not any("running_mean" in str(k) for k in z["keys"]):
            # eval mode: the same forward, nothing recorded
            mod.eval()
            with torch.no_grad():
                out_eval = mod(x.detach())
            assert torch.equal(out_eval, out.detach())
    finally:
        ydl.set_compute_dtype("bf16")


def _setup(mode):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype(mode)
    torch.manual_seed(11)
    m = ydl.SegYoloModel(YAML).cuda().train()
    opt = ydl.smart_optimizer(m, "SGD", lr=0.01, momentum=0.937, decay=5e-4)
    crit = ydl.SegmentationLoss(12, 0.0, torch.ones(12), "dice", sync=False)
    gen = torch.Generator("cuda").manual_seed(3)
    xs = [torch.rand(2, 3, 32, 32, device="cuda", generator=gen) for _ in range(2)]
    ts = [torch.randint(0, 12, (2, 16, 16), device="cuda", generator=gen) for _ in range(2)]
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
        assert out.shape == (2, 12, 16, 16)
        total, items = crit(out, ts[0])
        total.backward()
        blk = m.model[1].m
        params = dict(m.named_parameters())
        assert all(getattr(p, "_ydl_touched", False) for p in params.values()), [k for k, p in params.items() if not p._ydl_touched]
        opt.step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(total)) and bool(torch.isfinite(opt.params_arena).all())
        after = _state(m, opt)
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
                losses = [None, None, float(r.loss_items[0])]
                r.poison()
                for st in range(3, 5):
                    x.copy_(xs[st % 2]); t.copy_(ts[st % 2])
                    losses.append(float(r.step()[0]))
            torch.cuda.synchronize()
            res[how] = (losses, _state(m, opt))
        le, lr_ = res["eager"][0], res["replay"][0]
        print("[transformer replay] losses", le, lr_)
        assert le[2:] == lr_[2:], (le, lr_)
        for k, v in res["eager"][1].items():
            assert torch.equal(v, res["replay"][1][k]), k
    finally:
        config.set_deterministic(None)
        ydl.set_compute_dtype("bf16")
