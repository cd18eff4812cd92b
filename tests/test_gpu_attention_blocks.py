"""GPU: the AttentionConv / AttentionStem modules.
* f32 mode against the fixtures recorded from the reference's own classes (tools/make_attn_golden.py): the output, the gradient of x
  and of every parameter, 1e-4 relative to each tensor's max;
* the eval-mode forward equals the train-mode forward;
* the small yaml model of tests/test_builders_attention_cpu.py takes a full eager training step in bf16 and in f32;
* in deterministic f32 mode the step replayed from the launch list leaves the same losses and the same state as the eager step, bit
  for bit (the pattern of tests/test_gpu_replay.py).
(The projections run as separate GEMM launches, so there is no row-concatenated form to compare.)"""
import glob
import os

import numpy as np
import pytest
import torch

from tests.test_builders_attention_cpu import YAML

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "attn_*.npz")))


def _err(got, want):
    want = torch.as_tensor(want)
    scale = float(want.abs().max())             # an all-zero gradient (the mixing table of m = 1 is constant): absolute error
    return float((got.detach().double().cpu() - want).abs().max()) / (scale if scale > 0 else 1.0)


def _module(z):
    import yolo_dual_amd as ydl
    c1, c2, ks, s, p, g, m = (int(v) for v in z["args"])
    mod = ydl.AttentionStem(c1, c2, ks, s, p, g, m) if m else ydl.AttentionConv(c1, c2, ks, s, p, g)
    mod.load_state_dict({str(k): torch.from_numpy(z["p." + str(k)]).float() for k in z["keys"]})
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
        ac, st = m.model[1], m.model[2]
        params = dict(m.named_parameters())
        assert all(getattr(p, "_ydl_touched", False) for p in params.values()), [k for k, p in params.items() if not p._ydl_touched]
        opt.step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(total)) and bool(torch.isfinite(opt.params_arena).all())
        after = _state(m, opt)
        # the fused optimizer step moved every new parameter
        for k in ("model.1.rel_h", "model.1.rel_w", "model.1.query_conv.weight", "model.1.key_conv.weight", "model.1.value_conv.weight",
                  "model.2.emb_a", "model.2.emb_b", "model.2.emb_mix", "model.2.query_conv.weight", "model.2.key_conv.weight",
                  "model.2.value_conv.0.weight", "model.2.value_conv.3.weight"):
            assert not torch.equal(before[k], after[k]), k
        assert ac.rel_h.data_ptr() >= opt.params_arena.data_ptr() and st.emb_mix.grad.data_ptr() >= opt.grads_arena.data_ptr()
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
        print("[attention replay] losses", le, lr_)
        assert le[2:] == lr_[2:], (le, lr_)
        for k, v in res["eager"][1].items():
            assert torch.equal(v, res["replay"][1][k]), k
    finally:
        config.set_deterministic(None)
        ydl.set_compute_dtype("bf16")
