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

import numpy as np
import pytest
import torch

from tests.test_builders_act_cpu import FILES, YAML, build

pytestmark = pytest.mark.gpu

FLOOR_FACTOR = 4.0
NEW_ENTRIES = ("ydl_bn_act_fwd_p", "ydl_bn_act_bwd_p", "ydl_bn_act_fwd_sums_p", "ydl_bn_act_bwd_sums_p", "ydl_bn_act_bwd_apply_sums_p",
               "ydl_bn_act_bwd_reduce_sums_p", "ydl_acon_fwd", "ydl_acon_bwd", "ydl_max2_fwd", "ydl_max2_bwd")


def _err(got, want):
    want = torch.as_tensor(want).double()
    scale = float(want.abs().max())
    return float((got.detach().double().cpu() - want).abs().max()) / (scale if scale > 0 else 1.0)


def _module(z):
    mod = build(z)
    sd = mod.state_dict()
    mod.load_state_dict({str(k): torch.from_numpy(z["p." + str(k)]).to(sd[str(k)].dtype) for k in z["keys"]})
    return mod.cuda().train()


def _step(z):
    """one train-mode forward + backward of the fixture's module -> (module, x, out, errors by tensor)"""
    mod = _module(z)
    x = torch.from_numpy(z["x"]).float().cuda().requires_grad_(True)
    out = mod(x)
    assert tuple(out.shape) == tuple(z["out"].shape)
    out.backward(torch.from_numpy(z["grad_out"]).float().cuda())
    torch.cuda.synchronize()
    errs = {"out": _err(out, z["out"]), "grad_x": _err(x.grad, z["grad_x"])}
    for k, p in mod.named_parameters():
        assert p.grad is not None, k
        errs["g." + k] = _err(p.grad, z["g." + k])
    sd = mod.state_dict()
    for k in z.files:
        if k.startswith("rm.") or k.startswith("rv."):
            errs[k] = _err(sd[k[3:]], z[k])
    return mod, x, out, errs


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_modules_match_the_reference_fixtures(path):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    try:
        z = np.load(path)
        mod, x, out, errs = _step(z)
        print(os.path.basename(path), {k: f"{v:.1e}" for k, v in errs.items()})
        assert any(k.startswith("rv.") for k in errs)
        assert all(v < 1e-4 for v in errs.values()), {k: v for k, v in errs.items() if not v < 1e-4}
        # eval mode: the forward runs on the running statistics and records nothing
        before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
        mod.eval()
        with torch.no_grad():
            out_eval = mod(x.detach())
        torch.cuda.synchronize()
        assert out_eval.shape == out.shape and bool(torch.isfinite(out_eval).all()) and out_eval.grad_fn is None
        # fuse(): every dense Conv folds its own BatchNorm; AconC / FReLU run behind the folded conv, FReLU's inner BatchNorm stays
        fused = 0
        for m in mod.modules():
            if isinstance(m, ydl.Conv) and not m.depthwise:
                m.fuse()
                fused += 1
        if fused:
            with torch.no_grad():
                out_fused = mod(x.detach())
            torch.cuda.synchronize()
            assert _err(out_fused, out_eval.cpu()) < 1e-4
        for k, v in mod.state_dict().items():
            assert torch.equal(v, before[k]), k
    finally:
        ydl.set_compute_dtype("bf16")


def _kind(k):
    return "out" if k == "out" else "run" if k[:3] in ("rm.", "rv.") else "grad"


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_bf16_mode_against_the_fixtures(path):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("bf16")
    z = np.load(path)
    name = os.path.basename(path)[:-4]
    floor = {k: float(z["floor." + k]) for k in ("out", "grad", "run")}
    _mod, _x, _out, errs = _step(z)
    worst = {"out": (0.0, ""), "grad": (0.0, ""), "run": (0.0, "")}
    for k, v in errs.items():
        worst[_kind(k)] = max(worst[_kind(k)], (v, k))
    print("[act bf16]", name, {k: f"{v:.2e} ({w}) floor {floor[k]:.2e} ratio {v / floor[k]:.2f}" for k, (v, w) in worst.items()})
    bad = {k: (v, FLOOR_FACTOR * floor[_kind(k)]) for k, v in errs.items() if not v < FLOOR_FACTOR * floor[_kind(k)]}
    assert not bad, bad


def _setup(mode):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype(mode)
    torch.manual_seed(11)
    m = ydl.SegYoloModel(dict(YAML, activation="nn.Mish()"))
    with ydl.default_activation("nn.Mish()"):
        down = ydl.Conv(16, 32, 3, 2, act=ydl.AconC(32))                    # the down-sampler, under AconC
        down.i, down.f, down.type, down.np = m.model[1].i, m.model[1].f, m.model[1].type, m.model[1].np
        m.model[1] = down
        m.model[2].cv3 = ydl.Conv(32, 32, 1, 1, act=ydl.FReLU(32))          # the C3's output convolution, under FReLU
    m = m.cuda().train()
    opt = ydl.smart_optimizer(m, "SGD", lr=0.01, momentum=0.937, decay=5e-4)
    crit = ydl.SegmentationLoss(12, 0.0, torch.ones(12), "dice", sync=False)
    gen = torch.Generator("cuda").manual_seed(3)
    xs = [torch.rand(2, 3, 32, 32, device="cuda", generator=gen) for _ in range(2)]
    ts = [torch.randint(0, 12, (2, 8, 8), device="cuda", generator=gen) for _ in range(2)]
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
        assert sum(isinstance(c.act, torch.nn.Mish) for c in m.modules() if isinstance(c, ydl.Conv)) == 8
        before = _state(m, opt)
        opt.zero_grad()
        out = m(xs[0])
        assert out.shape == (2, 12, 8, 8)
        total, items = crit(out, ts[0])
        total.backward()
        params = dict(m.named_parameters())
        for k in ("model.1.act.p1", "model.1.act.p2", "model.1.act.beta", "model.2.cv3.act.conv.weight", "model.2.cv3.act.bn.weight"):
            assert k in params, k
        assert all(getattr(p, "_ydl_touched", False) for p in params.values()), [k for k, p in params.items() if not getattr(p, "_ydl_touched", False)]
        opt.step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(total)) and bool(torch.isfinite(opt.params_arena).all())
        after = _state(m, opt)
        for k in params:                                   # the fused optimizer step moved every parameter
            assert not torch.equal(before[k], after[k]), k
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
                for fn in NEW_ENTRIES:
                    assert r.rec.fn.get(fn) is not None, fn
                losses = [None, None, float(r.loss_items[0])]
                r.poison()
                for st in range(3, 5):
                    x.copy_(xs[st % 2]); t.copy_(ts[st % 2])
                    losses.append(float(r.step()[0]))
            torch.cuda.synchronize()
            res[how] = (losses, _state(m, opt))
        le, lr_ = res["eager"][0], res["replay"][0]
        print("[act replay] losses", le, lr_)
        assert le[2:] == lr_[2:], (le, lr_)
        for k, v in res["eager"][1].items():
            assert torch.equal(v, res["replay"][1][k]), k
    finally:
        config.set_deterministic(None)
        ydl.set_compute_dtype("bf16")


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
