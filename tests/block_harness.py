"""What the block-family tests (tests/test_gpu_*_blocks.py, tests/test_builders_*_cpu.py) share: the error measure, the one step of a
fixture's module and its f32 / bf16 checks, the small yaml model's setup, eager step and replayed-equals-eager check.  A family's file
keeps its tolerances with the comment on how they were measured, its ``build``, its thin test functions and its own tails; a new family
starts from this module and tools/golden_blocks.py, not from a copy of another family's file.  Not collected, not a conftest."""
import json
import os

import numpy as np
import torch

F32_TOL = 1e-4          # the project's bound for module fixtures in f32 mode, relative to each tensor's max


def rel_max_err(got, want, scale=None):
    """max |got - want| in float64, relative to max |want| (or ``scale``); against an all-zero ``want`` the absolute error"""
    want = torch.as_tensor(want).double()
    scale = float(want.abs().max()) if scale is None else scale
    return float((got.detach().double().cpu() - want).abs().max()) / (scale if scale > 0 else 1.0)


def kind(key):
    return "out" if key == "out" else "run" if key[:3] in ("rm.", "rv.") else "grad"


def build_from_json(z):
    """the module a fixture describes (weights not loaded): class name and positional arguments as a JSON list"""
    import yolo_dual_amd as ydl
    return getattr(ydl, str(z["cls"]))(*json.loads(str(z["args"])))


def check_state_dict_layout(path, build):
    """the module's state_dict has the fixture's keys and shapes, in order, and loads the fixture's values -> (z, module, [(key, shape)])"""
    z = np.load(path)
    mod = build(z)
    want = [(str(k), tuple(z["p." + str(k)].shape)) for k in z["keys"]]
    assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == want
    mod.load_state_dict({k: torch.from_numpy(z["p." + k]).to(mod.state_dict()[k].dtype) for k, _ in want})
    return z, mod, want


def load_module(z, build):
    mod = build(z)
    sd = mod.state_dict()
    mod.load_state_dict({str(k): torch.from_numpy(z["p." + str(k)]).to(sd[str(k)].dtype) for k in z["keys"]})
    return mod.cuda().train()


def zero_bias_scale(z, key, zero_bias_rel):
    """A BatchNorm bias in front of a linear layer and another train-mode BatchNorm has an exactly zero gradient: float64 leaves round-off
    and no scale of its own.  Where the fixture's ``g.<key>`` of a ``bn.bias`` is below ``zero_bias_rel`` times the same layer's weight
    gradient (a sum over the same dz), that weight gradient's max is the scale its error is measured against; otherwise, and always with
    ``zero_bias_rel=None``, None: the tensor's own max."""
    if zero_bias_rel is None or not key.endswith("bn.bias"):
        return None
    gw = float(np.abs(z["g." + key[:-4] + "weight"]).max())
    return gw if float(np.abs(z["g." + key]).max()) < zero_bias_rel * gw else None


def fixture_step(z, build, zero_bias_rel=None):
    """one train-mode forward + backward of the fixture's module -> (module, x, out, errors by tensor); the running statistics are
    compared where the fixture holds them"""
    mod = load_module(z, build)
    x = torch.from_numpy(z["x"]).float().cuda().requires_grad_(True)
    out = mod(x)
    assert tuple(out.shape) == tuple(z["out"].shape)
    out.backward(torch.from_numpy(z["grad_out"]).float().cuda())
    torch.cuda.synchronize()
    errs = {"out": rel_max_err(out, z["out"]), "grad_x": rel_max_err(x.grad, z["grad_x"])}
    for k, p in mod.named_parameters():
        assert p.grad is not None, k
        errs["g." + k] = rel_max_err(p.grad, z["g." + k], zero_bias_scale(z, k, zero_bias_rel))
    sd = mod.state_dict()
    for k in z.files:
        if kind(k) == "run":
            errs[k] = rel_max_err(sd[k[3:]], z[k])
    return mod, x, out, errs


def _name(path):
    return os.path.basename(path)[:-4]


def _fmt(errs):
    return {k: f"{v:.1e}" for k, v in errs.items()}


def check_f32_fixture(path, build, expect_running_stats=True, zero_bias_rel=None, after_eval=None):
    """f32 mode: every tensor of the step within F32_TOL of the fixture; then the eval-mode forward runs on the running statistics, is
    finite, records nothing and leaves the state alone (checked after ``after_eval(mod, x, out, out_eval)``, a family's own addition)"""
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    try:
        mod, x, out, errs = fixture_step(np.load(path), build, zero_bias_rel)
        print(os.path.basename(path), _fmt(errs))
        assert not expect_running_stats or any(k.startswith("rv.") for k in errs)
        assert all(v < F32_TOL for v in errs.values()), {k: v for k, v in errs.items() if not v < F32_TOL}
        before = {k: v.detach().clone() for k, v in mod.state_dict().items()}
        mod.eval()
        with torch.no_grad():
            out_eval = mod(x.detach())
        torch.cuda.synchronize()
        assert out_eval.shape == out.shape and bool(torch.isfinite(out_eval).all()) and out_eval.grad_fn is None
        if after_eval is not None:
            after_eval(mod, x, out, out_eval)
        for k, v in mod.state_dict().items():
            assert torch.equal(v, before[k]), k
    finally:
        ydl.set_compute_dtype("bf16")


def worst_by_kind(errs, kinds=("out", "grad", "run")):
    worst = {k: (0.0, "") for k in kinds}
    for k, v in errs.items():
        worst[kind(k)] = max(worst[kind(k)], (v, k))
    return worst


def judge_against_tol(errs, tol):
    """errors by tensor against one bound per kind -> the tensors that miss it"""
    return {k: v for k, v in errs.items() if not v < tol[kind(k)]}


def judge_against_floor(errs, floor, factor):
    """errors by tensor against ``factor`` times the fixture's recorded bf16 floor of their kind -> {tensor: (error, bound)} of the misses"""
    return {k: (v, factor * floor[kind(k)]) for k, v in errs.items() if not v < factor * floor[kind(k)]}


def check_bf16_against_tol(files, build, tol, label, zero_bias_rel=None):
    """bf16 mode over all the family's fixtures against the bounds measured on an MI355X, ``tol`` by kind; prints every error and the worst"""
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("bf16")
    worst, bad = {k: (0.0, "") for k in tol}, {}
    for path in files:
        _mod, _x, _out, errs = fixture_step(np.load(path), build, zero_bias_rel)
        print(f"[{label} bf16]", _name(path), _fmt(errs))
        for k, (v, w) in worst_by_kind(errs, tuple(tol)).items():
            worst[k] = max(worst[k], (v, _name(path) + ":" + w))
        bad.update((_name(path) + ":" + k, v) for k, v in judge_against_tol(errs, tol).items())
    print(f"[{label} bf16] worst", {k: (f"{v:.2e}", w) for k, (v, w) in worst.items()})
    assert not bad, bad


def check_bf16_against_floor(path, build, factor, kinds, label):
    """bf16 mode on one fixture: per tensor the bound is ``factor`` times the bf16 floor the fixture records for its kind"""
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("bf16")
    z = np.load(path)
    floor = {k: float(z["floor." + k]) for k in kinds}
    _mod, _x, _out, errs = fixture_step(z, build)
    print(f"[{label} bf16]", _name(path),
          {k: f"{v:.2e} ({w}) floor {floor[k]:.2e} ratio {v / floor[k]:.2f}" for k, (v, w) in worst_by_kind(errs, kinds).items()})
    bad = judge_against_floor(errs, floor, factor)
    assert not bad, bad


def train_setup(yaml, mode, target_hw, patch=None):
    """the small yaml model under SGD and the dice loss, two 2 x 3 x 32 x 32 inputs and two targets of ``target_hw`` squared;
    ``patch(m)`` changes the model in place before it moves to the GPU"""
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype(mode)
    torch.manual_seed(11)
    m = ydl.SegYoloModel(yaml)
    if patch is not None:
        patch(m)
    m = m.cuda().train()
    opt = ydl.smart_optimizer(m, "SGD", lr=0.01, momentum=0.937, decay=5e-4)
    crit = ydl.SegmentationLoss(12, 0.0, torch.ones(12), "dice", sync=False)
    gen = torch.Generator("cuda").manual_seed(3)
    xs = [torch.rand(2, 3, 32, 32, device="cuda", generator=gen) for _ in range(2)]
    ts = [torch.randint(0, 12, (2, target_hw, target_hw), device="cuda", generator=gen) for _ in range(2)]
    return m, opt, crit, xs, ts


def train_state(m, opt):
    out = {k: v.detach().clone() for k, v in m.state_dict().items()}
    out["__momentum"] = opt.mom_arena.detach().clone()
    out["__ema"] = opt.ema_arena.detach().clone()
    return out


def eager_step_checks(m, opt, crit, xs, ts, out_shape):
    """one full eager training step: the output's shape, every parameter touched by the backward, loss and parameters finite ->
    (parameters by name, state before, state after) for the family's own tail"""
    before = train_state(m, opt)
    opt.zero_grad()
    out = m(xs[0])
    assert out.shape == out_shape
    total, _items = crit(out, ts[0])
    total.backward()
    params = dict(m.named_parameters())
    assert all(getattr(p, "_ydl_touched", False) for p in params.values()), [k for k, p in params.items() if not getattr(p, "_ydl_touched", False)]
    opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(total)) and bool(torch.isfinite(opt.params_arena).all())
    return params, before, train_state(m, opt)


def check_replay_equals_eager(setup, label, entries=()):
    """deterministic f32 mode: five steps, eager against recorded-then-replayed (two warm-up steps, the recording, two replays after
    the pool was poisoned), leave the same losses from the recording on and the same state, bit for bit; ``entries`` are entry points
    that must be in the replay table"""
    import yolo_dual_amd as ydl
    from yolo_dual_amd import config
    from yolo_dual_amd.replay import ReplayedTrainStep
    config.set_deterministic(True)
    try:
        res = {}
        for how in ("eager", "replay"):
            m, opt, crit, xs, ts = setup("f32")
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
                for fn in entries:
                    assert r.rec.fn.get(fn) is not None, fn
                losses = [None, None, float(r.loss_items[0])]
                r.poison()
                for st in range(3, 5):
                    x.copy_(xs[st % 2]); t.copy_(ts[st % 2])
                    losses.append(float(r.step()[0]))
            torch.cuda.synchronize()
            res[how] = (losses, train_state(m, opt))
        le, lr_ = res["eager"][0], res["replay"][0]
        print(f"[{label} replay] losses", le, lr_)
        assert le[2:] == lr_[2:], (le, lr_)
        for k, v in res["eager"][1].items():
            assert torch.equal(v, res["replay"][1][k]), k
    finally:
        config.set_deterministic(None)
        ydl.set_compute_dtype("bf16")
