"""GPU: the fused Adam / AdamW / RMSProp + EMA steps (csrc/optim.hip, yolo_dual_amd/optim.py) against ``torch.optim`` itself — the
single-tensor CPU path the reference's ``smart_optimizer`` runs — and through every consumer of the optimizer protocol: the
one-launch run table, the launch-list replay, checkpoints, data parallelism and the CLI.  The three entry forms of every rule of
the family, SGD among them, are held to each other bit for bit.

Tolerance of the trajectory tests: the error is measured against float64 torch.optim on the same f32 inputs, relative to the distance
the parameters moved, and the HIP error may be at most 4x the error of torch's OWN f32 run measured in the same test (room for FMA
contraction and for the rounding of division and square root; a wrong bias correction or a misplaced decay is off by orders of
magnitude)."""
import copy
import io
import math
import os
import socket

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

NAMES = ("Adam", "AdamW", "RMSProp")
RULES = {"Adam": 1, "AdamW": 2, "RMSProp": 3}
FORMATS = {"Adam": "ydl-flat-adam-ema-1", "AdamW": "ydl-flat-adamw-ema-1", "RMSProp": "ydl-flat-rmsprop-ema-1"}
LR0, MOM, WD, GSCALE, STEPS = 0.004, 0.937, 5e-4, 0.5, 14
CFG = os.path.join(os.path.dirname(__file__), "..", "yolo_dual_amd", "cfg")


class _Blob(nn.Module):
    """a parameter named ``weight`` outside a norm layer: the decay group"""

    def __init__(self, n):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n))


def _flat_model(seed=0):
    """390 413 parameters in three groups; sizes that are not multiples of four, so runs start at unaligned arena offsets"""
    m = nn.Sequential(nn.Linear(300, 400), nn.BatchNorm1d(60001), _Blob(100003), _Blob(7), _Blob(50001))
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=gen))
        m[1].running_mean.copy_(torch.randn(60001, generator=gen))
        m[1].running_var.copy_(torch.rand(60001, generator=gen) + 0.5)
    return m


def _torch_optimizer(m, name, lr):
    """the reference's smart_optimizer on plain torch: biases | weights with decay | norm weights"""
    g0 = [m[0].weight, m[2].weight, m[3].weight, m[4].weight]
    g1, g2 = [m[1].weight], [m[0].bias, m[1].bias]
    if name == "Adam":
        o = torch.optim.Adam(g2, lr=lr, betas=(MOM, 0.999), foreach=False)
    elif name == "AdamW":
        o = torch.optim.AdamW(g2, lr=lr, betas=(MOM, 0.999), weight_decay=0.0, foreach=False)
    else:
        o = torch.optim.RMSprop(g2, lr=lr, momentum=MOM, foreach=False)
    o.add_param_group({"params": g0, "weight_decay": WD})
    o.add_param_group({"params": g1, "weight_decay": 0.0})
    return o


def _grads(m, step):
    """seeded gradients whose scale varies by step; every 97th element is exactly 0"""
    gen = torch.Generator().manual_seed(1000 + step)
    scale = 10.0 ** (1.5 * math.sin(1.7 * step))
    out = {}
    for k, p in m.named_parameters():
        g = torch.randn(p.shape, generator=gen) * scale
        g.view(-1)[::97] = 0.0
        out[k] = g
    return out


def _lrs(step):
    """(bias, weights, norm weights) learning rates of a step: they change every step and differ by group"""
    lr = LR0 * (1.0 + 0.5 * math.sin(0.9 * step + 0.3))
    return 2.0 * lr, lr, 0.5 * lr


def _ema_d(n):
    return 0.9999 * (1.0 - math.exp(-n / 2000.0))


def _torch_trajectory(name, dtype, live):
    """torch.optim on the CPU in ``dtype`` + ModelEMA's update (utils/torch_utils.py:404-428); ``live(key, step)`` says whether a
    parameter has a gradient in a step (None otherwise, as for the reference's dead head layers)"""
    m = _flat_model().to(dtype)
    opt = _torch_optimizer(m, name, LR0)
    ema = {k: v.detach().clone() for k, v in m.state_dict().items() if v.dtype.is_floating_point}
    for step in range(STEPS):
        for g, lr in zip(opt.param_groups, _lrs(step)):
            g["lr"] = lr
        gs = _grads(m, step)
        for k, p in m.named_parameters():
            p.grad = (gs[k] * GSCALE).to(dtype) if live(k, step) else None
        opt.step()
        d = _ema_d(step + 1)
        with torch.no_grad():
            msd = m.state_dict()
            for k, v in ema.items():
                v *= d
                v += (1 - d) * msd[k].detach()
    return {k: v.detach().clone() for k, v in m.state_dict().items() if v.dtype.is_floating_point}, ema, opt


def _hip_trajectory(name, live, steps=STEPS, opt_and_model=None, first_step=0):
    import yolo_dual_amd as ydl
    from yolo_dual_amd import config
    if opt_and_model is None:
        m = _flat_model().cuda()
        opt = ydl.smart_optimizer(m, name, LR0, MOM, WD)
    else:
        opt, m = opt_and_model
    for step in range(first_step, first_step + steps):
        for g, lr in zip(opt.param_groups, _lrs(step)):
            g["lr"] = lr
        opt.zero_grad()
        gs = _grads(m, step)
        for k, p in m.named_parameters():
            if live(k, step):
                p.grad.copy_(gs[k])                       # the arena view, as the wgrad / BN-backward kernels write it
                config.mark_touched(p)                    # what the tape does when a gradient kernel ran
        opt.step(grad_scale=GSCALE)
    torch.cuda.synchronize()
    return opt, m


def _cat(sd, keys):
    return torch.cat([sd[k].detach().reshape(-1).double().cpu() for k in keys])


def _err(x, ref64, start64, keys):
    moved = float((_cat(ref64, keys) - _cat(start64, keys)).abs().max())
    return float((_cat(x, keys) - _cat(ref64, keys)).abs().max()) / moved


def _always(_k, _step):
    return True


@pytest.mark.parametrize("name", NAMES)
def test_trajectory_matches_torch_optim(name):
    """14 steps, lr changing every step, grad_scale 0.5, weight decay on the weights group: parameters and EMA shadow against
    torch.optim in float64, within 4x the error of torch.optim in float32"""
    start = {k: v.clone() for k, v in _flat_model().state_dict().items() if v.dtype.is_floating_point}
    p64, e64, _ = _torch_trajectory(name, torch.float64, _always)
    p32, e32, _ = _torch_trajectory(name, torch.float32, _always)
    opt, m = _hip_trajectory(name, _always)
    pkeys = [k for k, _ in m.named_parameters()]
    allkeys = list(start)
    hip = m.state_dict()
    err_hip, err_f32 = _err(hip, p64, start, pkeys), _err(p32, p64, start, pkeys)
    print(f"{name} parameters: HIP error {err_hip:.3e}, torch f32 error {err_f32:.3e}, ratio {err_hip / err_f32:.2f}")
    assert err_hip <= 4.0 * err_f32, (err_hip, err_f32)
    ema = opt.ema_state_dict()
    eerr_hip, eerr_f32 = _err(ema, e64, start, allkeys), _err(e32, e64, start, allkeys)
    print(f"{name} EMA: HIP error {eerr_hip:.3e}, torch f32 error {eerr_f32:.3e}, ratio {eerr_hip / eerr_f32:.2f}")
    assert eerr_hip <= 4.0 * eerr_f32, (eerr_hip, eerr_f32)
    assert opt.updates == STEPS and set(opt._steps) == {STEPS}
    # the per-group values a scheduler wrote are the ones the kernels used (a wrong lr index is far outside the tolerance above)
    for k in ("running_mean", "running_var"):
        assert torch.equal(hip["1." + k].cpu(), start["1." + k])


@pytest.mark.parametrize("name", NAMES)
def test_skipped_and_late_parameters(name):
    """a parameter that never gets a gradient keeps its value and state bit for bit and its step count 0; one whose first gradient
    arrives at step 4 is bias-corrected with t = 1 there, as torch.optim does for ``grad is None``"""
    dead, late = "2.weight", "4.weight"

    def live(k, step):
        return k != dead and (k != late or step >= 3)

    start = {k: v.clone() for k, v in _flat_model().state_dict().items() if v.dtype.is_floating_point}
    p64, e64, _ = _torch_trajectory(name, torch.float64, live)
    p32, e32, o32 = _torch_trajectory(name, torch.float32, live)
    opt, m = _hip_trajectory(name, live)
    hip = m.state_dict()
    slot = {id(p): (i, off, n) for i, (p, off, n, _g) in enumerate(opt._slots)}
    i, off, n = slot[id(m[2].weight)]
    assert torch.equal(hip[dead].cpu(), start[dead])
    assert opt._steps[i] == 0
    assert not bool(opt.state1_arena[off:off + n].any()) and not bool(opt.state2_arena[off:off + n].any())
    assert torch.equal(p32[dead], start[dead])                                  # torch skips it too
    i, off, n = slot[id(m[4].weight)]
    assert opt._steps[i] == STEPS - 3 and max(opt._steps) == STEPS
    for keys, what in (([late], "late parameter"), ([k for k, _ in m.named_parameters() if k != dead], "all live parameters")):
        err_hip, err_f32 = _err(hip, p64, start, keys), _err(p32, p64, start, keys)
        print(f"{name} {what}: HIP error {err_hip:.3e}, torch f32 error {err_f32:.3e}, ratio {err_hip / err_f32:.2f}")
        assert err_hip <= 4.0 * err_f32, (what, err_hip, err_f32)
    ema = opt.ema_state_dict()
    eerr_hip, eerr_f32 = _err(ema, e64, start, list(start)), _err(e32, e64, start, list(start))
    print(f"{name} EMA: HIP error {eerr_hip:.3e}, torch f32 error {eerr_f32:.3e}")
    assert eerr_hip <= 4.0 * eerr_f32, (eerr_hip, eerr_f32)


def _hyper_vector(name):
    """device hyper vector of a rule (ydl.h) with three bias-correction classes, and the same f32 values as Python floats"""
    from yolo_dual_amd import _lib as L
    lrs, b1, b2, wd = (0.01, 0.02, 0.03), 0.9, 0.999, 5e-4
    vals = [*lrs, b1, wd, 0.5, 0.999]
    if name != "SGD":
        vals += [b2, 1e-8, 1.0 - b1, 1.0 - b2, 1.0 - lrs[0] * wd] + [0.0] * (L.OPT_HYPER_FLOATS - 12)
        for c, t in enumerate((1, 5, 12)):
            for i in range(3):
                vals[12 + 4 * c + i] = lrs[i] / (1.0 - b1 ** t)
            vals[12 + 4 * c + 3] = (1.0 - b2 ** t) ** 0.5
    hyper_cpu = torch.tensor(vals, dtype=torch.float64).float()
    return hyper_cpu.cuda(), [float(v) for v in hyper_cpu]


def _entry(name):
    return ("ydl_sgd_ema_step", ()) if name == "SGD" else ("ydl_optim_ema_step", (RULES[name],))


def _step_multi(name, arrs, rows, hyper, use_ema):
    """all rows in one launch; ``arrs`` = [params, grads, state arena(s), ema]"""
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.tape import _p, _stream
    entry, rule = _entry(name)
    tab = torch.tensor(rows, dtype=torch.int64).cuda()
    L.call(entry + "_multi", *rule, *[_p(x) for x in arrs[:-1]], _p(arrs[-1]) if use_ema else None, _p(tab), len(rows),
           max(r[3] for r in rows), _p(hyper), use_ema, _stream())
    torch.cuda.synchronize()                               # the table is a local


def _step_runs(name, form, arrs, rows, hyper, h, use_ema):
    """the same rows one launch each, through the device-hyper (``dev``) or the host-scalar (``host``) entry point"""
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.tape import _p, _stream
    entry, rule = _entry(name)
    for row in rows:
        off, nd, npar, n, gi, fl = row[:6]
        if npar == 0 and not use_ema:
            continue
        ptrs = [_p(x[off:]) for x in arrs[:-1]] + [_p(arrs[-1][off:]) if use_ema else None]
        d = h[6] if use_ema else -1.0
        if form == "dev":
            tail = (gi, fl & 1, (fl >> 1) & 1) if name == "SGD" else (gi, row[6], fl & 1)
            L.call(entry + "_dev", *rule, *ptrs, nd, npar, n, _p(hyper), *tail, use_ema, _stream())
        elif name == "SGD":
            L.call(entry, *ptrs, nd, npar, n, h[gi], h[gi], h[3], h[4] if fl & 1 else 0.0, h[5], (fl >> 1) & 1, d, _stream())
        else:
            c = row[6]
            step_size = h[gi] if name == "RMSProp" else h[12 + 4 * c + gi]
            L.call(entry, *rule, *ptrs, nd, npar, n, step_size, h[12 + 4 * c + 3], h[11], h[4] if fl & 1 else 0.0, h[3], h[7], h[9], h[10],
                   h[8], h[5], d, _stream())


def _check_three_forms(name, base, rows):
    """multi == dev run by run == host scalars run by run, bit for bit on every array, with and without EMA"""
    hyper, h = _hyper_vector(name)
    assert rows[-1][0] + rows[-1][3] == base[0].numel() and all(a[0] + a[3] == b[0] for a, b in zip(rows, rows[1:]))
    for use_ema in (1, 0):
        a, b, c = ([t.clone() for t in base] for _ in range(3))
        _step_multi(name, a, rows, hyper, use_ema)
        _step_runs(name, "dev", b, rows, hyper, h, use_ema)
        _step_runs(name, "host", c, rows, hyper, h, use_ema)
        torch.cuda.synchronize()
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z)
        assert torch.equal(a[1], base[1]) and all(not torch.equal(x, y) for x, y in zip(a[:-1], base[:-1]) if x is not a[1])
        assert torch.equal(a[-1], base[-1]) != bool(use_ema)
        assert bool(torch.isfinite(a[0]).all())


def _arrays(n, count, seed=3):
    gen = torch.Generator("cuda").manual_seed(seed)
    return [torch.randn(n, device="cuda", generator=gen) for _ in range(count)]


@pytest.mark.parametrize("name", NAMES)
def test_multi_run_launch_equals_the_per_run_launches(name):
    """ydl_optim_ema_step_multi (one launch, float4 groups aligned to the arena, element form at the run ends) against
    ydl_optim_ema_step_dev run by run and against the host-scalar ydl_optim_ema_step, bit for bit — runs at offsets that are not
    multiples of four, of lengths 1..5 and large, with and without weight decay, EMA-only rows, three bias-correction classes"""
    base = _arrays(70001, 5)
    base[3] = base[3].abs()                                # exp_avg_sq / square_avg are sums of squares
    # (offset, n_decay, n_params, n_total, lr index, flags, class, 0)
    rows = [(0, 3, 3, 3, 0, 1, 0, 0), (3, 0, 5, 5, 1, 0, 1, 0), (8, 0, 0, 1, 0, 0, 0, 0), (9, 30001, 30001, 30001, 0, 1, 2, 0),
            (30010, 0, 20002, 20002, 2, 0, 1, 0), (50012, 2, 2, 2, 0, 1, 1, 0), (50014, 0, 4, 4, 2, 0, 0, 0), (50018, 0, 0, 19983, 0, 0, 0, 0)]
    _check_three_forms(name, base, rows)


def test_multi_run_optimizer_launch_equals_the_per_run_launches():
    """the same for SGD: ydl_sgd_ema_step_multi against ydl_sgd_ema_step_dev and the host-scalar ydl_sgd_ema_step run by run, bit
    for bit on parameters, momentum, EMA and the untouched gradients — rows of lengths 1..5 at offsets 1, 2 and 3 mod 4 and large,
    with and without weight decay / first step (also a first-step row without decay), EMA-only rows between them"""
    base = _arrays(70001, 4)
    # (offset, n_decay, n_params, n_total, lr index, flags: 1 weight decay | 2 first step)
    rows = [(0, 3, 3, 3, 0, 1), (3, 0, 5, 5, 1, 0), (8, 0, 0, 1, 0, 0), (9, 30001, 30001, 30001, 0, 1 | 2), (30010, 0, 20002, 20002, 2, 0),
            (50012, 0, 1, 1, 1, 2), (50013, 5, 5, 5, 0, 1), (50018, 0, 4, 4, 2, 2), (50022, 0, 0, 1, 0, 0), (50023, 2, 2, 2, 0, 1 | 2),
            (50025, 0, 3, 3, 1, 0), (50028, 0, 2, 2, 2, 0), (50030, 1, 1, 1, 0, 1), (50031, 0, 0, 19970, 0, 0)]
    assert {(r[0] % 4, r[3]) for r in rows} >= {(1, 5), (2, 4), (3, 2), (1, 3), (2, 1)}
    _check_three_forms("SGD", base, rows)


def test_sgd_host_scalar_step_keeps_two_learning_rates():
    """one ydl_sgd_ema_step over [decay | no decay | buffers] (n_decay 3 < n_params 7 < n_total 9) with a learning rate per part
    equals, bit for bit, the three ranges stepped one uniform call each — at an arena offset that is not a multiple of four, on a
    first and on a later step"""
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.tape import _p, _stream
    base = _arrays(16, 4, seed=4)
    lr0, lr1, mom, wd, gs, d, off = 0.01, 0.07, 0.9, 5e-4, 0.5, 0.999, 5
    for first in (1, 0):
        a, b = ([t.clone() for t in base] for _ in range(2))
        L.call("ydl_sgd_ema_step", *[_p(x[off:]) for x in a], 3, 7, 9, lr0, lr1, mom, wd, gs, first, d, _stream())
        for o, nd, npar, n, lr in ((off, 3, 3, 3, lr0), (off + 3, 0, 4, 4, lr1), (off + 7, 0, 0, 2, 0.0)):
            L.call("ydl_sgd_ema_step", *[_p(x[o:]) for x in b], nd, npar, n, lr, lr, mom, wd, gs, first, d, _stream())
        torch.cuda.synchronize()
        for x, y, z in zip(a, b, base):
            assert torch.equal(x, y) and torch.equal(x[:off], z[:off]) and torch.equal(x[off + 9:], z[off + 9:])
        assert torch.equal(a[1], base[1]) and not torch.equal(a[0][off:off + 7], base[0][off:off + 7])
        assert torch.equal(a[0][off + 7:], base[0][off + 7:]) and not torch.equal(a[3][off:off + 9], base[3][off:off + 9])


@pytest.mark.parametrize("name", ("SGD", "AdamW"))
def test_per_run_launches_on_arrays_that_are_not_co_aligned(name):
    """the per-run forms with the gradient array one element out of step with the others (a view from element 1 of a longer tensor)
    cannot rebase onto a common 16-byte boundary and take the element walk: bit for bit the multi launch on co-aligned copies"""
    n = 4099
    base = _arrays(n, 4 if name == "SGD" else 5)
    base[-2] = base[-2].abs()                              # the adaptive rule's sums of squares (SGD: its momentum, any sign would do)
    cols, none = ((), ()) if name == "SGD" else ((1, 0), (0, 0))          # the family's rows go on with {class, 0}
    rows = [(0, 1501, 1501, 1501, 0, 1) + cols, (1501, 0, 1300, 1300, 1, 0) + cols, (2801, 0, 0, 298, 0, 0) + none,
            (3099, 0, 1000, 1000, 2, 0) + cols]
    hyper, h = _hyper_vector(name)
    for use_ema in (1, 0):
        a = [t.clone() for t in base]
        _step_multi(name, a, rows, hyper, use_ema)
        for form in ("dev", "host"):
            b = [t.clone() for t in base]
            longer = torch.zeros(n + 1, device="cuda")
            longer[1:].copy_(base[1])
            b[1] = longer[1:]
            assert b[1].data_ptr() % 16 == 4 and all(x.data_ptr() % 16 == 0 for x in b if x is not b[1])
            _step_runs(name, form, b, rows, hyper, h, use_ema)
            torch.cuda.synchronize()
            for x, y in zip(a, b):
                assert torch.equal(x, y), form
            assert float(longer[0]) == 0.0 and torch.equal(b[1], base[1]) and not torch.equal(b[0], base[0])


class _TorchConv(nn.Module):
    """Conv2d(bias=False) + BatchNorm2d + SiLU with the key names of yolo_dual_amd.Conv"""

    def __init__(self, c1, c2, k, bn):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, 1, k // 2, bias=False)
        self.bn = nn.BatchNorm2d(c2, eps=bn.eps, momentum=bn.momentum)
        self.act = nn.SiLU()

    def forward(self, x):
        return self.act(self.bn(self.conv(x)))


def test_adamw_on_a_real_model_matches_plain_torch():
    """Conv(4,8,3) -> Conv(8,4,1) in f32 mode, 3 AdamW steps with fused EMA, against the same modules in plain torch on the CPU with
    the reference's smart_optimizer groups and ModelEMA (tolerance of test_sgd_ema_flat_optimizer for this net)"""
    import yolo_dual_amd as ydl
    from tests.util import rel_err
    ydl.set_compute_dtype("f32")
    try:
        torch.manual_seed(5)
        net = nn.Sequential(ydl.Conv(4, 8, 3, 1), ydl.Conv(8, 4, 1, 1))
        ref = nn.Sequential(_TorchConv(4, 8, 3, net[0].bn), _TorchConv(8, 4, 1, net[1].bn))
        ref.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
        ref.train()
        lr, wd = 0.01, 5e-4
        ropt = torch.optim.AdamW([p for k, p in ref.named_parameters() if k.endswith("bias")], lr=lr, betas=(MOM, 0.999), weight_decay=0.0,
                                 foreach=False)
        ropt.add_param_group({"params": [p for k, p in ref.named_parameters() if k.endswith("conv.weight")], "weight_decay": wd})
        ropt.add_param_group({"params": [p for k, p in ref.named_parameters() if k.endswith("bn.weight")], "weight_decay": 0.0})
        rema = {k: v.detach().clone() for k, v in ref.state_dict().items() if v.dtype.is_floating_point}
        net = net.cuda().train()
        opt = ydl.smart_optimizer(net, "AdamW", lr, MOM, wd)
        assert type(opt).__name__ == "FlatAdamWEMA"
        x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(6))
        for st in range(3):
            opt.zero_grad()
            net[1](net[0](x.cuda())).square().mean().backward()
            opt.step()
            ropt.zero_grad()
            ref(x).square().mean().backward()
            ropt.step()
            d = _ema_d(st + 1)
            with torch.no_grad():
                msd = ref.state_dict()
                for k, v in rema.items():
                    v *= d
                    v += (1 - d) * msd[k].detach()
        sd, want = net.state_dict(), ref.state_dict()
        ema = opt.ema_state_dict()
        for k, v in want.items():
            if v.dtype.is_floating_point:
                assert rel_err(sd[k].cpu(), v) < 2e-4, k
                assert rel_err(ema[k].cpu(), rema[k]) < 2e-4, k
            else:
                assert torch.equal(sd[k].cpu(), v), k
    finally:
        ydl.set_compute_dtype("bf16")


def _yaml_model(seed=5, size=64):
    import yaml
    import yolo_dual_amd as ydl
    from oracle.fill import fill_state_dict
    cfg = yaml.safe_load(open(os.path.join(CFG, "yolov5_seg.yaml")))
    for sec in ("backbone", "head"):
        for l in cfg[sec]:
            l[2] = {"C3_DCN": "C3", "C2f_DCN": "C2f"}.get(l[2], l[2])
    m = ydl.YOLOv5Seg(cfg)
    m.img_size = [size, size]
    sd = m.state_dict()
    fill_state_dict(sd, seed, bn_stats=False)
    m.load_state_dict(sd)
    return m.cuda().train()


def test_replayed_adam_step_equals_the_eager_step_bit_for_bit():
    """the launch-list replay with Adam on the yaml model, deterministic mode, an lr that changes every step: 3 steps inside the
    constructor (2 warm-up + the recorded one) and 4 replayed ones against the same 7 steps eager — parameters, BatchNorm buffers,
    both state arenas, the EMA shadow and the step counts.  A bias correction or an lr baked into the recording fails this."""
    import yolo_dual_amd as ydl
    from yolo_dual_amd import config
    from yolo_dual_amd.replay import ReplayedTrainStep
    cw = torch.tensor([1, 2, 25, 2, 10, 3, 25, 10, 5, 15, 25, 1], dtype=torch.float32)
    config.set_deterministic(True)
    ydl.set_compute_dtype("f32")
    try:
        res = {}
        for how in ("eager", "replay"):
            m = _yaml_model()
            opt = ydl.smart_optimizer(m, "Adam", 0.002, MOM, WD)
            crit = ydl.SegmentationLoss(12, 0.0, cw, "dice", sync=False)
            gen = torch.Generator("cuda").manual_seed(3)
            xs = [torch.rand(2, 3, 64, 64, device="cuda", generator=gen) for _ in range(3)]
            ts = [torch.randint(0, 12, (2, 64, 64), device="cuda", generator=gen) for _ in range(3)]
            x, t = xs[0].clone(), ts[0].clone()

            def begin(i):
                x.copy_(xs[i % 3]); t.copy_(ts[i % 3])
                for g, lr in zip(opt.param_groups, _lrs(i)):
                    g["lr"] = lr

            losses = []
            if how == "eager":
                for st in range(7):
                    begin(st)
                    opt.zero_grad()
                    total, items = crit(m(x), t)
                    total.backward()
                    opt.step()
                    losses.append(float(items[0]))
            else:
                step_no = [0]

                def pre(_mod, _inp):
                    begin(step_no[0])
                    step_no[0] += 1
                hk = m.register_forward_pre_hook(pre)
                r = ReplayedTrainStep(m, crit, opt, x, t, warmup=2)
                hk.remove()
                assert step_no[0] == 3
                losses = [None, None, float(r.loss_items[0])]
                r.poison()
                for st in range(3, 7):
                    begin(st)
                    losses.append(float(r.step()[0]))
                assert opt.updates == 7
            torch.cuda.synchronize()
            state = {k: v.detach().clone() for k, v in m.state_dict().items()}
            state["__state1"], state["__state2"] = opt.state1_arena.clone(), opt.state2_arena.clone()
            state["__ema"] = opt.ema_arena.clone()
            res[how] = (losses, state, list(opt._steps))
        assert res["eager"][0][2:] == res["replay"][0][2:], (res["eager"][0], res["replay"][0])
        assert res["eager"][2] == res["replay"][2] and max(res["eager"][2]) == 7
        for k, v in res["eager"][1].items():
            assert torch.equal(v, res["replay"][1][k]), k
        assert bool(res["eager"][1]["__state2"].any())
    finally:
        config.set_deterministic(None)
        ydl.set_compute_dtype("bf16")


@pytest.mark.parametrize("name", NAMES)
def test_resume_continues_bit_for_bit(name):
    """2 steps, state_dict through a weights_only file into a fresh optimizer, 2 more steps == 4 straight steps"""
    import yolo_dual_amd as ydl

    def live(k, step):
        return k != "2.weight" and (k != "4.weight" or step >= 1)

    straight, ms = _hip_trajectory(name, live, steps=4)
    a, ma = _hip_trajectory(name, live, steps=2)
    buf = io.BytesIO()
    torch.save({"optimizer": a.state_dict(), "model": ma.state_dict(), "ema": a.ema_state_dict()}, buf)
    buf.seek(0)
    ck = torch.load(buf, weights_only=True)
    assert ck["optimizer"]["format"] == FORMATS[name]
    mb = _flat_model(seed=9).cuda()
    mb.load_state_dict(ck["model"])
    b = ydl.smart_optimizer(mb, name, 0.5, 0.5, 0.0)                 # every hyper-parameter comes from the file
    b.load_state_dict(ck["optimizer"])
    b.load_ema_state_dict(ck["ema"])
    b, mb = _hip_trajectory(name, live, steps=2, opt_and_model=(b, mb), first_step=2)
    assert b._steps == straight._steps and b.updates == straight.updates == 4
    for x, y in ((b.params_arena, straight.params_arena), (b.state1_arena, straight.state1_arena),
                 (b.state2_arena, straight.state2_arena), (b.ema_arena, straight.ema_arena)):
        assert torch.equal(x, y)
    other = [n for n in NAMES if n != name][0]
    with pytest.raises(ValueError):
        ydl.smart_optimizer(_flat_model().cuda(), other, 0.01, 0.9, 0.0).load_state_dict(ck["optimizer"])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import yolo_dual_amd as ydl
        from yolo_dual_amd.parallel import DataParallel
        torch.cuda.set_device(0)
        ydl.set_compute_dtype("bf16")
        m = _yaml_model(seed=11 + rank)                              # replicas start different: the broadcast must fix it
        opt = ydl.smart_optimizer(m, "AdamW", 0.002, MOM, WD, ema=(rank == 0))
        dp = DataParallel(m, opt, bucket_bytes=1 << 20)
        cw = torch.tensor([1, 2, 25, 2, 10, 3, 25, 10, 5, 15, 25, 1], dtype=torch.float32)
        crit = ydl.SegmentationLoss(12, 0.0, cw, "dice", sync=False)
        gen = torch.Generator("cuda").manual_seed(100 + rank)        # different data per rank
        x = torch.rand(2, 3, 64, 64, device="cuda", generator=gen)
        t = torch.randint(0, 12, (2, 64, 64), device="cuda", generator=gen)
        start = opt.params_arena[:opt.n_params].clone()
        for _ in range(3):
            opt.zero_grad()
            dp.begin()
            total, items = crit(m(x), t)
            total.backward()
            opt.step(grad_scale=dp.finish())
        torch.cuda.synchronize()
        n = opt.n_params
        ok = True
        for arena in (opt.params_arena[:n], opt.state1_arena, opt.state2_arena):
            mine = arena.clone()
            ref = mine.clone()
            dist.broadcast(ref, src=0)
            ok = ok and bool(torch.equal(mine, ref)) and bool(torch.isfinite(mine).all())
        ok = ok and not torch.equal(start, opt.params_arena[:n]) and max(opt._steps) == 3
        q.put((rank, "ok" if ok else "fail"))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "fail: " + repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_two_rank_data_parallel_adamw():
    """two ranks on one GPU (gloo transport, all-reduce): after 3 AdamW steps the replicas' parameters and both state arenas are
    bit-equal"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=280) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == "ok" for r in res), res


def test_train_cli_with_adamw_saves_and_resumes(tmp_path):
    import train_seg
    import yolo_dual_amd as ydl
    sd = str(tmp_path / "run")
    common = ["--cfg", os.path.join(CFG, "yolov5_seg.yaml"), "--batch-size", "2", "--imgsz", "64", "--steps-per-epoch", "4",
              "--save-dir", sd, "--dtype", "f32", "--optimizer", "AdamW"]
    try:
        fit = train_seg.train(train_seg.parse_opt(common + ["--epochs", "1"]))
        assert 0.0 <= fit <= 1.0 and math.isfinite(float(train_seg.LAST_RUN["loss"]))
        last = os.path.join(sd, "last.pt")
        ck = ydl.load_checkpoint(last)
        assert ck["optimizer"]["format"] == "ydl-flat-adamw-ema-1" and ck["epoch"] == 0
        assert int(ck["optimizer"]["steps"].max()) >= 1 and bool(ck["optimizer"]["state2"].any())
        fit2 = train_seg.train(train_seg.parse_opt(common + ["--epochs", "2", "--weights", last, "--resume"]))
        assert ydl.load_checkpoint(last)["epoch"] == 1 and 0.0 <= fit2 <= 1.0
        with pytest.raises(SystemExit):
            train_seg.parse_opt(common[:-1] + ["Lion"])
    finally:
        ydl.set_compute_dtype("bf16")
