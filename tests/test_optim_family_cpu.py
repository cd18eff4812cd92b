"""CPU: the Adam / AdamW / RMSProp branches of ``smart_optimizer`` (utils/torch_utils.py:318-346) — construction without a kernel,
the parameter groups a scheduler or user code sees, the checkpoint state, and the host-side argument validation of the new entry
points."""
import ctypes
import io

import pytest
import torch
import torch.nn as nn

NAMES = ("Adam", "AdamW", "RMSProp")
FORMATS = {"Adam": "ydl-flat-adam-ema-1", "AdamW": "ydl-flat-adamw-ema-1", "RMSProp": "ydl-flat-rmsprop-ema-1"}


def _model():
    torch.manual_seed(0)
    return nn.Sequential(nn.Conv2d(3, 4, 3, bias=True), nn.BatchNorm2d(4), nn.Conv2d(4, 2, 1, bias=False))


def _torch_reference(model, name, lr, momentum, decay):
    """what the reference's smart_optimizer builds, on the same grouping"""
    g0 = [model[0].weight, model[2].weight]
    g1 = [model[1].weight]
    g2 = [model[0].bias, model[1].bias]
    if name == "Adam":
        o = torch.optim.Adam(g2, lr=lr, betas=(momentum, 0.999))
    elif name == "AdamW":
        o = torch.optim.AdamW(g2, lr=lr, betas=(momentum, 0.999), weight_decay=0.0)
    else:
        o = torch.optim.RMSprop(g2, lr=lr, momentum=momentum)
    o.add_param_group({"params": g0, "weight_decay": decay})
    o.add_param_group({"params": g1, "weight_decay": 0.0})
    return o


@pytest.mark.parametrize("name", NAMES)
def test_smart_optimizer_builds_the_reference_groups(name):
    import yolo_dual_amd as ydl
    m = _model()
    opt = ydl.smart_optimizer(m, name, 0.004, 0.937, 5e-4)
    assert isinstance(opt, ydl.FlatArenaOptimizer) and isinstance(opt, torch.optim.Optimizer)
    ref = _torch_reference(_model(), name, 0.004, 0.937, 5e-4)
    assert len(opt.param_groups) == 3
    keys = ("lr", "betas", "eps", "weight_decay") if name != "RMSProp" else ("lr", "alpha", "eps", "momentum", "weight_decay", "centered")
    for g, r in zip(opt.param_groups, ref.param_groups):
        assert [tuple(p.shape) for p in g["params"]] == [tuple(p.shape) for p in r["params"]]
        for k in keys:
            assert g[k] == r[k], (k, g[k], r[k])
    if name != "RMSProp":
        assert opt.param_groups[1]["betas"][0] == 0.937
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 5e-4, 0.0]
    # the consumers' protocol
    assert opt.n_params == sum(p.numel() for p in m.parameters()) and opt.n_total > opt.n_params
    assert opt.params_arena.numel() == opt.n_total == opt.ema_arena.numel() and opt.grads_arena.numel() == opt.n_params
    assert opt.state1_arena.numel() == opt.n_params == opt.state2_arena.numel()
    assert len(opt._slots) == 5 and opt.updates == 0 and opt.live_ranges() == []
    for attr in ("zero_grad", "reattach", "step", "ensure_hyper", "ensure_runs_table", "prepare_step", "step_device_hyper",
                 "ema_state_dict", "load_ema_state_dict"):
        assert callable(getattr(opt, attr)), attr
    assert set(opt.ema_state_dict()) == set(m.state_dict())


def test_unknown_optimizer_name_raises_like_the_reference():
    import yolo_dual_amd as ydl
    with pytest.raises(NotImplementedError, match="Optimizer Lion not implemented."):
        ydl.smart_optimizer(_model(), "Lion", 0.01, 0.9, 0.0)
    assert type(ydl.smart_optimizer(_model(), "SGD", 0.01, 0.9, 0.0)).__name__ == "FlatSGDEMA"


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_round_trips_through_a_weights_only_file(name):
    import yolo_dual_amd as ydl
    a = ydl.smart_optimizer(_model(), name, 0.004, 0.937, 5e-4)
    gen = torch.Generator().manual_seed(1)
    a.state1_arena.copy_(torch.randn(a.n_params, generator=gen))
    a.state2_arena.copy_(torch.rand(a.n_params, generator=gen))
    a._steps = [3, 0, 7, 7, 1]
    a.updates = 9
    a.param_groups[1]["lr"] = 0.123
    sd = a.state_dict()
    assert sd["format"] == FORMATS[name]
    buf = io.BytesIO()
    torch.save({"optimizer": sd}, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=True)["optimizer"]
    b = ydl.smart_optimizer(_model(), name, 0.01, 0.9, 0.0)
    b.load_state_dict(back)
    assert torch.equal(a.state1_arena, b.state1_arena) and torch.equal(a.state2_arena, b.state2_arena)
    assert b._steps == [3, 0, 7, 7, 1] and b.updates == 9
    for ga, gb in zip(a.param_groups, b.param_groups):
        assert {k: v for k, v in ga.items() if k != "params"} == {k: v for k, v in gb.items() if k != "params"}
    assert b.param_groups[1]["lr"] == 0.123 and b.param_groups[1]["weight_decay"] == 5e-4


def test_state_of_another_rule_or_model_is_refused():
    import yolo_dual_amd as ydl
    opts = {n: ydl.smart_optimizer(_model(), n, 0.01, 0.9, 1e-5) for n in NAMES + ("SGD",)}
    for src in opts:
        for dst in opts:
            if src != dst:
                with pytest.raises(ValueError):
                    opts[dst].load_state_dict(opts[src].state_dict())
    other = ydl.smart_optimizer(nn.Sequential(nn.Conv2d(3, 5, 3), nn.BatchNorm2d(5)), "Adam", 0.01, 0.9, 1e-5)
    with pytest.raises(ValueError, match="different model"):
        opts["Adam"].load_state_dict(other.state_dict())


def test_new_entry_points_validate_on_the_host():
    """null pointers, a bad arena partition, an unknown rule, a bad class / lr index, too many runs and arenas of the run-table
    forms (the family's and SGD's) that are not 16-byte aligned are refused before any launch"""
    from yolo_dual_amd import _lib as L
    lib = L.lib()
    vp = ctypes.c_void_p
    buf = (ctypes.c_float * 64)()
    ptr = vp(ctypes.addressof(buf))
    sc = [0.1, 1.0, 1.0, 0.0, 0.9, 0.999, 0.1, 0.001, 1e-8, 1.0, -1.0]

    def err():
        return lib.ydl_last_error().decode()

    assert lib.ydl_optim_ema_step(L.OPT_ADAM, None, ptr, ptr, ptr, None, 0, 4, 4, *sc, None) != 0 and "null pointer" in err()
    assert lib.ydl_optim_ema_step(L.OPT_ADAM, ptr, ptr, ptr, None, None, 0, 4, 4, *sc, None) != 0 and "null pointer" in err()
    assert lib.ydl_optim_ema_step(L.OPT_ADAMW, ptr, ptr, ptr, ptr, None, 5, 4, 4, *sc, None) != 0 and "partition" in err()
    assert lib.ydl_optim_ema_step(L.OPT_RMSPROP, ptr, ptr, ptr, ptr, None, 0, 9, 4, *sc, None) != 0 and "partition" in err()
    assert lib.ydl_optim_ema_step(0, ptr, ptr, ptr, ptr, None, 0, 4, 4, *sc, None) != 0 and "rule" in err()
    assert lib.ydl_optim_ema_step(4, ptr, ptr, ptr, ptr, None, 0, 4, 4, *sc, None) != 0 and "rule" in err()
    assert lib.ydl_optim_ema_step_dev(L.OPT_ADAM, ptr, ptr, ptr, ptr, None, 0, 4, 4, None, 0, 0, 0, 0, None) != 0 and "null pointer" in err()
    assert lib.ydl_optim_ema_step_dev(L.OPT_ADAM, ptr, ptr, ptr, ptr, None, 0, 4, 2, ptr, 0, 0, 0, 0, None) != 0 and "partition" in err()
    assert lib.ydl_optim_ema_step_dev(L.OPT_ADAM, ptr, ptr, ptr, ptr, None, 0, 4, 4, ptr, 3, 0, 0, 0, None) != 0 and "lr index" in err()
    assert lib.ydl_optim_ema_step_dev(L.OPT_ADAM, ptr, ptr, ptr, ptr, None, 0, 4, 4, ptr, 0, L.OPT_MAX_CLASSES, 0, 0, None) != 0
    assert lib.ydl_optim_ema_step_dev(7, ptr, ptr, ptr, ptr, None, 0, 4, 4, ptr, 0, 0, 0, 0, None) != 0 and "rule" in err()
    assert lib.ydl_optim_ema_step_multi(L.OPT_ADAM, ptr, ptr, ptr, ptr, None, None, 1, 4, ptr, 0, None) != 0 and "null pointer" in err()
    assert lib.ydl_optim_ema_step_multi(L.OPT_ADAM, ptr, ptr, ptr, ptr, None, ptr, 65536, 4, ptr, 0, None) != 0 and "run count" in err()
    assert lib.ydl_optim_ema_step_multi(L.OPT_ADAM, ptr, ptr, ptr, ptr, None, ptr, 0, 4, ptr, 0, None) != 0 and "run count" in err()
    assert lib.ydl_optim_ema_step_multi(-1, ptr, ptr, ptr, ptr, None, ptr, 1, 4, ptr, 0, None) != 0 and "rule" in err()
    off4 = vp(ctypes.addressof(buf) + 4)
    assert lib.ydl_optim_ema_step_multi(L.OPT_ADAM, off4, ptr, ptr, ptr, None, ptr, 1, 4, ptr, 0, None) != 0 and "aligned" in err()
    assert lib.ydl_sgd_ema_step_multi(off4, ptr, ptr, None, ptr, 1, 4, ptr, 0, None) != 0 and "aligned" in err()


def test_host_numbers_follow_torch_in_double_precision():
    """the factors the kernels receive: lr / (1 - beta1^t) and sqrt(1 - beta2^t) exactly as torch's single-tensor Adam forms them, a
    class per distinct step count in ascending order, runs split where the step count changes"""
    import yolo_dual_amd as ydl
    from yolo_dual_amd import config
    m = _model()
    opt = ydl.smart_optimizer(m, "Adam", 0.004, 0.937, 5e-4, ema=False)
    for t in (1, 2, 5, 1000):
        step_size, bc2s = opt._corrections(t, 0.004)
        assert step_size == 0.004 / (1 - 0.937 ** t) and bc2s == (1 - 0.999 ** t) ** 0.5
    rms = ydl.smart_optimizer(_model(), "RMSProp", 0.004, 0.937, 5e-4, ema=False)
    assert rms._corrections(7, 0.004) == (0.004, 1.0)
    for p, *_r in opt._slots:
        config.mark_touched(p)
    opt._steps = [4, 1, 4, 4, 4]         # the second decay weight got its first gradient three steps late
    assert opt._classes() == {1: 0, 4: 1}
    rows = opt._run_rows(opt._runs())
    assert [r[6] for r in rows] == [1, 0, 1, 1] and [r[4] for r in rows] == [0, 0, 1, 2]
    assert sum(r[3] for r in rows) == opt.n_params and all(r[1] in (0, r[2]) for r in rows)
