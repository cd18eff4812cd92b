"""The fused replicated tail (ydl_seg_tail_fwd / ydl_seg_tail_bwd) wired into the model: YOLOv5Seg at 2 x 64^2, f32 parity mode,
deterministic weight gradients.  The step with config.set_fused_seg_tail(True) is compared with the same step with the switch off (the
five-launch form): which entry points are issued, the loss, every parameter gradient; the recorded step replays bit for bit; a second
loss on the prediction and a prediction with another consumer still give the switch-off gradients.

Bounds between the two forms.  Loss: rtol 2e-6, what tests/test_gpu_blocks.py::test_loss_replicated_matches_full allows between two
associations of the same float32 sums.  Gradients: the backward of the model is linear in the gradient of the logits, and the two
forms differ only through the merged sums behind it, so the suite's path-against-path figure applies: 2e-4 of the largest entry
(test_loss_fast_path_survives_only_untouched_predictions), here per parameter; a parameter whose whole gradient is below 1e-3 of the
largest entry of any parameter is float32 cancellation noise in either run and is compared on that scale instead of its own."""
import os

import pytest
import torch
import yaml

from oracle.fill import fill_state_dict
from tests.block_harness import train_state

pytestmark = pytest.mark.gpu
CW = torch.tensor([1, 2, 25, 2, 10, 3, 25, 10, 5, 15, 25, 1], dtype=torch.float32)
S, BS = 64, 2
STORED = ("ydl_seg_loss_rep_fwd", "ydl_seg_loss_rep_bwd", "ydl_softmax_bwd")


def _model():
    import yolo_dual_amd as ydl
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(ydl.__file__), "cfg", "yolov5_seg.yaml")))
    for sec in ("backbone", "head"):
        for l in cfg[sec]:
            l[2] = "C3" if l[2] == "C3_DCN" else l[2]
    m = ydl.YOLOv5Seg(cfg)
    m.img_size = [S, S]
    sd = m.state_dict()
    fill_state_dict(sd, 5, bn_stats=False)
    m.load_state_dict(sd)
    return m.cuda().train()


def _batch():
    gen = torch.Generator("cuda").manual_seed(3)
    x = torch.rand(BS, 3, S, S, device="cuda", generator=gen)
    t = torch.randint(0, 12, (BS, S, S), device="cuda", generator=gen)
    t[0, :9, :13] = 255                                  # labels outside [0, C): no class
    extra = torch.randn(BS, 12, S, S, device="cuda", generator=gen)
    return x, t, extra


@pytest.fixture
def parity():
    import yolo_dual_amd as ydl
    from yolo_dual_amd import config
    ydl.set_compute_dtype("f32")
    config.set_deterministic(True)
    was = config.fused_seg_tail()
    yield config
    config.set_fused_seg_tail(was)
    config.set_deterministic(None)
    ydl.set_compute_dtype("bf16")


def _step(config, fused, scenario, monkeypatch):
    """one forward + backward -> (total, {parameter name: gradient}, [(entry point, arguments)])"""
    import yolo_dual_amd as ydl
    from yolo_dual_amd import _lib as L
    config.set_fused_seg_tail(fused)
    m = _model()
    x, t, extra = _batch()
    calls = []
    real = L.call

    def logged(name, *args):
        calls.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(L, "call", logged)
    crit = ydl.SegmentationLoss(12, 0.0, CW, "dice", sync=False)
    pred = m(x)
    total, _ = crit(pred, t)
    if scenario == "second_loss":
        total = total + ydl.SegmentationLoss(12, 0.1, None, "jaccard", sync=False)(pred, t)[0]
    elif scenario == "other_consumer":
        total = total + (pred * extra).sum() * 1e-3
    total.backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(L, "call", real)
    grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
    return float(total.detach()), grads, calls


def _names(calls):
    return [n for n, _ in calls]


def _stored_softmax_fwd(calls):
    """ydl_softmax_fwd launches at the stored resolution (rep_h = rep_w = 1; the dense export replicates)"""
    return [a for n, a in calls if n == "ydl_softmax_fwd" and (int(a[12]), int(a[13])) == (1, 1)]


def _compare(on, off):
    (ta, ga, _), (tb, gb, _) = on, off
    print(f"  total: fused {ta!r} switch-off {tb!r}")
    assert abs(ta - tb) <= 2e-6 * abs(tb), (ta, tb)
    assert ga.keys() == gb.keys()
    gmax = max(float(g.abs().max()) for g in gb.values())
    worst = 0.0
    for n in gb:
        scale = max(float(gb[n].abs().max()), 1e-3 * gmax)
        e = float((ga[n].double() - gb[n].double()).abs().max()) / scale
        worst = max(worst, e)
        assert e < 2e-4, (n, e)
    print(f"  parameter gradients: worst max-norm difference {worst:.2e} of the parameter's scale ({len(gb)} parameters)")


def test_fused_tail_replaces_the_stored_resolution_launches(parity, monkeypatch):
    on = _step(parity, True, "plain", monkeypatch)
    off = _step(parity, False, "plain", monkeypatch)
    n_on, n_off = _names(on[2]), _names(off[2])
    assert n_on.count("ydl_seg_tail_fwd") == 1 and n_on.count("ydl_seg_tail_bwd") == 1, n_on
    assert not _stored_softmax_fwd(on[2])
    for name in STORED:
        assert name not in n_on, name
    # the switch selects the five-launch form
    assert "ydl_seg_tail_fwd" not in n_off and "ydl_seg_tail_bwd" not in n_off
    assert len(_stored_softmax_fwd(off[2])) == 1
    for name in STORED:
        assert n_off.count(name) == 1, name
    assert len(n_on) == len(n_off) - 2
    _compare(on, off)


@pytest.mark.parametrize("scenario", ["second_loss", "other_consumer"])
def test_fused_tail_falls_back_where_the_prediction_has_other_consumers(scenario, parity, monkeypatch):
    """the dense gradient of the other consumer and the replica-summed one of the first loss are folded as before; the stored
    probabilities are computed on demand for it"""
    on = _step(parity, True, scenario, monkeypatch)
    off = _step(parity, False, scenario, monkeypatch)
    n_on = _names(on[2])
    assert n_on.count("ydl_seg_tail_fwd") == 1 and "ydl_seg_tail_bwd" not in n_on
    assert len(_stored_softmax_fwd(on[2])) == 1 and n_on.count("ydl_seg_loss_rep_bwd") == 1
    _compare(on, off)


def test_default_keeps_the_five_launch_form_below_the_size_threshold(parity, monkeypatch):
    """512 stored pixels: far under config.SEG_TAIL_MIN_PIXELS, so the unforced switch leaves the step as the launch-trace fixture has it"""
    names = _names(_step(parity, None, "plain", monkeypatch)[2])
    assert "ydl_seg_tail_fwd" not in names and "ydl_seg_tail_bwd" not in names
    for name in STORED:
        assert names.count(name) == 1, name


def test_fused_tail_replays_bit_for_bit(parity):
    import yolo_dual_amd as ydl
    from yolo_dual_amd.replay import ReplayedTrainStep
    parity.set_fused_seg_tail(True)
    x0, t0, _ = _batch()
    res = {}
    for how in ("eager", "replay"):
        m = _model()
        opt = ydl.FlatSGDEMA(m, lr=0.01, momentum=0.937, weight_decay=5e-4)
        crit = ydl.SegmentationLoss(12, 0.0, CW, "dice", sync=False)
        x, t = x0.clone(), t0.clone()
        losses = []
        if how == "eager":
            for _ in range(5):
                opt.zero_grad()
                total, items = crit(m(x), t)
                total.backward()
                opt.step()
                losses.append(float(items[0]))
        else:
            r = ReplayedTrainStep(m, crit, opt, x, t, warmup=2)          # two eager steps and the recorded one
            losses = [None, None, float(r.loss_items[0])]
            r.poison()
            for _ in range(2):
                losses.append(float(r.step()[0]))
        torch.cuda.synchronize()
        res[how] = (losses, train_state(m, opt))
    assert res["eager"][0][2:] == res["replay"][0][2:], (res["eager"][0], res["replay"][0])
    for k, v in res["eager"][1].items():
        assert torch.equal(v, res["replay"][1][k]), k
