"""GPU: the training step of YOLOv5Seg with native C3_DCN blocks replays from the launch list (the step stays ATen-free):
forward bit-equal to the eager step, gradients equal to atomic-order rounding (the pattern of
test_gpu_replay.py::test_replayed_step_of_the_dcnv3_model)."""
import os

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu


def _setup():
    import yolo_dual_amd as ydl
    from oracle.fill import fill_state_dict
    ydl.set_compute_dtype("bf16")
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "..", "yolo_dual_amd", "cfg", "yolov5_seg.yaml")))
    m = ydl.YOLOv5Seg(cfg, deformable=True)
    m.img_size = [128, 128]
    sd = m.state_dict()
    fill_state_dict(sd, 5, bn_stats=False)
    m.load_state_dict(sd)
    m = m.cuda().train()
    opt = ydl.FlatSGDEMA(m, lr=0.01, momentum=0.937, weight_decay=5e-4)
    crit = ydl.SegmentationLoss(12, 0.0, torch.ones(12), "dice", sync=False)
    gen = torch.Generator("cuda").manual_seed(3)
    xs = [torch.rand(4, 3, 128, 128, device="cuda", generator=gen) for _ in range(2)]
    ts = [torch.randint(0, 12, (4, 128, 128), device="cuda", generator=gen) for _ in range(2)]
    return m, opt, crit, xs, ts


def test_replayed_step_of_the_native_dcn_model():
    import yolo_dual_amd as ydl
    from yolo_dual_amd import config
    from yolo_dual_amd.replay import ReplayedTrainStep
    from tests.util import l2_err
    config.set_deterministic(True)
    try:
        mA, oA, cA, xs, ts = _setup()
        mB, oB, cB, _, _ = _setup()
        x, t = xs[0].clone(), ts[0].clone()
        r = ReplayedTrainStep(mB, cB, oB, x, t, warmup=2)
        r.poison()
        r.step()
        with torch.no_grad():
            oA.params_arena.copy_(oB.params_arena); oA.mom_arena.copy_(oB.mom_arena); oA.ema_arena.copy_(oB.ema_arena)
        oA._has_buf = {id(pa): oB._has_buf.get(id(pb), False) for (pa, *_a), (pb, *_b) in zip(oA._slots, oB._slots)}
        config.bump_weight_epoch()
        x.copy_(xs[1]); t.copy_(ts[1])
        eager = []
        for _ in range(3):
            oA.zero_grad()
            total, items = cA(mA(x), t)
            total.backward()
            torch.cuda.synchronize()
            eager.append(oA.grads_arena.detach().cpu().clone())
        noise = max(l2_err(eager[1], eager[0]), l2_err(eager[2], eager[0]))
        oB.prepare_step(1.0)
        r.rec.run(0, r._n_fb)
        torch.cuda.synchronize()
        assert float(items[0]) == float(r.loss_items[0])
        got = l2_err(oB.grads_arena.cpu(), eager[0])
        print(f"[replay deform] gradient arena: replay vs eager {got:.2e}, eager vs eager {noise:.2e}")
        assert got <= 3 * noise + 1e-6, (got, noise)
    finally:
        config.set_deterministic(None)
        ydl.set_compute_dtype("bf16")
