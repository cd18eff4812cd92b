"""GPU parity: every block of the hot path, through the nn.Module facade and the C ABI, against the golden vectors
the reference's own classes produced (tests/golden, oracle/make_golden.py) and against the CPU oracle.

Tolerances (max-abs error relative to the reference tensor's max-abs):
  f32 mode  — outputs 1e-4 (north_star: fp32 logits within 1e-4 relative), gradients 5e-4, BN running stats 1e-4;
  bf16 mode — outputs 3e-2, gradients 0.15 in relative L2 norm (bf16 storage has 8 mantissa bits; validated end-to-end by loss curves).
Index arithmetic (nearest upsample, concat copy) is checked bit-exact in f32 mode."""
import numpy as np
import pytest
import torch

from tests.util import Golden, l2_err, names, rel_err

pytestmark = pytest.mark.gpu

TOL = {"f32": dict(out=1e-4, gx=5e-4, gp=1e-3, stat=1e-4), "bf16": dict(out=3e-2, gx=0.15, gp=0.15, stat=2e-2)}


@pytest.fixture(params=["f32", "bf16"])
def mode(request):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype(request.param)
    yield request.param
    ydl.set_compute_dtype("bf16")


def _load(mod, g):
    sd = g.group("sd") if not g.has("sd_keys") else g.rebuild_sd()
    mod.load_state_dict(sd)
    return mod.cuda().train()


def _run(mod, g, mode, n_in=1, as_list=False, tie_prone=False):
    """tie_prone: max-pool blocks in bf16 mode — bf16 rounding creates ties, so single gradients are routed to a
    different (equal-valued) window element than in the f32 reference; gradients are then compared in L2 norm."""
    xs = [g.t(f"x{i}").cuda().requires_grad_(True) for i in range(n_in)]
    out = mod(xs) if as_list else mod(*xs)
    t = dict(TOL[mode])
    # bf16 mode: gradients are compared in relative L2 norm — a bf16-rounded activation that lands on the other side
    # of a ReLU kink or ties inside a max-pool window re-routes single gradient elements without changing the fit
    rel_err_ = l2_err if mode == "bf16" else rel_err
    if tie_prone and mode == "bf16":
        t.update(gx=0.35, gp=0.35)
    ref = g.t("out")
    assert out.shape == ref.shape
    assert out.dtype == torch.float32
    assert rel_err(out.detach().cpu(), ref) < t["out"], (g.name, "out", rel_err(out.detach().cpu(), ref))
    (out * g.t("gup").cuda()).sum().backward()
    torch.cuda.synchronize()
    for i, x in enumerate(xs):
        if g.has(f"gx{i}"):
            e = rel_err_(x.grad.cpu(), g.t(f"gx{i}"))
            assert e < t["gx"], (g.name, f"gx{i}", e)
    sd = dict(mod.named_parameters())
    if g.has("grad_names"):
        for k, n in zip(g.strs("grad_names"), g.flat["grad_norms"]):
            got = float(sd[k].grad.double().norm())
            assert abs(got - n) <= t["gp"] * max(n, 1e-6), (g.name, k, got, n)
    else:
        for k, v in g.group("grad").items():
            e = rel_err_(sd[k].grad.cpu(), v)
            assert e < t["gp"], (g.name, k, e)
    after = mod.state_dict()
    for k, v in g.group("sd_after").items():
        if v.dtype.is_floating_point:
            e = rel_err(after[k].cpu(), v)
            assert e < t["stat"], (g.name, k, e)
        else:
            assert torch.equal(after[k].cpu(), v), (g.name, k)
    return out


@pytest.mark.parametrize("name", names("v5_conv_"))
def test_conv(name, mode):
    import yolo_dual_amd as ydl
    g = Golden(name)
    c1, c2, k, s, p, act = [int(v) for v in g.flat["meta"]]
    m = _load(ydl.Conv(c1, c2, k, s, None if p < 0 else p, 1, bool(act)), g)
    _run(m, g, mode)


@pytest.mark.parametrize("name", names("v5_c3_"))
def test_c3_script(name, mode):
    import yolo_dual_amd as ydl
    g = Golden(name)
    c1, c2, n = [int(v) for v in g.flat["meta"]]
    m = ydl.C3(c1, c2, n, False) if "noshortcut" in name else ydl.C3(c1, c2, n)
    _run(_load(m, g), g, mode)


@pytest.mark.parametrize("name", names("v5_sppf") + ["cm_sppf"])
def test_sppf(name, mode):
    import yolo_dual_amd as ydl
    g = Golden(name)
    sd = g.group("sd")
    c1 = sd["cv1.conv.weight"].shape[1]
    c2 = sd["cv2.conv.weight"].shape[0]
    _run(_load(ydl.SPPF(c1, c2, 5), g), g, mode, tie_prone=True)


@pytest.mark.parametrize("name", ["cm_bottleneck", "cm_c3_n1", "cm_c3_n2"])
def test_common_blocks(name, mode):
    import yolo_dual_amd as ydl
    g = Golden(name)
    if name == "cm_bottleneck":
        m = ydl.Bottleneck(16, 16, True)
    else:
        c1, c2, n = [int(v) for v in g.flat["meta"]]
        m = ydl.C3Common(c1, c2, n)
    _run(_load(m, g), g, mode)


@pytest.mark.parametrize("name", names("v8_c2f_"))
def test_c2f(name, mode):
    import yolo_dual_amd as ydl
    g = Golden(name)
    c1, c2, n = [int(v) for v in g.flat["meta"]]
    _run(_load(ydl.C2f(c1, c2, n), g), g, mode)


def test_c3k2(mode):
    import yolo_dual_amd as ydl
    g = Golden("v9_c3k2")
    _run(_load(ydl.C3k2(16, 16, 1), g), g, mode)


def test_gam(mode):
    import yolo_dual_amd as ydl
    g = Golden("v9_gam")
    m = _load(ydl.GAM(int(g.flat["meta"][0])), g)
    # the pooled branches run BatchNorm over 2 values per channel (batch 2 at 1x1): bf16 rounding of those inputs is
    # amplified without bound, so the bf16 mode only checks that the block runs and stays finite
    if mode == "bf16":
        x = g.t("x0").cuda().requires_grad_(True)
        out = m(x)
        out.sum().backward()
        assert torch.isfinite(out).all() and torch.isfinite(x.grad).all()
        return
    _run(m, g, mode)


def test_gam_bf16_against_the_oracle_at_a_batch_of_64():
    """GAM (seg_diceloss_yolov9.py:475-510) in throughput mode with a bound: at batch 64 its pooled branches run BatchNorm over 64
    values per channel (the golden fixture has 2, where bf16 rounding is amplified without bound).  Reference = oracle.ref_cpu.gam
    in f32 on the bf16-rounded input and weights; output 3e-2 and gradients 0.1 in relative L2 (the block is x * sigmoid(gate):
    a bf16-rounded gate moves every element of a channel together)."""
    import numpy as np
    import yolo_dual_amd as ydl
    from oracle import ref_cpu as R
    from oracle.fill import fill_state_dict
    from tests.util import l2_err
    ydl.set_compute_dtype("bf16")
    C, N, H, W = 64, 64, 8, 8
    m = ydl.GAM(C)
    sd = m.state_dict()
    fill_state_dict(sd, 21, bn_stats=False)
    for k in sd:
        if sd[k].dim() == 4:
            sd[k] = sd[k].bfloat16().float()
    m.load_state_dict(sd)
    m = m.cuda().train()
    rs = np.random.RandomState(5)
    x = torch.from_numpy((rs.standard_normal((N, C, H, W)) + 0.2).astype(np.float32)).bfloat16().float()
    gup = torch.from_numpy(rs.standard_normal((N, C, H, W)).astype(np.float32))
    xg = x.cuda().requires_grad_(True)
    out = m(xg)
    (out * gup.cuda()).sum().backward()
    torch.cuda.synchronize()
    ps = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}
    run = {"g." + k: v.clone() for k, v in sd.items()}
    run.update({"g." + k: v for k, v in ps.items()})
    xr = x.clone().requires_grad_(True)
    o = R.gam(run, "g", xr)
    (o * gup).sum().backward()
    assert l2_err(out.detach().cpu(), o.detach()) < 3e-2, l2_err(out.detach().cpu(), o.detach())
    assert l2_err(xg.grad.detach().cpu(), xr.grad) < 0.1, l2_err(xg.grad.detach().cpu(), xr.grad)
    named = dict(m.named_parameters())
    errs = {k: l2_err(named[k].grad.detach().float().cpu(), p.grad) for k, p in ps.items() if p.grad is not None}
    assert errs and max(errs.values()) < 0.1, sorted(errs.items(), key=lambda kv: -kv[1])[:4]


@pytest.mark.parametrize("name", ["r18_basic", "r18_basic_down", "r50_bneck", "r50_bneck_down"])
def test_resnet_blocks(name, mode):
    import yolo_dual_amd as ydl
    g = Golden(name)
    a, b, stride = [int(v) for v in g.flat["meta"]]
    if name.startswith("r18"):
        ds = ydl.Conv(a, b, 1, stride, 0, act=False) if "down" in name else None
        m = ydl.BasicBlock(a, b, stride, ds)
    else:
        ds = ydl.Conv(a, b * 4, 1, stride, 0, act=False) if "down" in name else None
        m = ydl.BottleneckBlock(a, b, stride, ds)
    _run(_load(m, g), g, mode)


def test_resnet_stem(mode):
    import torch.nn as nn
    import yolo_dual_amd as ydl
    from yolo_dual_amd.modules import YdlModule

    class Stem(YdlModule):
        def __init__(self):
            super().__init__()
            self.add_module("0", ydl.Conv(3, 16, 7, 2, 3))
            self.add_module("1", ydl.MaxPool2d(3, 2, 1))

        def _fwd(self, tape, x):
            return getattr(self, "1")._fwd(tape, getattr(self, "0")._fwd(tape, x))

    g = Golden("r18_stem")
    _run(_load(Stem(), g), g, mode, tie_prone=True)


def test_segment_head(mode):
    import yolo_dual_amd as ydl
    g = Golden("seghead")
    m = _load(ydl.SegmentHead(12, [16, 24, 32]), g)
    _run(m, g, mode, n_in=3, as_list=True)


@pytest.mark.parametrize("name", names("v5_concat_"))
def test_concat(name, mode):
    import yolo_dual_amd as ydl
    g = Golden(name)
    m = ydl.Concat(1).cuda()
    xs = [g.t(f"x{i}").cuda().requires_grad_(True) for i in range(2)]
    out = m(xs)
    t = TOL[mode]
    if mode == "f32":
        c0 = xs[0].shape[1]
        assert torch.equal(out[:, :c0].cpu(), g.t("out")[:, :c0])        # pass-through slice: bit-exact copy
        if "same" in name:
            assert torch.equal(out.cpu(), g.t("out"))
    assert rel_err(out.detach().cpu(), g.t("out")) < t["out"]
    (out * g.t("gup").cuda()).sum().backward()
    for i, x in enumerate(xs):
        assert rel_err(x.grad.cpu(), g.t(f"gx{i}")) < t["gx"], (name, i)


@pytest.mark.parametrize("name", names("v5_upsample_"))
def test_upsample_nearest(name, mode):
    import yolo_dual_amd as ydl
    g = Golden(name)
    m = ydl.Upsample(scale_factor=float(name[-1]), mode="nearest").cuda()
    x = g.t("x0").cuda().requires_grad_(True)
    out = m(x)
    if mode == "f32":
        assert torch.equal(out.cpu(), g.t("out"))                         # index arithmetic bit-exact
    assert rel_err(out.detach().cpu(), g.t("out")) < TOL[mode]["out"]
    (out * g.t("gup").cuda()).sum().backward()
    assert rel_err(x.grad.cpu(), g.t("gx0")) < TOL[mode]["gx"]


@pytest.mark.parametrize("name", names("bilinear_"))
def test_bilinear(name, mode):
    import yolo_dual_amd as ydl
    g = Golden(name)
    ac = name.endswith("ac1")
    size = tuple(g.t("out").shape[2:])
    m = ydl.Upsample(size=size, mode="bilinear", align_corners=ac).cuda()
    x = g.t("x0").cuda().requires_grad_(True)
    out = m(x)
    tol = 2e-6 if mode == "f32" else TOL[mode]["out"]
    assert rel_err(out.detach().cpu(), g.t("out")) < tol
    (out * g.t("gup").cuda()).sum().backward()
    assert rel_err(x.grad.cpu(), g.t("gx0")) < (1e-5 if mode == "f32" else TOL[mode]["gx"])


@pytest.mark.parametrize("name", names("loss_"))
def test_losses(name):
    import yolo_dual_amd as ydl
    g = Golden(name)
    logits = g.t("logits").cuda().requires_grad_(True)
    pred = logits.softmax(1) if int(g.flat["softmax_in"]) else logits
    cw = g.t("cw")
    kind = "jaccard" if "jaccard" in name else "dice"
    crit = ydl.SegmentationLoss(pred.shape[1], float(g.flat["ls"]), cw if cw.numel() else None, kind)
    total, items = crit(pred, g.t("target").cuda())
    ref = g.flat["items"]
    for a, b in zip(items, ref):
        assert abs(a - b) <= 1e-4 * abs(b), (name, items, ref)           # north_star: loss within 1e-4 relative
    assert abs(float(total) - ref[0]) <= 1e-4 * abs(ref[0])
    total.backward()
    assert rel_err(logits.grad.cpu(), g.t("glogits")) < 1e-4


def test_loss_nhwc_strides():
    """the kernel takes arbitrary (n,c,h,w) strides: channels_last predictions give the same numbers"""
    import yolo_dual_amd as ydl
    g = Golden("loss_dice_w")
    logits = g.t("logits").cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    crit = ydl.SegmentationLoss(12, 0.0, g.t("cw"), "dice")
    total, items = crit(logits, g.t("target").cuda())
    assert abs(items[0] - g.flat["items"][0]) <= 1e-4 * abs(g.flat["items"][0])
    total.backward()
    assert rel_err(logits.grad.cpu(), g.t("glogits")) < 1e-4


@pytest.mark.parametrize("kind,ls,rep", [("dice", 0.0, (4, 4)), ("jaccard", 0.1, (2, 3)), ("dice", 0.05, (4, 2))])
def test_loss_replicated_matches_full(kind, ls, rep):
    """ydl_seg_loss_rep_* (one thread per stored pixel of a nearest-replicated prediction, labels counted per class)
    == the full-resolution kernels on the materialised replication: same losses, and dlow == replica-sum of dpred."""
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.tape import _p, _stream
    torch.manual_seed(3)
    N, C, h, w = 3, 12, 9, 14
    rh, rw = rep
    low = torch.randn(N, C, h, w, device="cuda").softmax(1).contiguous()
    full = low.repeat_interleave(rh, 2).repeat_interleave(rw, 3).contiguous()
    target = torch.randint(0, C, (N, h * rh, w * rw), device="cuda")
    target[0, :3, :5] = 255                                         # out-of-range labels hit no class in either path
    cw = torch.rand(C, device="cuda") + 0.5
    k = L.LOSS_DICE if kind == "dice" else L.LOSS_JACCARD
    nws = L.lib().ydl_seg_loss_ws_floats(N, C)
    ws_a, ws_b = torch.zeros(nws, device="cuda"), torch.zeros(nws, device="cuda")
    la, lb = torch.zeros(3, device="cuda"), torch.zeros(3, device="cuda")
    g = torch.tensor([0.7], device="cuda")
    st = _stream()
    L.call("ydl_seg_loss_fwd", _p(full), *full.stride(), _p(target), h * rh, w * rw, _p(cw), k, ls, 1e-6, N, C, h * rh, w * rw,
           _p(ws_a), _p(la), st)
    dfull = torch.empty_like(full)
    L.call("ydl_seg_loss_bwd", _p(full), *full.stride(), _p(target), h * rh, w * rw, _p(cw), k, ls, 1e-6, N, C, h * rh, w * rw,
           _p(ws_a), _p(g), _p(dfull), st)
    L.call("ydl_seg_loss_rep_fwd", _p(low), *low.stride(), _p(target), _p(cw), k, ls, 1e-6, N, C, h, w, rh, rw, _p(ws_b), _p(lb), st)
    dlow = torch.empty_like(low)
    L.call("ydl_seg_loss_rep_bwd", _p(low), *low.stride(), _p(target), _p(cw), k, ls, 1e-6, N, C, h, w, rh, rw, _p(ws_b), _p(g),
           _p(dlow), st)
    torch.cuda.synchronize()
    assert torch.allclose(la, lb, rtol=2e-6, atol=0), (la, lb)
    ref = dfull.view(N, C, h, rh, w, rw).double().sum((3, 5)).float()
    assert rel_err(dlow.cpu(), ref.cpu()) < 1e-5


def test_loss_fast_path_survives_only_untouched_predictions():
    """the model tags its replicated output; an in-place edit by the caller must switch the loss back to the dense kernels"""
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    torch.manual_seed(0)
    import os, yaml
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(ydl.__file__), "cfg", "yolov5_seg.yaml")))
    for sec in ("backbone", "head"):
        for l in cfg[sec]:
            l[2] = "C3" if l[2] == "C3_DCN" else l[2]
    m = ydl.YOLOv5Seg(cfg)
    m.img_size = [64, 64]
    m = m.cuda().train()
    x = torch.randn(2, 3, 64, 64, device="cuda")
    t = torch.randint(0, 12, (2, 64, 64), device="cuda")
    crit = ydl.SegmentationLoss(12, 0.0, None, "dice", sync=False)
    res = []
    for mode in ("fast", "dense", "edited"):
        for p in m.parameters():
            p.grad = None
        crit.use_replicated = mode != "dense"
        pred = m(x)
        assert getattr(pred, "_ydl_lazy", None) is not None
        if mode == "edited":
            pred.mul_(1.0)                       # bumps the version counter: the tag is stale
        total, _ = crit(pred, t)
        total.backward()
        res.append((float(total), torch.cat([p.grad.flatten() for p in m.parameters() if p.grad is not None]).cpu()))
    for tot, gr in res[1:]:
        assert abs(tot - res[0][0]) <= 2e-6 * abs(res[0][0])
        assert rel_err(gr, res[0][1]) < 2e-4


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_batched_weight_prep_matches_single(mode):
    """the tiled (LDS-transposed) multi-layer weight re-layout == the element-wise single-layer kernel, padding included"""
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.tape import _p, _stream
    dt, tdt = (L.YDL_F32, torch.float32) if mode == "f32" else (L.YDL_BF16, torch.bfloat16)
    r8 = lambda v: (v + 7) // 8 * 8
    shapes = [(64, 36, 3), (12, 1, 64), (40, 9, 24), (128, 1, 640), (72, 9, 100)]       # (Cout, k*k, Cin)
    torch.manual_seed(0)
    rows, refs, outs = [], [], []
    for (co, kk, ci) in shapes:
        master = torch.randn(co, kk, ci, device="cuda")
        w1 = torch.full((co, kk, r8(ci)), 7.0, device="cuda", dtype=tdt)
        t1 = torch.full((ci, kk, r8(co)), 7.0, device="cuda", dtype=tdt)
        w2, t2 = w1.clone(), t1.clone()
        L.call("ydl_weight_prep", dt, _p(master), _p(w1), _p(t1), co, kk, ci, _stream())
        rows.append([master.data_ptr(), w2.data_ptr(), t2.data_ptr(), co, kk, ci, 0, 0])
        refs.append((w1, t1, master))
        outs.append((w2, t2))
    desc = torch.tensor(rows, dtype=torch.int64).cuda()
    L.call("ydl_weight_prep_batched", dt, _p(desc), len(rows), _stream())
    torch.cuda.synchronize()
    for (w1, t1, _m), (w2, t2) in zip(refs, outs):
        assert torch.equal(w1, w2) and torch.equal(t1, t2)


def test_sgd_ema_flat_optimizer():
    """FlatSGDEMA == smart_optimizer(SGD nesterov) + ModelEMA on the reference's own 3-step trajectory."""
    import torch.nn as nn
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype("f32")
    g = Golden("optim_sgd_ema")
    lr, mom, wd = [float(v) for v in g.flat["hyp"]]
    net = nn.Sequential(ydl.Conv(4, 8, 3, 1), ydl.Conv(8, 4, 1, 1))
    net.load_state_dict(g.group("sd"))
    net = net.cuda().train()
    opt = ydl.FlatSGDEMA(net, lr=lr, momentum=mom, weight_decay=wd)
    x = g.t("x0").cuda()
    for st in range(int(g.flat["steps"])):
        opt.zero_grad()
        net[1](net[0](x)).square().mean().backward()
        if st == 0:
            named = dict(net.named_parameters())
            for k, v in g.group("g0").items():
                assert rel_err(named[k].grad.cpu(), v) < 1e-3, k
        opt.step()
    sd = net.state_dict()
    for k, v in g.group("sd_after").items():
        if v.dtype.is_floating_point:
            assert rel_err(sd[k].cpu(), v) < 2e-4, k
        else:
            assert torch.equal(sd[k].cpu(), v), k
    ema = opt.ema_state_dict()
    for k, v in g.group("ema_after").items():
        if v.dtype.is_floating_point:
            assert rel_err(ema[k].cpu(), v) < 2e-4, k
    ydl.set_compute_dtype("bf16")


def test_miou_confusion():
    from yolo_dual_amd.evaluate import ConfusionMatrix
    g = Golden("miou")
    pred_cls = g.t("pred")
    prob = torch.zeros(2, 12, 24, 24)
    prob.scatter_(1, pred_cls.unsqueeze(1), 1.0)
    cm = ConfusionMatrix(12, ignore_index=11)
    cm.process_batch(prob.cuda(), g.t("target").cuda())
    assert torch.equal(cm.matrix.cpu(), g.t("matrix"))
    miou, ious = cm.compute_iou()
    assert abs(miou - float(g.flat["miou"])) < 1e-9
    assert np.allclose(ious, g.flat["ious"], atol=1e-9)


def test_two_losses_on_one_replicated_prediction_add_their_gradients():
    """a second SegmentationLoss on the same model output must not overwrite the first one's side-channel gradient: the sum of
    two losses gives the gradients of the two separate runs added up; a second backward through a consumed region raises"""
    import yaml, os
    import yolo_dual_amd as ydl
    from oracle.fill import fill_state_dict
    ydl.set_compute_dtype("f32")
    try:
        cfg = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "..", "yolo_dual_amd", "cfg", "yolov5_seg.yaml")))
        for sec in ("backbone", "head"):
            for l in cfg[sec]:
                l[2] = "C3" if l[2] == "C3_DCN" else l[2]
        cw = torch.tensor([1, 2, 25, 2, 10, 3, 25, 10, 5, 15, 25, 1], dtype=torch.float32)
        gen = torch.Generator("cuda").manual_seed(0)
        x = torch.rand(2, 3, 64, 64, device="cuda", generator=gen)
        t1 = torch.randint(0, 12, (2, 64, 64), device="cuda", generator=gen)
        t2 = torch.randint(0, 12, (2, 64, 64), device="cuda", generator=gen)

        def run(which):
            m = ydl.YOLOv5Seg(cfg)
            m.img_size = [64, 64]
            sd = m.state_dict()
            fill_state_dict(sd, 9, bn_stats=False)
            m.load_state_dict(sd)
            m = m.cuda().train()
            out = m(x)
            la, _ = ydl.SegmentationLoss(12, 0.0, cw, "dice")(out, t1)
            lb, _ = ydl.SegmentationLoss(12, 0.0, cw, "jaccard")(out, t2)
            tot = {"a": la, "b": lb, "ab": la + lb}[which]
            tot.backward()
            if which == "ab":
                # a second backward THROUGH THE REGION (a fresh graph on top of its output, so that no other node's freed buffers
                # stop autograd first): the region's own guard (modules._Region.backward) is what must raise
                with pytest.raises(RuntimeError, match="second backward through a taped region"):
                    out.sum().backward()
            return {k: p.grad.detach().clone() for k, p in m.named_parameters() if getattr(p, "_ydl_touched", False)}
        ga, gb, gab = run("a"), run("b"), run("ab")
        assert sorted(ga) == sorted(gab)
        for k in gab:
            want = ga[k] + gb[k]
            assert l2_err(gab[k].cpu(), want.cpu()) < 2e-4, (k, l2_err(gab[k].cpu(), want.cpu()))
    finally:
        ydl.set_compute_dtype("bf16")
