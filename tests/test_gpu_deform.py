"""GPU: deformable convolution (torchvision.ops.deform_conv2d) on the HIP kernels against the f64 restatement of
tests/deform_ref.py (itself pinned by F.conv2d answers in tests/test_deform_ref_cpu.py), and the script C3_DCN / C2f_DCN blocks
against a CPU f64 composition."""
import pytest
import torch
import torch.nn.functional as F

from tests.deform_ref import deform_conv2d_ref

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / max(float(b.abs().max()), 1e-30))


# (N, C, H, W, Cout, k, s, p, d, G, mask, sigma, expected backward kernel)
CASES = [
    (2, 128, 20, 20, 128, 3, 1, 1, 1, 1, False, 0.5, "window"),
    (2, 128, 20, 20, 128, 3, 1, 1, 1, 1, True, 0.0, "window"),
    (2, 64, 24, 24, 64, 3, 1, 1, 1, 1, True, 2.5, "window"),
    (2, 24, 13, 11, 16, 3, 1, 1, 1, 1, False, 6.0, "window"),
    (1, 72, 10, 14, 40, 3, 1, 1, 1, 2, True, 0.5, "window"),
    (2, 32, 17, 15, 24, 3, 2, 1, 1, 1, True, 0.5, "atomic"),
    (2, 32, 15, 15, 24, 3, 1, 2, 2, 1, False, 2.5, "atomic"),
    (2, 16, 9, 9, 8, 1, 1, 0, 1, 2, True, 6.0, "atomic"),
    (1, 16, 12, 12, 8, 5, 1, 2, 1, 1, True, 0.5, "atomic"),
]


def _inputs(N, C, H, W, Cout, k, s, p, d, G, mask, sigma, seed=0):
    g = torch.Generator().manual_seed(seed)
    Ho = (H + 2 * p - (d * (k - 1) + 1)) // s + 1
    Wo = (W + 2 * p - (d * (k - 1) + 1)) // s + 1
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    off = sigma * torch.randn(N, 2 * G * k * k, Ho, Wo, generator=g, dtype=torch.float64)
    # fractional parts kept 0.05 px away from integers: the offset gradient jumps where a position crosses one, and an f32 position
    # within rounding of an integer (~1e-5 px at 128 px) may land on the other side than the f64 one (about one tap in 1e5)
    if sigma > 0:
        off = torch.floor(off) + 0.05 + 0.9 * (off - torch.floor(off))
    w = torch.randn(Cout, C, k, k, generator=g, dtype=torch.float64) / (C * k * k) ** 0.5
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    m = torch.sigmoid(torch.randn(N, G * k * k, Ho, Wo, generator=g, dtype=torch.float64)) if mask else None
    gout = torch.randn(N, Cout, Ho, Wo, generator=g, dtype=torch.float64)
    return x, off, w, b, m, gout


def _run(case, dtype, win=True):
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.deform import deform_conv2d
    N, C, H, W, Cout, k, s, p, d, G, mask, sigma, _ = case
    x, off, w, b, m, gout = _inputs(*case[:12])
    tens = [x, off, w, b] + ([m] if m is not None else [])
    dev = [t.to(dtype).cuda().requires_grad_() for t in tens]
    L.debug_set(20, 1 if win else 0)
    try:
        out = deform_conv2d(dev[0], dev[1], dev[2], dev[3], s, p, d, dev[4] if m is not None else None)
        out.backward(gout.to(dtype).cuda())
        torch.cuda.synchronize()
        kname = L.last_kernel(4)
    finally:
        L.debug_set(20, 1)
    ref_in = [t.to(dtype).double().requires_grad_() for t in tens]      # bf16: the reference sees the bf16-rounded inputs
    ref = deform_conv2d_ref(ref_in[0], ref_in[1], ref_in[2], ref_in[3], s, p, d, ref_in[4] if m is not None else None)
    ref.backward(gout.to(dtype).double())
    errs = {"out": _rel(out.detach(), ref.detach())}
    for nm, a, r in zip(("input", "offset", "weight", "bias", "mask"), dev, ref_in):
        errs[nm] = _rel(a.grad, r.grad)
    return errs, kname


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"C{c[1]}_k{c[5]}s{c[6]}p{c[7]}d{c[8]}G{c[9]}{'m' if c[10] else ''}_sig{c[11]}")
def test_deform_conv2d_f32_matches_f64_restatement(case):
    errs, kname = _run(case, torch.float32)
    assert case[12] in kname, kname
    assert errs["out"] < 1e-5, errs
    assert max(v for k_, v in errs.items() if k_ != "out") < 1e-4, errs


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=["sig0.5", "sig6"])
def test_deform_conv2d_atomic_path_forced(case):
    errs, kname = _run(case, torch.float32, win=False)
    assert "atomic" in kname, kname
    assert errs["out"] < 1e-5 and max(errs.values()) < 1e-4, errs


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[5]], ids=["win", "win_mask", "strided"])
def test_deform_conv2d_bf16(case):
    errs, _ = _run(case, torch.bfloat16)
    # bf16 storage of col / dcol and bf16 MFMA operands against f64 on the same bf16-rounded inputs
    assert errs["out"] < 2e-2, errs
    assert max(errs.values()) < 5e-2, errs


# ---------------------------------------------------------------------------------------------- blocks
def _conv_ref(x, sd, pre, act=True, bn=None):
    """Conv = conv2d (no bias, 'same' padding) -> train-mode BatchNorm2d -> SiLU, f64; returns (y, new running stats)"""
    w = sd[f"{pre}.conv.weight"]
    y = F.conv2d(x, w, None, 1, w.shape[-1] // 2)
    return _bn_ref(y, sd, f"{pre}.bn", act)


def _bn_ref(y, sd, pre, act=True):
    rm, rv = sd[f"{pre}.running_mean"].clone(), sd[f"{pre}.running_var"].clone()
    z = F.batch_norm(y, rm, rv, sd[f"{pre}.weight"], sd[f"{pre}.bias"], True, 0.1, 1e-5)
    _bn_ref.stats[pre] = (rm, rv)
    return F.silu(z) if act else z


_bn_ref.stats = {}


def _c3_dcn_ref(x, sd, add):
    a = _conv_ref(x, sd, "cv1")
    a = _conv_ref(a, sd, "m.0.0", act=False)
    off = _conv_ref(a, sd, "m.0.1")
    a = _bn_ref(deform_conv2d_ref(a, off, sd["m.0.2.weight"], None, 1, 1), sd, "m.0.3.0")
    y = _conv_ref(torch.cat([a, _conv_ref(x, sd, "cv2")], 1), sd, "cv3")
    return y + x if add else y


def _c2f_dcn_ref(x, sd, add):
    y0 = _conv_ref(x, sd, "cv1")
    c = y0.shape[1] // 2
    a = _conv_ref(y0[:, c:], sd, "m.0.0", act=False)
    off = _conv_ref(a, sd, "m.0.1")
    a = _bn_ref(deform_conv2d_ref(a, off, sd["m.0.2.weight"], None, 1, 1), sd, "m.0.3.0")
    y = _conv_ref(torch.cat([y0, a], 1), sd, "cv2")
    return y + x if add else y


@pytest.mark.parametrize("kind", ["C3_DCN", "C2f_DCN"])
def test_block_train_step_matches_f64_composition(kind):
    import yolo_dual_amd as ydl
    torch.manual_seed(0)
    ydl.set_compute_dtype("f32")
    try:
        blk = getattr(ydl, kind)(32, 32)
        for n, p_ in blk.named_parameters():                    # non-trivial BN affine and offset-branch weights
            if n.endswith("bn.weight") or n.endswith(".3.0.weight"):
                p_.data.uniform_(0.5, 1.5)
            elif n.endswith("bn.bias") or n.endswith(".3.0.bias"):
                p_.data.uniform_(-0.2, 0.2)
        sd0 = {k: v.detach().double().clone() for k, v in blk.state_dict().items()}
        x = torch.randn(2, 32, 12, 10, dtype=torch.float64)
        gout = torch.randn(2, 32, 12, 10, dtype=torch.float64)
        blk = blk.cuda().train()
        xd = x.float().cuda().requires_grad_()
        out = blk(xd)
        out.backward(gout.float().cuda())
        torch.cuda.synchronize()
    finally:
        ydl.set_compute_dtype("bf16")
    params = {k: v.requires_grad_() if v.is_floating_point() and "running" not in k else v for k, v in sd0.items()}
    xr = x.clone().requires_grad_()
    _bn_ref.stats = {}
    ref = (_c3_dcn_ref if kind == "C3_DCN" else _c2f_dcn_ref)(xr, params, True)
    ref.backward(gout)
    assert _rel(out.detach(), ref.detach()) < 1e-4, _rel(out.detach(), ref.detach())
    assert _rel(xd.grad, xr.grad) < 1e-3, _rel(xd.grad, xr.grad)
    sd1 = blk.state_dict()
    for pre, (rm, rv) in _bn_ref.stats.items():
        assert _rel(sd1[f"{pre}.running_mean"], rm) < 1e-4, pre
        assert _rel(sd1[f"{pre}.running_var"], rv) < 1e-4, pre
    for n, p_ in blk.named_parameters():
        assert p_.grad is not None, n
        e = _rel(p_.grad, params[n].grad)
        assert e < 1e-3, (n, e)


def test_yolov5seg_deformable_trains_bf16():
    import yaml
    import yolo_dual_amd as ydl
    torch.manual_seed(0)
    cfg = yaml.safe_load(open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "yolo_dual_amd", "cfg",
                                                         "yolov5_seg.yaml")))
    ydl.set_compute_dtype("bf16")
    S = 128
    model = ydl.YOLOv5Seg(cfg, deformable=True)
    model.img_size = [S, S]
    cpu_sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.cuda().train()
    crit = ydl.SegmentationLoss(12, 0.0, torch.ones(12), "dice")
    opt = ydl.FlatSGDEMA(model, lr=0.01, momentum=0.9, weight_decay=5e-4)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 3, S, S, generator=g)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    t = (((yy // 32) + (xx // 32)) % 12).long().expand(2, S, S).contiguous()       # blobby synthetic labels
    x[:, 0] += t.float() / 12
    losses = []
    for _ in range(30):
        opt.zero_grad()
        total, items = crit(model(x.cuda()), t.cuda())
        total.backward()
        opt.step()
        losses.append(items[0])
    torch.cuda.synchronize()
    assert all(l == l and abs(l) < 1e6 for l in losses), losses
    assert sum(losses[-5:]) / 5 < sum(losses[:5]) / 5, losses
    # state_dict round trip with a CPU-built model
    m2 = ydl.YOLOv5Seg(cfg, deformable=True)
    m2.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    assert list(m2.state_dict().keys()) == list(cpu_sd.keys())


# ------------------------------------------------------------------ models/common.py family: DCNv2 / Bottleneck_DCN / C3_DCN
def _dcnv2_ref(x, sd, pre, train=True):
    """models/common.py:1662-1679: offset = om[:, :18], mask = sigmoid(om[:, 18:27]), deform_conv2d with bias, BN, SiLU"""
    om = F.conv2d(x, sd[f"{pre}.conv_offset_mask.weight"], sd[f"{pre}.conv_offset_mask.bias"], 1, 1)
    y = deform_conv2d_ref(x, om[:, :18], sd[f"{pre}.weight"], sd[f"{pre}.bias"], 1, 1, 1, torch.sigmoid(om[:, 18:27]))
    if train:
        return _bn_ref(y, sd, f"{pre}.bn")
    z = F.batch_norm(y, sd[f"{pre}.bn.running_mean"], sd[f"{pre}.bn.running_var"], sd[f"{pre}.bn.weight"], sd[f"{pre}.bn.bias"],
                     False, 0.1, 1e-5)
    return F.silu(z)


def _conv_eval(x, sd, pre):
    w = sd[f"{pre}.conv.weight"]
    y = F.conv2d(x, w, None, 1, w.shape[-1] // 2)
    return F.silu(F.batch_norm(y, sd[f"{pre}.bn.running_mean"], sd[f"{pre}.bn.running_var"], sd[f"{pre}.bn.weight"],
                               sd[f"{pre}.bn.bias"], False, 0.1, 1e-5))


def _c3_dcn_common_ref(x, sd, train=True):
    cv = _conv_ref if train else (lambda t, s, p: _conv_eval(t, s, p))
    a = cv(x, sd, "cv1")
    a = a + _dcnv2_ref(cv(a, sd, "m.0.cv1"), sd, "m.0.cv2", train)     # Bottleneck_DCN(c_, c_, shortcut=True): residual
    return cv(torch.cat([a, cv(x, sd, "cv2")], 1), sd, "cv3")


def test_common_c3_dcn_block_train_and_eval_match_f64():
    """DCNv2 inside models/common.py's C3_DCN: the logit mask (sigmoid applied in the kernels), the bias as a GEMM column (output,
    BN running mean, bias gradient), the biased conv_offset_mask; then eval mode on the running statistics"""
    import yolo_dual_amd as ydl
    torch.manual_seed(0)
    ydl.set_compute_dtype("f32")
    try:
        blk = ydl.C3_DCNCommon(32, 32, 1)
        dc = blk.m[0].cv2
        with torch.no_grad():                                 # generic offsets (~1 px) and masks instead of the zero initialisation
            dc.conv_offset_mask.weight.normal_(0, 0.08)
            dc.conv_offset_mask.bias.normal_(0, 0.5)
            dc.bias.normal_(0, 0.5)
            for n, p_ in blk.named_parameters():
                if n.endswith("bn.weight"):
                    p_.uniform_(0.5, 1.5)
                elif n.endswith("bn.bias"):
                    p_.uniform_(-0.2, 0.2)
        sd0 = {k: v.detach().double().clone() for k, v in blk.state_dict().items()}
        x = torch.randn(2, 32, 12, 10, dtype=torch.float64)
        gout = torch.randn(2, 32, 12, 10, dtype=torch.float64)
        blk = blk.cuda().train()
        xd = x.float().cuda().requires_grad_()
        out = blk(xd)
        out.backward(gout.float().cuda())
        torch.cuda.synchronize()
        blk.eval()
        with torch.no_grad():
            out_eval = blk(x.float().cuda())
        torch.cuda.synchronize()
    finally:
        ydl.set_compute_dtype("bf16")
    params = {k: v.requires_grad_() if v.is_floating_point() and "running" not in k else v for k, v in sd0.items()}
    xr = x.clone().requires_grad_()
    _bn_ref.stats = {}
    ref = _c3_dcn_common_ref(xr, params)
    ref.backward(gout)
    assert _rel(out.detach(), ref.detach()) < 1e-4, _rel(out.detach(), ref.detach())
    assert _rel(xd.grad, xr.grad) < 1e-3, _rel(xd.grad, xr.grad)
    sd1 = blk.state_dict()
    for pre, (rm, rv) in _bn_ref.stats.items():
        assert _rel(sd1[f"{pre}.running_mean"], rm) < 1e-4, (pre, _rel(sd1[f"{pre}.running_mean"], rm))
        assert _rel(sd1[f"{pre}.running_var"], rv) < 1e-4, pre
    wscale = float(params["m.0.cv2.weight"].grad.abs().max())
    for n, p_ in blk.named_parameters():
        assert p_.grad is not None, n
        if n == "m.0.cv2.bias":       # a bias in front of train-mode BN: its exact gradient is 0 (the reference's is rounding noise)
            assert float(p_.grad.abs().max()) < 1e-4 * wscale, float(p_.grad.abs().max())
            continue
        e = _rel(p_.grad, params[n].grad)
        assert e < 1e-3, (n, e)
    # eval mode: the running statistics (bias included in the running mean) against the f64 composition
    sde = {k: v.detach().double().cpu() for k, v in sd1.items()}
    ref_eval = _c3_dcn_common_ref(x, sde, train=False)
    assert _rel(out_eval, ref_eval) < 1e-4, _rel(out_eval, ref_eval)


@pytest.mark.parametrize("N,C,H", [(2, 128, 80), (1, 128, 128)], ids=["cfg2_128@80", "128@128"])
def test_deform_conv2d_layer_sizes(N, C, H):
    """the issue's layer shapes: many window tiles, offsets with taps off the image, f32 against f64"""
    case = (N, C, H, H, C, 3, 1, 1, 1, 1, False, 0.5, "window")
    errs, kname = _run(case, torch.float32)
    assert "window" in kname, kname
    assert errs["out"] < 1e-5 and max(errs.values()) < 1e-4, errs


def _bf16_f32_grad_gap(cfg, native, S=64):
    """relative L2 of the bf16 parameter gradients against the f32 ones, one step from the same weights and batch"""
    import yolo_dual_amd as ydl
    from oracle.fill import fill_state_dict
    sd = ydl.YOLOv5Seg(cfg, deformable=native).state_dict()
    fill_state_dict(sd, 5, bn_stats=False)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 3, S, S, generator=g)
    t = torch.randint(0, 12, (2, S, S), generator=g)
    grads = {}
    for mode in ("f32", "bf16"):
        ydl.set_compute_dtype(mode)
        m = ydl.YOLOv5Seg(cfg, deformable=native)
        m.load_state_dict(sd)
        m.img_size = [S, S]
        m = m.cuda().train()
        crit = ydl.SegmentationLoss(12, 0.0, torch.ones(12), "dice")
        total, _ = crit(m(x.cuda()), t.cuda())
        total.backward()
        torch.cuda.synchronize()
        # (parameters of the dead head layers keep grad None)
        grads[mode] = torch.cat([p.grad.detach().float().flatten().cpu() for p in m.parameters() if p.grad is not None])
    ydl.set_compute_dtype("bf16")
    return float((grads["bf16"] - grads["f32"]).norm() / grads["f32"].norm()), m, x


def test_yolov5seg_deformable_bf16_grads_near_f32_and_eval_fuse():
    """bf16 against f32 parameter gradients of the native model stay within 2.5x the gap of the same model with C3 substituted
    (measured 0.66 against 0.37 at 64^2: the offset branch's gradient jumps where a tap crosses a pixel, and bf16 offsets move taps
    by ~0.01 px); then eval mode (running statistics) and model.fuse() (DCN blocks stay unfused) run and agree"""
    import yaml
    import os
    import yolo_dual_amd as ydl
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "..", "yolo_dual_amd", "cfg", "yolov5_seg.yaml")))
    sub = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "..", "yolo_dual_amd", "cfg", "yolov5_seg.yaml")))
    for sec in ("backbone", "head"):
        for l in sub[sec]:
            l[2] = {"C3_DCN": "C3"}.get(l[2], l[2])
    gap_sub, _, _ = _bf16_f32_grad_gap(sub, False)
    gap, m, x = _bf16_f32_grad_gap(cfg, True)
    assert gap < 2.5 * gap_sub, f"bf16 vs f32 gradient relative L2: native {gap:.3e}, substituted {gap_sub:.3e}"
    ydl.set_compute_dtype("f32")
    try:
        m.eval()
        with torch.no_grad():
            a = m(x.cuda())
            m.fuse()
            b = m(x.cuda())
        torch.cuda.synchronize()
    finally:
        ydl.set_compute_dtype("bf16")
    assert torch.isfinite(a).all() and _rel(b, a.cpu().double()) < 1e-4, _rel(b, a.cpu().double())
