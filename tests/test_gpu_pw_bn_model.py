"""config.fuse_bn_pw_backward() at model level: bench.py's cfg2 model (YOLOv5Seg) at 8 x 512 x 512, the smallest input whose 1/4-scale
layers (8 x 128 x 128 = 131 072 pixels) the one-pass 1x1 backward still takes.  One forward + backward from the same weights and inputs
with the switch off, off again and on.  Every parameter gradient of the fused step must lie within twice the distance (L2 over the
parameter) of the two unfused steps, which differ because BatchNorm sums and weight gradients are added atomically in arrival order;
the fused entry points appear in the recorded launches only with the switch on, and every other launch is the same.

The loss: the forward does not depend on the switch, but in throughput mode it is not reproducible from run to run either (the
BatchNorm statistics are f32 atomic sums: two unfused steps gave 2.920916796 and 2.920918226 on one MI355X), so "equal" cannot be
asked of any two steps.  The bound is what reordering an f32 sum of n terms costs, sqrt(n) x 2^-24 relative with n the number of
output pixels (8.6e-5 here, 60 times the difference seen between unfused steps; a forward that changed would move the loss by
percent)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class _Names:
    def __init__(self):
        self.names = []

    def add(self, name, args):
        self.names.append(name)

    def edge(self, src, dst):
        pass


def test_fused_bn_backward_step_matches_the_unfused_step():
    import bench
    import yolo_dual_amd as ydl
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd import config
    wl = bench.WORKLOADS["cfg2"]
    dev = torch.device("cuda", torch.cuda.current_device())
    ydl.set_compute_dtype("bf16")
    bs, size = 8, 512
    torch.manual_seed(0)
    model = getattr(ydl, wl["model"])(bench.load_cfg(wl["yaml"], wl["swap"])).to(dev).train()
    model.img_size = [size, size]
    crit = ydl.SegmentationLoss(12, 0.0, torch.tensor(bench.CW, dtype=torch.float32), wl["loss"], sync=False)
    opt = ydl.FlatSGDEMA(model, lr=0.01, momentum=0.937, weight_decay=5e-4 * bs / 64.0)      # (flat gradient storage, as the benchmark has it)
    g = torch.Generator(device=dev).manual_seed(1234)
    imgs = torch.rand(bs, 3, size, size, device=dev, generator=g)
    tgts = torch.randint(0, 12, (bs, size, size), device=dev, generator=g)
    params = [(n, p) for n, p in model.named_parameters() if p.requires_grad]

    def step(on):
        config.set_fuse_bn_pw_backward(on)
        rec = _Names()
        opt.zero_grad()
        L.set_recorder(rec)
        try:
            out = model(imgs)
            loss, _items = crit(out, tgts)
            loss.backward()
        finally:
            L.set_recorder(None)
        torch.cuda.synchronize()
        return float(loss.detach()), [p.grad.detach().double().clone() for _n, p in params], rec.names

    was = config.fuse_bn_pw_backward()
    try:
        step(False)                                            # warm-up: sibling pairs fuse from the second step on
        l0, g0, n0 = step(False)
        l1, g1, n1 = step(False)
        l2, g2, n2 = step(True)
    finally:
        config.set_fuse_bn_pw_backward(was)
    fused = ("ydl_conv_bwd_pw_bn", "ydl_bn_act_bwd_reduce_sums")
    assert not any(n in fused for n in n0 + n1), "fused entry points launched with the switch off"
    count = {n: n2.count(n) for n in fused}
    print("launches with the switch on:", count, " ydl_conv_bwd_pw:", n2.count("ydl_conv_bwd_pw"), "(off:", n0.count("ydl_conv_bwd_pw"), ")")
    assert count["ydl_conv_bwd_pw_bn"] >= 1 and count["ydl_bn_act_bwd_reduce_sums"] >= count["ydl_conv_bwd_pw_bn"]
    assert n2.count("ydl_conv_bwd_pw_bn") + n2.count("ydl_conv_bwd_pw") == n0.count("ydl_conv_bwd_pw")
    moved = fused + ("ydl_conv_bwd_pw", "ydl_bn_act_bwd_sums")
    assert [n for n in n2 if n not in moved] == [n for n in n0 if n not in moved], "a launch outside the fused layers changed"
    assert n0.count("ydl_bn_act_bwd_sums") - n2.count("ydl_bn_act_bwd_sums") == count["ydl_bn_act_bwd_reduce_sums"]
    tol = (bs * size * size) ** 0.5 * 2.0 ** -24 * abs(l0)
    print(f"loss: off {l0!r} off {l1!r} on {l2!r}  bound {tol:.3e}")
    assert abs(l2 - l0) <= tol, (l0, l1, l2)
    worst = (0.0, "")
    for (n, _p), a, b, c in zip(params, g0, g1, g2):
        spread = float((a - b).norm())
        d = float((c - a).norm())
        ratio = d / spread if spread > 0 else (0.0 if d == 0 else float("inf"))
        if ratio > worst[0]:
            worst = (ratio, n)
        assert d <= 2.0 * spread, f"{n}: |fused - unfused| = {d:.3e}, spread of two unfused steps = {spread:.3e}"
    print(f"largest |fused - unfused| / spread of two unfused steps: {worst[0]:.3f} ({worst[1]})")
