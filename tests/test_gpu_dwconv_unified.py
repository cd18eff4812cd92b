"""GPU: a depth-wise ``Conv`` at stride 1 through the one depth-wise path of the tape (Tape.dw_bn_act: ydl_dwconv2_fwd with the
BatchNorm partial rows from the convolution launch), which the ``dw_conv`` branch of DCNv3 takes too, against oracle.ref_cpu in
float64, in f32 and in bf16 mode.

* ``Conv(16, 16, 3, g=16)`` at N = 2, H = 5, W = 7: the 4-column run of the forward kernel crosses row ends, and the 70 pixels are
  one full 64-pixel statistics block plus a 6-pixel tail.  Output, running statistics, input gradient, weight / gamma / beta
  gradients.
* a 12-channel layer writing channels [4, 16) of a 24-channel buffer: neither end is a multiple of 8 channels, so the result is
  staged and copied into place; the neighbouring channels stay as they were.
* the 16-channel layer with a residual joined after the activation (reachable only at stride 2 before): d/dres as well.

Tolerances are those of tests/test_gpu_ghost_blocks.py for its depth-wise layers: 1e-4 of each tensor's max in f32 mode, BF16_TOL in
bf16 mode."""
import functools

import pytest
import torch

from tests.block_harness import kind as _kind, rel_max_err as _err
from tests.test_gpu_ghost_blocks import BF16_TOL

pytestmark = pytest.mark.gpu

N, H, W = 2, 5, 7


@functools.lru_cache(maxsize=None)
def _case(C):
    """inputs, parameters and the float64 reference of one train-mode step of Conv(C, C, 3, g=C); computed once per width"""
    from oracle import ref_cpu as R
    g = torch.Generator().manual_seed(100 + C)
    t = {"x": torch.randn(N, C, H, W, generator=g), "gout": torch.randn(N, C, H, W, generator=g),
         "res": torch.randn(N, C, H, W, generator=g), "w": torch.randn(C, 1, 3, 3, generator=g) * 0.4,
         "gamma": torch.rand(C, generator=g) + 0.5, "beta": torch.rand(C, generator=g) * 0.6 - 0.3}
    leaf = {k: t[k].double().requires_grad_(True) for k in ("x", "w", "gamma", "beta")}
    sd = {"m.conv.weight": leaf["w"], "m.bn.weight": leaf["gamma"], "m.bn.bias": leaf["beta"],
          "m.bn.running_mean": torch.zeros(C, dtype=torch.float64), "m.bn.running_var": torch.ones(C, dtype=torch.float64)}
    out = R.dwconv_bn_act(sd, "m", leaf["x"], train=True)
    out.backward(t["gout"].double())
    ref = {"out": out.detach(), "grad_x": leaf["x"].grad, "g.conv.weight": leaf["w"].grad, "g.bn.weight": leaf["gamma"].grad,
           "g.bn.bias": leaf["beta"].grad, "rm.bn.running_mean": sd["m.bn.running_mean"], "rv.bn.running_var": sd["m.bn.running_var"]}
    return t, ref


def _layer(C):
    import yolo_dual_amd as ydl
    t, _ref = _case(C)
    m = ydl.Conv(C, C, 3, g=C)
    assert m.depthwise and m.s == 1
    with torch.no_grad():
        m.conv.weight.copy_(t["w"])
        m.bn.weight.copy_(t["gamma"])
        m.bn.bias.copy_(t["beta"])
    return m


def _check(mode, errs):
    print(f"[dw unified {mode}]", {k: f"{v:.1e}" for k, v in errs.items()})
    if mode == "f32":
        bad = {k: v for k, v in errs.items() if not v < 1e-4}
    else:
        bad = {k: v for k, v in errs.items() if not v < BF16_TOL[_kind(k)]}
    assert not bad, bad


def _param_errs(m, ref):
    errs = {}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        errs["g." + k] = _err(p.grad, ref["g." + k])
    sd = m.state_dict()
    errs["rm.bn.running_mean"] = _err(sd["bn.running_mean"], ref["rm.bn.running_mean"])
    errs["rv.bn.running_var"] = _err(sd["bn.running_var"], ref["rv.bn.running_var"])
    return errs


def _run(mode, fn):
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype(mode)
    try:
        fn()
    finally:
        ydl.set_compute_dtype("bf16")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_stride_one_layer_against_float64(mode):
    def body():
        t, ref = _case(16)
        m = _layer(16).cuda().train()
        x = t["x"].cuda().requires_grad_(True)
        out = m(x)
        out.backward(t["gout"].cuda())
        torch.cuda.synchronize()
        errs = {"out": _err(out, ref["out"]), "grad_x": _err(x.grad, ref["grad_x"])}
        errs.update(_param_errs(m, ref))
        _check(mode, errs)
    _run(mode, body)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_unaligned_destination_is_staged_and_neighbours_stay(mode):
    from yolo_dual_amd.modules import YdlModule

    class IntoSlice(YdlModule):
        def __init__(self):
            super().__init__()
            self.dw = _layer(12)

        def _fwd(self, tape, x):
            cat = tape.new(x.N, 24, x.H, x.W, zero=True)
            dst = cat.slice(4, 16)
            assert not dst.aligned()
            self.dw._fwd(tape, x, out=dst)
            return cat

    def body():
        t, ref = _case(12)
        m = IntoSlice().cuda().train()
        x = t["x"].cuda().requires_grad_(True)
        gout = torch.randn(N, 24, H, W, generator=torch.Generator().manual_seed(7))
        gout[:, 4:16] = t["gout"]
        out = m(x)
        out.backward(gout.cuda())
        torch.cuda.synchronize()
        assert out.shape == (N, 24, H, W)
        assert not bool(out[:, :4].any()) and not bool(out[:, 16:].any()), "channels beside the destination slice were written"
        errs = {"out": _err(out[:, 4:16], ref["out"]), "grad_x": _err(x.grad, ref["grad_x"])}
        errs.update(_param_errs(m.dw, ref))
        _check(mode, errs)
    _run(mode, body)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_residual_after_the_activation(mode):
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.modules import YdlModule

    class WithResidual(YdlModule):
        takes_list = True

        def __init__(self):
            super().__init__()
            self.dw = _layer(16)

        def _fwd(self, tape, xs):
            return self.dw._fwd(tape, xs[0], res=xs[1], res_mode=L.RES_AFTER_ACT)

    def body():
        t, ref = _case(16)
        m = WithResidual().cuda().train()
        x = t["x"].cuda().requires_grad_(True)
        r = t["res"].cuda().requires_grad_(True)
        out = m([x, r])
        out.backward(t["gout"].cuda())
        torch.cuda.synchronize()
        # out = silu(bn(dw(x))) + r: d/dr is the incoming gradient, everything else is the plain layer's
        errs = {"out": _err(out, ref["out"] + t["res"].double()), "grad_x": _err(x.grad, ref["grad_x"]),
                "grad_res": _err(r.grad, t["gout"].double())}
        errs.update(_param_errs(m.dw, ref))
        _check(mode, errs)
    _run(mode, body)
