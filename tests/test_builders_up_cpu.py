"""CPU: the decoder up-samplers.  ``ConvTranspose2d`` has torch's constructor signature, state_dict layout and default initialisation and
serves stride 2 with (kernel_size, padding, output_padding) in {(2,0,0), (4,1,0), (3,1,1)}, groups 1, dilation 1, channels multiples of
8; ``DWConvTranspose2d(c1, c2, k, s, p1, p2)`` (models/common.py:73-76) serves the same forms depth-wise (c1 == c2); everything else is
refused by class and argument name, the constructor's own defaults k = 1, s = 1 included.  ``parse_model`` resolves both rows with the
width gain, ``Upsample`` builds in mode 'bicubic', and every fixture under tests/golden/up_*.npz (tools/make_up_golden.py) is reproduced
on the CPU in float64 by torch (the transposed convolutions) and by tests/up_ref.py (bicubic)."""
import glob
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "up_*.npz")))
NAMES = ["up_bicubic_7x10_ac", "up_bicubic_x2", "up_dwtconv_16_k4", "up_dwtconv_24_k2", "up_tconv_16_16_k4_nobias", "up_tconv_16_24_k2",
         "up_tconv_24_8_k3"]
FORMS = ((2, 0, 0), (4, 1, 0), (3, 1, 1))
# 3 x 32 x 32 -> stem 16 ch @ 16^2 -> 32 ch @ 8^2 -> C3 -> 32 ch @ 4^2 -> DWConvTranspose2d k4 (32 ch @ 8^2) -> Concat with the C3 (64 ch)
# -> nn.ConvTranspose2d k2 (16 ch @ 16^2) -> Concat with the stem (32 ch) -> bicubic x2 (32^2) -> 12 classes
YAML = {"nc": 12, "width_multiple": 0.5, "depth_multiple": 0.33,
        "backbone": [[-1, 1, "Conv", [32, 6, 2, 2]], [-1, 1, "Conv", [64, 3, 2]], [-1, 3, "C3", [64]], [-1, 1, "Conv", [64, 3, 2]]],
        "head": [[-1, 1, "DWConvTranspose2d", [64, 4, 2, 1, 0]], [[-1, 2], 1, "Concat", [1]], [-1, 1, "nn.ConvTranspose2d", [32, 2, 2]],
                 [[-1, 0], 1, "Concat", [1]], [-1, 1, "nn.Upsample", ["None", 2, "bicubic"]], [-1, 1, "Conv", [12, 1, 1]]]}


def build(z):
    """the module a fixture describes (weights not loaded); JSON turned tuples into lists"""
    import yolo_dual_amd as ydl
    args = [tuple(a) if isinstance(a, list) else a for a in json.loads(str(z["args"]))]
    return getattr(ydl, str(z["cls"]))(*args, **json.loads(str(z["kwargs"])))


def test_the_seven_fixtures_are_present_small_and_carry_the_floors():
    assert [os.path.basename(f)[:-4] for f in FILES] == NAMES
    assert all(os.path.getsize(f) < 100 * 1024 for f in FILES)           # each well under the gconv_* fixtures (175 / 355 KB)
    for f in FILES:
        z = np.load(f)
        assert z["x"].shape[0] == 2 and z["x"].shape[2:] == (5, 7)
        for kind in ("out", "grad"):
            v = float(z["floor." + kind])
            assert 2.0 ** -10 < v < 0.1, (f, kind, v)


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_is_reproduced_in_float64(path):
    """torch's own float64 operators for the transposed convolutions, the restatement of tests/up_ref.py for bicubic; the arrays are
    stored as float32, so 1e-6 of each tensor's max"""
    import torch
    import torch.nn.functional as F
    from tests import up_ref as B
    z = np.load(path)
    cls, args, kwargs = str(z["cls"]), json.loads(str(z["args"])), json.loads(str(z["kwargs"]))
    x, gout = z["x"].astype(np.float64), z["grad_out"].astype(np.float64)
    got = {}
    if cls == "Upsample":
        size, sf, mode, align = (args + [None])[:4]
        assert mode == "bicubic"
        xh, gh = x.transpose(0, 2, 3, 1), gout.transpose(0, 2, 3, 1)
        Ho, Wo = gh.shape[1:3]
        g = 0.0 if (align or sf is None) else 1.0 / sf
        th, tw = B.cub_taps(bool(align), 5, Ho, g, np.float64), B.cub_taps(bool(align), 7, Wo, g, np.float64)
        got["out"] = B.bicubic_fwd_ref(xh, th, tw)[0].transpose(0, 3, 1, 2)
        got["grad_x"] = B.bicubic_bwd_ref(gh, th, tw, 5, 7)[0].transpose(0, 3, 1, 2)
    else:
        c1, c2, k, s = args[:4]
        p, op = (args + [0, 0])[4:6]
        w = torch.from_numpy(z["p.weight"]).double().requires_grad_(True)
        b = torch.from_numpy(z["p.bias"]).double().requires_grad_(True) if "p.bias" in z.files else None
        assert (b is None) == (kwargs.get("bias") is False)
        xt = torch.from_numpy(x).requires_grad_(True)
        groups = c1 if cls == "DWConvTranspose2d" else 1
        assert tuple(w.shape) == (c1, c2 // groups, k, k)
        out = F.conv_transpose2d(xt, w, b, stride=s, padding=p, output_padding=op, groups=groups)
        out.backward(torch.from_numpy(gout))
        got = {"out": out.detach().numpy(), "grad_x": xt.grad.numpy(), "g.weight": w.grad.numpy()}
        if b is not None:
            got["g.bias"] = b.grad.numpy()
    assert set(got) == {k for k in z.files if k in ("out", "grad_x") or k.startswith("g.")}
    for k, v in got.items():
        want = z[k].astype(np.float64)
        assert v.shape == want.shape and np.abs(v - want).max() <= 1e-6 * np.abs(want).max(), k


def test_constructor_forms_and_state_dict_equal_torchs():
    import torch
    import torch.nn as nn
    import yolo_dual_amd as ydl
    for k, p, op in FORMS:
        for bias in (True, False):
            torch.manual_seed(5)
            m = ydl.ConvTranspose2d(16, 24, k, 2, p, op, bias=bias)
            torch.manual_seed(5)
            ref = nn.ConvTranspose2d(16, 24, k, 2, p, op, bias=bias)
            assert isinstance(m, nn.ConvTranspose2d) and (m.k, m.s, m.p, m.op) == (k, 2, p, op)
            assert [(n, tuple(v.shape)) for n, v in m.state_dict().items()] == [(n, tuple(v.shape)) for n, v in ref.state_dict().items()]
            assert m.weight.shape == (16, 24, k, k) and (m.bias is None) == (not bias)
            assert torch.equal(m.weight, ref.weight) and (not bias or torch.equal(m.bias, ref.bias))       # torch's default initialisation
            # channels_last storage [c1][k*k][c2]: the KRSC master of the mirrored convolution c2 -> c1
            assert m.weight.permute(0, 2, 3, 1).is_contiguous() and m._gemm_dims() == (16, k * k, 24)
            fresh = nn.ConvTranspose2d(16, 24, k, 2, p, op, bias=bias)
            m.load_state_dict(fresh.state_dict())
            assert torch.equal(m.weight, fresh.weight) and m.weight.permute(0, 2, 3, 1).is_contiguous()
            assert m._master_krsc().shape == (16, k, k, 24)
        d = ydl.DWConvTranspose2d(24, 24, k, 2, p, op)
        assert isinstance(d, nn.ConvTranspose2d) and d.groups == 24 and d.weight.shape == (24, 1, k, k) and d.bias.shape == (24,)
        assert list(d.state_dict()) == ["weight", "bias"] and d.master_dw().shape == (24, k, k, 1) and d.master_dw().is_contiguous()
    assert ydl.ConvTranspose2d(8, 8, (4, 4), (2, 2), (1, 1)).k == 4                      # a pair with equal entries means the int
    assert "ConvTranspose2d" in ydl.__all__ and "DWConvTranspose2d" in ydl.__all__


def test_what_lies_outside_the_served_set_is_refused_by_name():
    import yolo_dual_amd as ydl
    T = ydl.ConvTranspose2d
    for word, args, kw in (("stride", (16, 16, 4), {}), ("stride", (16, 16, 4, 1, 1), {}), ("stride", (16, 16, 4, 3, 1), {}),
                           ("stride", (16, 16, 4, (2, 1), 1), {}), ("kernel_size", (16, 16, 5, 2, 2, 1), {}), ("kernel_size", (16, 16, 1, 2), {}),
                           ("kernel_size", (16, 16, (4, 2), 2), {}), ("padding", (16, 16, 4, 2, 0), {}), ("padding", (16, 16, 2, 2, 1), {}),
                           ("output_padding", (16, 16, 3, 2, 1, 0), {}), ("output_padding", (16, 16, 4, 2, 1, 1), {}),
                           ("groups", (16, 16, 4, 2, 1), {"groups": 2}), ("groups", (16, 16, 4, 2, 1), {"groups": 16}),
                           ("dilation", (16, 16, 4, 2, 1), {"dilation": 2}), ("padding_mode", (16, 16, 4, 2, 1), {"padding_mode": "reflect"}),
                           ("in_channels", (12, 16, 4, 2, 1), {}), ("out_channels", (16, 12, 4, 2, 1), {})):
        with pytest.raises(NotImplementedError, match="ConvTranspose2d.*" + word):
            T(*args, **kw)
    D = ydl.DWConvTranspose2d
    for word, args in (("s=", (16, 16)), ("s=", (16, 16, 4)), ("s=", (16, 16, 4, 1, 1)), ("k=", (16, 16, 1, 2)), ("k=", (16, 16, 5, 2, 2, 1)),
                       ("p1=", (16, 16, 4, 2, 0)), ("p2=", (16, 16, 3, 2, 1, 0)), ("p2=", (16, 16, 2, 2, 0, 1)), ("groups", (16, 32, 4, 2, 1)),
                       ("groups", (16, 24, 4, 2, 1)), ("c1=", (12, 12, 4, 2, 1))):
        with pytest.raises(NotImplementedError, match="DWConvTranspose2d.*" + word):
            D(*args)
    with pytest.raises(NotImplementedError, match="output_size"):
        T(16, 16, 2, 2)(None, output_size=(4, 4))


def test_upsample_builds_bicubic_and_still_refuses_area():
    import yolo_dual_amd as ydl
    from yolo_dual_amd.models import _upsample_from_yaml
    for ac in (None, False, True):
        u = ydl.Upsample(scale_factor=2, mode="bicubic", align_corners=ac)
        assert u.mode == "bicubic" and u.align_corners is ac
    assert ydl.Upsample(size=(7, 10), mode="bicubic").size == (7, 10)
    with pytest.raises(NotImplementedError, match="area"):
        ydl.Upsample(scale_factor=2, mode="area")
    u = _upsample_from_yaml(["None", 2, "bicubic"], "v5")
    assert (u.mode, u.scale_factor, u.size, u.align_corners) == ("bicubic", 2.0, None, False)


def test_parse_model_builds_the_two_transposed_rows():
    import yolo_dual_amd as ydl
    d = {"nc": 12, "width_multiple": 0.5, "backbone": [[-1, 1, "Conv", [32, 3, 2]], [-1, 1, "nn.ConvTranspose2d", [48, 4, 2, 1]],
                                                       [-1, 1, "DWConvTranspose2d", [48, 3, 2, 1, 1]]], "head": []}
    seq, _save = ydl.parse_model(d, [3])
    t, dw = seq[1], seq[2]
    # width gain 0.5 on c2 (48 -> 24), c1 from the previous row, no n inserted
    assert type(t) is ydl.ConvTranspose2d and t.weight.shape == (16, 24, 4, 4) and (t.k, t.s, t.p, t.op) == (4, 2, 1, 0)
    assert type(dw) is ydl.DWConvTranspose2d and dw.weight.shape == (24, 1, 3, 3) and (dw.k, dw.s, dw.p, dw.op) == (3, 2, 1, 1)
    assert t.type == "models.common.nn.ConvTranspose2d" and dw.type == "models.common.DWConvTranspose2d"
    assert t.np == 16 * 24 * 16 + 24 and dw.np == 24 * 9 + 24


def test_the_small_yaml_model_builds():
    import torch
    import yolo_dual_amd as ydl
    torch.manual_seed(0)
    net = ydl.SegYoloModel(YAML)
    assert [type(m).__name__ for m in net.model] == ["Conv", "Conv", "C3Common", "Conv", "DWConvTranspose2d", "Concat", "ConvTranspose2d", "Concat",
                                                     "Upsample", "Conv"]
    dw, t, up, last = net.model[4], net.model[6], net.model[8], net.model[9]
    assert dw.weight.shape == (32, 1, 4, 4) and t.weight.shape == (64, 16, 2, 2) and t.bias.shape == (16,)
    assert up.mode == "bicubic" and up.scale_factor == 2 and last.conv.weight.shape == (12, 32, 1, 1)
    # the kaiming pass of the yaml models re-draws nn.Conv2d weights only: the transposed layers keep torch's default initialisation
    bound = 1.0 / (16 * 4) ** 0.5
    assert float(t.weight.detach().abs().max()) <= bound + 1e-6 and t.weight.permute(0, 2, 3, 1).is_contiguous()
    assert net.save == [0, 2]
