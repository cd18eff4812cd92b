"""CPU: the space / depth layers, the bare BatchNorm2d row and BottleneckCSP.  ``Focus``, ``Contract``, ``Expand`` and ``BottleneckCSP``
have the reference's class names, positional signatures and state_dict keys (models/common.py:128-144, 241-250, 282-307), ``BatchNorm2d``
has torch's; every fixture under tests/golden/sd_*.npz (tools/make_sd_golden.py) builds from its recorded arguments; ``parse_model``
resolves the five rows with the reference's channel bookkeeping (models/yolo.py:318-343); ``MixConv2d`` stays refused by name; an
``Expand`` or ``Contract`` that cannot divide raises ValueError naming the class and the number."""
import glob
import os

import numpy as np
import pytest

from tests.block_harness import build_from_json as build, check_state_dict_layout

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "sd_*.npz")))
NAMES = ["sd_bn_24", "sd_contract_g2_c12", "sd_contract_g4_c8", "sd_csp_16_32_n2_noadd", "sd_csp_32_32_n1", "sd_expand_g2_c32",
         "sd_expand_g2_c48", "sd_focus_3_16_k3", "sd_focus_8_24_k1"]
# width 0.5, depth 0.5.  3 x 32 x 32 -> Focus 16 ch @ 16^2 -> BottleneckCSP 32 ch, n = 2 -> Contract(2) 128 ch @ 8^2 -> Conv 64 ch -> Expand(2)
# 16 ch @ 16^2 -> BatchNorm2d -> Concat with the BottleneckCSP (16 + 32 = 48 ch) -> Conv 48 ch, k 3 -> Expand(2): 12 classes @ 32^2
YAML = {"nc": 12, "width_multiple": 0.5, "depth_multiple": 0.5,
        "backbone": [[-1, 1, "Focus", [32, 3]], [-1, 4, "BottleneckCSP", [64]], [-1, 1, "Contract", [2]], [-1, 1, "Conv", [128, 1]]],
        "head": [[-1, 1, "Expand", [2]], [-1, 1, "nn.BatchNorm2d", []], [[-1, 1], 1, "Concat", [1]], [-1, 1, "Conv", [96, 3]],
                 [-1, 1, "Expand", [2]]]}


def has_running_stats(path):
    return any(k.startswith("rv.") for k in np.load(path).files)


def test_the_nine_fixtures_are_present_small_and_carry_the_floors():
    assert [os.path.basename(f)[:-4] for f in FILES] == NAMES
    assert all(os.path.getsize(f) < 128 * 1024 for f in FILES)
    for f in FILES:
        z = np.load(f)
        assert z["x"].shape[0] == 2
        for kind in ("out", "grad") + (("run",) if has_running_stats(f) else ()):
            v = float(z["floor." + kind])
            assert 2.0 ** -10 < v < 0.1, (f, kind, v)


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_class_builds_with_the_reference_state_dict_layout(path):
    z, mod, want = check_state_dict_layout(path, build)
    name = os.path.basename(path)
    if name.startswith(("sd_contract", "sd_expand")):
        assert want == [] and list(mod.parameters()) == []
    if name.startswith("sd_focus"):
        assert [k for k, _ in want] == ["conv.conv.weight"] + ["conv.bn." + n for n in ("weight", "bias", "running_mean", "running_var",
                                                                                        "num_batches_tracked")]
    if name.startswith("sd_csp"):
        keys = dict(want)
        c_ = keys["bn.weight"][0] // 2
        assert keys["cv2.weight"] == (c_, mod.cv1.c1, 1, 1) and keys["cv3.weight"] == (c_, c_, 1, 1)
        assert "cv2.bias" not in keys and "cv3.bias" not in keys and keys["bn.num_batches_tracked"] == ()
        assert type(mod.act).__name__ == "SiLU" and all(type(b).__name__ == "Bottleneck" for b in mod.m)
    if name == "sd_bn_24":
        assert [k for k, _ in want] == ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]


def test_torch_indexing_reproduces_the_fixtures_of_the_parameter_free_layers():
    """Contract / Expand as the two index maps the kernels implement (order 0), against the reference's view / permute results"""
    import json
    from tests.sd_ref import depth_to_space_ref, space_to_depth_ref
    seen = 0
    for f in FILES:
        z = np.load(f)
        cls, s = str(z["cls"]), json.loads(str(z["args"]))[0]
        if cls not in ("Contract", "Expand"):
            continue
        fwd, bwd = (space_to_depth_ref, depth_to_space_ref) if cls == "Contract" else (depth_to_space_ref, space_to_depth_ref)
        assert np.array_equal(fwd(z["x"], s, 0).numpy(), z["out"]) and np.array_equal(bwd(z["grad_out"], s, 0).numpy(), z["grad_x"])
        seen += 1
    assert seen == 4


def test_constructors_and_refusals():
    import torch.nn as nn
    import yolo_dual_amd as ydl
    f = ydl.Focus(3, 16, 3)
    assert type(f.conv) is ydl.Conv and f.conv.conv.weight.shape == (16, 12, 3, 3) and f.conv.p == 1
    assert type(ydl.Focus(8, 24, 1, act=False).conv.act) is nn.Identity
    assert ydl.Contract().gain == 2 and ydl.Expand().gain == 2 and ydl.Contract(1).gain == 1 and ydl.Expand(3).gain == 3
    for cls in (ydl.Contract, ydl.Expand):
        with pytest.raises(ValueError, match=cls.__name__ + ".*gain"):
            cls(0)
    b = ydl.BatchNorm2d(24, 1e-3, 0.03)
    assert isinstance(b, nn.BatchNorm2d) and (b.eps, b.momentum, b.num_features) == (1e-3, 0.03, 24)
    with pytest.raises(NotImplementedError, match="BatchNorm2d.*affine"):
        ydl.BatchNorm2d(24, affine=False)
    csp = ydl.BottleneckCSP(16, 32, 2, False)
    assert isinstance(csp.cv2, nn.Conv2d) and csp.cv2.bias is None and len(csp.m) == 2 and not csp.m[0].add
    assert isinstance(csp.bn, nn.BatchNorm2d) and csp.bn.num_features == 32
    # each half's holder views its own channels of the block's BatchNorm, taken at the call
    assert csp.cv3.bn.weight.data_ptr() == csp.bn.weight.data_ptr()
    assert csp.cv2.bn.running_var.data_ptr() == csp.bn.running_var.data_ptr() + 16 * 4 and csp.cv2.bn.weight.shape == (16,)
    with pytest.raises(NotImplementedError, match="BottleneckCSP.*c_"):
        ydl.BottleneckCSP(16, 24)              # c_ = 12
    for n in ("Focus", "Contract", "Expand", "BottleneckCSP", "BatchNorm2d"):
        assert n in ydl.__all__


def test_the_small_yaml_resolves_with_the_channel_bookkeeping_and_the_gains():
    import torch
    import yolo_dual_amd as ydl
    torch.manual_seed(0)
    net = ydl.SegYoloModel(YAML)
    assert [type(m).__name__ for m in net.model] == ["Focus", "BottleneckCSP", "Contract", "Conv", "Expand", "BatchNorm2d", "Concat", "Conv",
                                                     "Expand"]
    focus, csp, contract, conv3, expand4, bn, _cat, conv7, expand8 = net.model
    assert focus.conv.conv.weight.shape == (16, 12, 3, 3)                       # width gain 32 -> 16, c1 = 4 * 3
    assert csp.c_ == 16 and len(csp.m) == 2 and csp.cv4.conv.weight.shape == (32, 32, 1, 1)      # depth gain 4 -> 2, n inserted
    assert csp.cv2.weight.shape == (16, 16, 1, 1) and csp.bn.num_features == 32
    assert contract.gain == 2 and conv3.conv.weight.shape == (64, 128, 1, 1)    # Contract: 32 * 4 = 128 channels, not scaled
    assert expand4.gain == 2 and bn.num_features == 16                           # Expand: 64 // 4 = 16; BatchNorm2d: args = [ch[f]]
    assert conv7.conv.weight.shape == (48, 48, 3, 3) and expand8.gain == 2      # Concat: 16 + 32 = 48; Expand: 48 // 4 = 12 = nc
    assert net.save == [1]
    assert csp.type == "models.common.BottleneckCSP" and bn.type == "models.common.nn.BatchNorm2d"
    assert contract.np == 0 and expand8.np == 0 and bn.np == 32
    # the kaiming pass re-drew the block's plain convolutions and left every BatchNorm at (1, 0)
    assert bool((csp.bn.weight == 1).all()) and bool((bn.bias == 0).all()) and float(csp.cv3.weight.detach().std()) > 0.1


def test_mixconv2d_is_still_refused_by_name():
    import yolo_dual_amd as ydl
    d = {"nc": 12, "backbone": [[-1, 1, "Conv", [32, 3, 2]], [-1, 1, "MixConv2d", [32]]], "head": []}
    with pytest.raises(NotImplementedError, match="MixConv2d.*outside the segmentation hot path"):
        ydl.parse_model(d, [3])
    for row in ("Detect", "Segment"):
        with pytest.raises(NotImplementedError, match=row):
            ydl.parse_model({"nc": 12, "backbone": [[-1, 1, "Conv", [32, 3, 2]]], "head": [[-1, 1, row, [12]]]}, [3])


def test_indivisible_shapes_raise_value_error_naming_the_class_and_the_number():
    import torch
    import yolo_dual_amd as ydl
    from yolo_dual_amd.tape import Tape, Var

    def var(c, h, w):                                  # a placeholder Var: the layers refuse before any launch
        tape = Tape.__new__(Tape)
        return Var(tape, torch.empty(1).expand(2, c, h, w), c, True)
    with pytest.raises(ValueError, match="Expand.*30"):
        ydl.Expand(2)._fwd(None, var(30, 4, 4))
    with pytest.raises(ValueError, match="Contract.*7"):
        ydl.Contract(2)._fwd(None, var(8, 4, 7))
    with pytest.raises(ValueError, match="Focus.*5"):
        ydl.Focus(8, 16)._fwd(None, var(8, 5, 4))
