"""CPU: the squeeze-excitation modules.  ``SqueezeExcitation``, ``Conv2dNormActivation``, ``InvertedResidual``, ``MBConv`` and the rows
``MobileNetV3s1`` / ``2`` / ``3`` and ``efficientnet_b01`` / ``2`` / ``3`` (models/common.py:870-936) have torchvision's state_dict keys
and shapes, written out here from the tables of mobilenet_v3_small and efficientnet_b0; the parameter counts are torchvision's
(927 008 and 4 007 548 without the classifiers); BatchNorm eps / momentum are 1e-3 / 0.01 in the MobileNetV3 rows and the defaults in
EfficientNet's; the stochastic-depth probabilities are 0.2 j / 16; the key maps round-trip a synthetic ``features.*`` dict;
``parse_model`` resolves both backbone yamls' rows with ``c2 = args[0]``; the wrappers that are not built are refused by name; a map that
does not divide by a row's stride raises ValueError naming the class and the number; the host functions of csrc/se.hip answer; the
recorded-step paths refuse a training model with stochastic depth."""
import glob
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "se_*.npz")))
NAMES = ["se_gate_16_8_hsig", "se_gate_96_4_sig", "se_ir_16_s2", "se_ir_40_res", "se_mbconv_24_40_s2", "se_mbconv_24_keep"]


def _yaml(rows, chans):
    """the three backbone rows of models/backbone/<family>.yaml and a short head: SPPF, a 1x1 Conv, an up-sampling, the concat with the
    second row's output and a 12-channel 1x1"""
    return {"nc": 12, "depth_multiple": 1.0, "width_multiple": 1.0,
            "backbone": [[-1, 1, r, [c]] for r, c in zip(rows, chans)] + [[-1, 1, "SPPF", [64, 5]]],
            "head": [[-1, 1, "Conv", [32, 1, 1]], [-1, 1, "nn.Upsample", ["None", 2, "nearest"]], [[-1, 1], 1, "Concat", [1]],
                     [-1, 1, "Conv", [12, 1, 1]]]}


YAML_MNV3 = _yaml(("MobileNetV3s1", "MobileNetV3s2", "MobileNetV3s3"), (24, 48, 576))
YAML_EFF = _yaml(("efficientnet_b01", "efficientnet_b02", "efficientnet_b03"), (40, 112, 1280))


def build(z):
    """the module a fixture describes, by its class and arguments (a recorded keep vector replaces the draw)"""
    import yolo_dual_amd as ydl
    mod = getattr(ydl, str(z["cls"]))(*json.loads(str(z["args"])))
    if "keep" in z.files:
        keep = torch.from_numpy(z["keep"]).float()
        mod.draw_keep = lambda N, device: keep.to(device)
    return mod


def cna_keys(prefix, c1, c2, k, groups=1):
    return [(prefix + "0.weight", (c2, c1 // groups, k, k))] + [(prefix + "1." + n, s) for n, s in (
        ("weight", (c2,)), ("bias", (c2,)), ("running_mean", (c2,)), ("running_var", (c2,)), ("num_batches_tracked", ()))]


def se_keys(prefix, c, cs):
    return [(prefix + "fc1.weight", (cs, c, 1, 1)), (prefix + "fc1.bias", (cs,)), (prefix + "fc2.weight", (c, cs, 1, 1)), (prefix + "fc2.bias", (c,))]


def block_keys(prefix, cin, k, exp, cout, cs):
    """[expand], depth-wise, [SE when cs], project -- under block.0, block.1, ..."""
    out, i = [], 0
    if exp != cin:
        out += cna_keys(f"{prefix}block.{i}.", cin, exp, 1)
        i += 1
    out += cna_keys(f"{prefix}block.{i}.", exp, exp, k, exp)
    i += 1
    if cs:
        out += se_keys(f"{prefix}block.{i}.", exp, cs)
        i += 1
    return out + cna_keys(f"{prefix}block.{i}.", exp, cout, 1)


# mobilenet_v3_small features[1..11]: (in, kernel, expanded, out, squeeze width or 0, stride)
MNV3 = [(16, 3, 16, 16, 8, 2), (16, 3, 72, 24, 0, 2), (24, 3, 88, 24, 0, 1), (24, 5, 96, 40, 24, 2), (40, 5, 240, 40, 64, 1),
        (40, 5, 240, 40, 64, 1), (40, 5, 120, 48, 32, 1), (48, 5, 144, 48, 40, 1), (48, 5, 288, 96, 72, 2), (96, 5, 576, 96, 144, 1),
        (96, 5, 576, 96, 144, 1)]
# efficientnet_b0 blocks in order: (expand ratio, kernel, stride, in, out, squeeze width), stage boundaries after 1, 3, 5, 8, 11, 15, 16
EFF = [(1, 3, 1, 32, 16, 8), (6, 3, 2, 16, 24, 4), (6, 3, 1, 24, 24, 6), (6, 5, 2, 24, 40, 6), (6, 5, 1, 40, 40, 10), (6, 3, 2, 40, 80, 10),
       (6, 3, 1, 80, 80, 20), (6, 3, 1, 80, 80, 20), (6, 5, 1, 80, 112, 20), (6, 5, 1, 112, 112, 28), (6, 5, 1, 112, 112, 28),
       (6, 5, 2, 112, 192, 28), (6, 5, 1, 192, 192, 48), (6, 5, 1, 192, 192, 48), (6, 5, 1, 192, 192, 48), (6, 3, 1, 192, 320, 48)]
EFF_STAGES = [1, 2, 2, 3, 3, 4, 1]


def mnv3_row_keys(first, last):
    out = []
    for j, n in enumerate(range(first, last)):
        if n == 0:
            out += cna_keys(f"model.{j}.", 3, 16, 3)
        elif n == 12:
            out += cna_keys(f"model.{j}.", 96, 576, 1)
        else:
            cin, k, exp, cout, cs, _s = MNV3[n - 1]
            out += block_keys(f"model.{j}.", cin, k, exp, cout, cs)
    return out


def eff_row_keys(first, last):
    out = []
    for j, n in enumerate(range(first, last)):
        if n == 0:
            out += cna_keys(f"model.{j}.", 3, 32, 3)
        elif n == 8:
            out += cna_keys(f"model.{j}.", 320, 1280, 1)
        else:
            b0 = sum(EFF_STAGES[:n - 1])
            for r in range(EFF_STAGES[n - 1]):
                ratio, k, _s, cin, cout, cs = EFF[b0 + r]
                out += block_keys(f"model.{j}.{r}.", cin, k, cin * ratio, cout, cs)
    return out


def _shapes(mod):
    return [(k, tuple(v.shape)) for k, v in mod.state_dict().items()]


def test_the_fixtures_are_present_small_and_carry_the_floors():
    assert [os.path.basename(f)[:-4] for f in FILES] == NAMES
    assert all(os.path.getsize(f) < 512 * 1024 for f in FILES)
    for f in FILES:
        z = np.load(f)
        for kind in ("out", "grad") + (("run",) if "InvertedResidual" in str(z["cls"]) or "MBConv" in str(z["cls"]) else ()):
            assert 2.0 ** -11 < float(z["floor." + kind]) < 0.1, (f, kind)
        for k in (str(k) for k in z["keys"]):
            if k.endswith(("fc1.bias", "fc2.bias")):
                assert float(np.abs(z["p." + k]).max()) > 0.2, k                # away from the trivial value
    assert 0.0 in np.load(os.path.join(GOLDEN, "se_mbconv_24_keep.npz"))["keep"]


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_modules_build_with_the_recorded_state_dict_layout(path):
    from tests.block_harness import check_state_dict_layout
    check_state_dict_layout(path, build)


def test_block_state_dict_keys_and_shapes():
    import yolo_dual_amd as ydl
    assert _shapes(ydl.SqueezeExcitation(96, 4, "silu", "sigmoid")) == se_keys("", 96, 4)
    assert _shapes(ydl.Conv2dNormActivation(16, 72, 1)) == cna_keys("", 16, 72, 1)
    assert _shapes(ydl.Conv2dNormActivation(72, 72, 5, 2, 72, "hardswish")) == cna_keys("", 72, 72, 5, 72)
    assert _shapes(ydl.InvertedResidual(16, 3, 16, 16, True, "RE", 2)) == block_keys("", 16, 3, 16, 16, 8)
    assert _shapes(ydl.InvertedResidual(40, 5, 240, 40, True, "HS", 1)) == block_keys("", 40, 5, 240, 40, 64)
    assert _shapes(ydl.InvertedResidual(16, 3, 72, 24, False, "RE", 2)) == block_keys("", 16, 3, 72, 24, 0)
    assert _shapes(ydl.MBConv(6, 5, 2, 24, 40)) == block_keys("", 24, 5, 144, 40, 6)
    assert _shapes(ydl.MBConv(1, 3, 1, 32, 16)) == block_keys("", 32, 3, 32, 16, 8)
    ir, mb = ydl.InvertedResidual(40, 5, 240, 40, True, "HS", 1), ydl.MBConv(6, 3, 1, 24, 24, 0.3)
    assert ir.use_res_connect and mb.use_res_connect and not ydl.MBConv(6, 5, 2, 24, 40).use_res_connect and mb.stochastic_depth_prob == 0.3
    se = ir.block[2]
    assert (se.act_code, se.gate_code) == (2, 1) and (mb.block[2].act_code, mb.block[2].gate_code) == (1, 0)     # RELU / HSIGMOID, SILU / SIGMOID
    assert type(ir.block[0].act).__name__ == "Hardswish" and type(ir.block[3].act).__name__ == "Identity"
    # a Conv2dNormActivation is a Conv to the rest of the project: conv / bn readable, the weight the KRSC master
    cna = ir.block[0]
    assert isinstance(cna, ydl.Conv) and cna.conv is cna._modules["0"] and cna.bn is cna._modules["1"]
    assert cna.conv.weight.permute(0, 2, 3, 1).is_contiguous() and bool((se.fc1.bias == 0).all())
    with pytest.raises(ValueError, match="SqueezeExcitation.*multiple of 8"):
        ydl.SqueezeExcitation(12, 4)
    with pytest.raises(ValueError, match="SqueezeExcitation.*1..512"):
        ydl.SqueezeExcitation(16, 0)
    with pytest.raises(NotImplementedError, match="scale_activation"):
        ydl.SqueezeExcitation(16, 4, "relu", "tanh")
    with pytest.raises(NotImplementedError, match="InvertedResidual.*activation"):
        ydl.InvertedResidual(16, 3, 16, 16, True, "R6", 1)
    with pytest.raises(ValueError, match="stochastic_depth_prob"):
        ydl.MBConv(6, 3, 1, 24, 24, 1.0)
    for n in ("SqueezeExcitation", "Conv2dNormActivation", "InvertedResidual", "MBConv", "MobileNetV3s1", "MobileNetV3s2", "MobileNetV3s3",
              "efficientnet_b01", "efficientnet_b02", "efficientnet_b03", "mobilenet_v3_small_key_map", "efficientnet_b0_key_map"):
        assert n in ydl.__all__


def _mn_rows():
    import yolo_dual_amd as ydl
    return [ydl.MobileNetV3s1(24), ydl.MobileNetV3s2(48), ydl.MobileNetV3s3(576)]


def _eff_rows(**kw):
    import yolo_dual_amd as ydl
    return [ydl.efficientnet_b01(40, **kw), ydl.efficientnet_b02(112, **kw), ydl.efficientnet_b03(1280, **kw)]


def test_rows_have_the_slices_of_mobilenet_v3_small():
    rows = _mn_rows()
    for row, (a, b) in zip(rows, ((0, 4), (4, 9), (9, 13))):
        assert _shapes(row) == mnv3_row_keys(a, b)
    assert [sum(p.numel() for p in r.parameters()) for r in rows] == [10488, 180032, 736488]              # 927 008: torchvision's features
    bns = [m for r in rows for m in r.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 34 and all(m.eps == 1e-3 and m.momentum == 0.01 for m in bns)
    ses = [m.fc1.out_channels for r in rows for m in r.modules() if type(m).__name__ == "SqueezeExcitation"]
    assert ses == [8, 24, 64, 64, 32, 40, 72, 144, 144]


def test_rows_have_the_slices_of_efficientnet_b0():
    rows = _eff_rows()
    for row, (a, b) in zip(rows, ((0, 4), (4, 6), (6, 9))):
        assert _shapes(row) == eff_row_keys(a, b)
    assert [sum(p.numel() for p in r.parameters()) for r in rows] == [65730, 786078, 3155740]             # 4 007 548: torchvision's features
    bns = [m for r in rows for m in r.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 49 and all(m.eps == 1e-5 and m.momentum == 0.1 for m in bns)
    ses = [m.fc1.out_channels for r in rows for m in r.modules() if type(m).__name__ == "SqueezeExcitation"]
    assert ses == [e[5] for e in EFF]
    ps = [m.stochastic_depth_prob for r in rows for m in r.modules() if type(m).__name__ == "MBConv"]
    assert len(ps) == 16 and all(abs(p - 0.2 * j / 16) < 1e-12 for j, p in enumerate(ps))
    assert all(m.stochastic_depth_prob == 0.0 for r in _eff_rows(stochastic_depth_prob=0.0) for m in r.modules() if type(m).__name__ == "MBConv")


@pytest.mark.parametrize("family", ["mobilenet_v3_small", "efficientnet_b0"])
def test_the_key_maps_round_trip_a_synthetic_features_dict(family):
    import yolo_dual_amd as ydl
    rows, fn = (_mn_rows(), ydl.mobilenet_v3_small_key_map) if family == "mobilenet_v3_small" else (_eff_rows(), ydl.efficientnet_b0_key_map)
    km = fn()
    assert len(km) == sum(len(r.state_dict()) for r in rows) and all(k.startswith("features.") for k in km)
    if family == "mobilenet_v3_small":
        assert km["features.0.0.weight"] == (0, "model.0.0.weight") and km["features.4.block.2.fc1.bias"] == (1, "model.0.block.2.fc1.bias")
        assert km["features.12.1.running_var"] == (2, "model.3.1.running_var")
    else:
        assert km["features.1.0.block.1.fc2.weight"] == (0, "model.1.0.block.1.fc2.weight")
        assert km["features.5.2.block.3.1.bias"] == (1, "model.1.2.block.3.1.bias") and km["features.8.0.weight"] == (2, "model.2.0.weight")
    gen = torch.Generator().manual_seed(0)
    full = {}
    for k, (r, kk) in km.items():
        v = rows[r].state_dict()[kk]
        full[k] = torch.randn(v.shape, generator=gen) if v.dtype.is_floating_point else torch.tensor(7)
    full["classifier.0.weight"] = torch.randn(10, 8, generator=gen)                  # not a backbone key: left out
    assert set(fn(full)) == set(km)
    parts = [{}, {}, {}]
    for k, (r, kk) in fn(full).items():
        parts[r][kk] = full[k]
    for r, row in enumerate(rows):
        row.load_state_dict(parts[r])                    # strict: every key present, none left over
        back = row.state_dict()
        assert all(torch.equal(back[kk], full[k]) for k, (rr, kk) in km.items() if rr == r)


@pytest.mark.parametrize("cfg,names,chans", [(YAML_MNV3, ("MobileNetV3s1", "MobileNetV3s2", "MobileNetV3s3"), (24, 48, 576)),
                                             (YAML_EFF, ("efficientnet_b01", "efficientnet_b02", "efficientnet_b03"), (40, 112, 1280))])
def test_parse_model_resolves_the_backbone_rows(cfg, names, chans):
    import yolo_dual_amd as ydl
    torch.manual_seed(0)
    net = ydl.SegYoloModel(cfg)
    assert [type(m).__name__ for m in net.model] == list(names) + ["SPPF", "Conv", "Upsample", "Concat", "Conv"]
    r1, r2, r3, sppf, c4, _up, _cat, c7 = net.model
    assert sppf.cv1.conv.weight.shape[1] == chans[2]                              # c2 = args[0], without the width gain
    assert c4.conv.weight.shape == (32, 64, 1, 1) and c7.conv.weight.shape == (12, 32 + chans[1], 1, 1)
    assert net.save == [1] and r1.type == "models.common." + names[0]
    # every parameter is an ordinary one under torchvision's name; the builder's initialisation: kaiming fan-out, zero SE biases
    se = [m for m in r1.modules() if type(m).__name__ == "SqueezeExcitation"][0]
    assert bool((se.fc1.bias == 0).all()) and float(se.fc1.weight.detach().std()) > 0
    d = dict(cfg, width_multiple=0.25, head=[])
    d["backbone"] = cfg["backbone"][:3] + [[-1, 1, "Conv", [64, 1, 1]]]
    layers, _save = ydl.parse_model(d, [3])
    assert layers[3].conv.weight.shape == (16, chans[2], 1, 1)
    stem = r1.model[0]                                                            # fuse() reads conv / bn under their new names
    assert stem.fuse()._fused["w"].shape == (stem.c2, 3, 3, 3) and stem.unfuse()._fused is None


@pytest.mark.parametrize("name,why", [("efficientnet_b11", "B0"), ("efficientnet_b13", "B0"), ("efficientnet_v2_s2", "FusedMBConv"),
                                      ("RegNety4001", "group width 8"), ("RegNety4003", "group width 8"), ("mobilenet_v22", "ReLU6"),
                                      ("resnet181", "ResNet"), ("resnet342", "ResNet"), ("resnet503", "ResNet"),
                                      ("wide_resnet50_21", "ResNet"), ("vgg11_bn1", "VGG"), ("vgg11_bn3", "VGG")])
def test_wrappers_that_are_not_built_are_refused_by_name(name, why):
    import yolo_dual_amd as ydl
    d = {"nc": 12, "depth_multiple": 1.0, "width_multiple": 1.0, "backbone": [[-1, 1, name, [64]]], "head": []}
    with pytest.raises(NotImplementedError, match=f"{name} is not served.*{why}"):
        ydl.parse_model(d, [3])


def test_a_map_that_does_not_divide_by_the_stride_raises_value_error_naming_the_class_and_the_number():
    import yolo_dual_amd as ydl
    from yolo_dual_amd.tape import Tape, Var

    def var(c, h, w):                                  # a placeholder Var: the rows refuse before any launch
        return Var(Tape.__new__(Tape), torch.empty(1).expand(2, c, h, w), c, False)
    with pytest.raises(ValueError, match="MobileNetV3s1.*30 x 30.*8"):
        ydl.MobileNetV3s1(24)._fwd(None, var(3, 30, 30))
    with pytest.raises(ValueError, match="MobileNetV3s2.*5 x 4.*2"):
        ydl.MobileNetV3s2(48)._fwd(None, var(24, 5, 4))
    with pytest.raises(ValueError, match="efficientnet_b01.*36 x 32.*8"):
        ydl.efficientnet_b01(40)._fwd(None, var(3, 36, 32))
    with pytest.raises(ValueError, match="efficientnet_b03.*3 x 3.*2"):
        ydl.efficientnet_b03(1280)._fwd(None, var(112, 3, 3))


def test_the_host_functions_answer():
    from yolo_dual_amd import _lib as L
    lib = L.lib()
    ok = [(c, cs) for c, cs in ((0, 4), (8, 1), (12, 4), (16, 0), (96, 4), (1152, 48), (2048, 512), (2056, 8), (64, 513)) if lib.ydl_se_supported(c, cs)]
    assert ok == [(8, 1), (96, 4), (1152, 48), (2048, 512)]
    # about 64 pixels per slice, at most 64 slices and 1024 / N
    assert [lib.ydl_se_pool_splits(n, hw) for n, hw in ((1, 1), (2, 15), (1, 257), (3, 4099), (16, 102400), (64, 6400), (2000, 100))] == \
        [1, 1, 5, 64, 64, 16, 1]
    assert lib.ydl_se_pool_ws_bytes(3, 4099, 24) == 3 * 64 * 24 * 4 and lib.ydl_se_pool_ws_bytes(3, 4099, 12) == 0
    assert lib.ydl_se_excite_bwd_ws_bytes(16, 1152, 48) == 16 * 1200 * 4 and lib.ydl_se_excite_bwd_ws_bytes(16, 1150, 48) == 0


def test_the_recorded_step_paths_refuse_stochastic_depth_in_training():
    import yolo_dual_amd as ydl
    from yolo_dual_amd.modules import refuse_stochastic_depth
    row = ydl.efficientnet_b02(112).train()
    with pytest.raises(NotImplementedError, match="stochastic depth.*MBConv"):
        refuse_stochastic_depth(row, "a launch list")
    refuse_stochastic_depth(row.eval(), "a launch list")
    refuse_stochastic_depth(ydl.efficientnet_b02(112, stochastic_depth_prob=0.0).train(), "graph capture")
    refuse_stochastic_depth(ydl.MobileNetV3s2(48).train(), "graph capture")
    # a block without the residual draws nothing, whatever its probability
    refuse_stochastic_depth(ydl.MBConv(6, 5, 2, 24, 40, 0.3).train(), "a launch list")
