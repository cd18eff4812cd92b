"""CPU: the ConvNeXt modules.  ``LayerNorm2d``, ``CNBlock`` and the rows ``convnext_tiny1`` / ``2`` / ``3`` (models/common.py:1241-1269)
have torchvision's state_dict keys and shapes; the optimizer's three groups come out as in utils/torch_utils.py:318-346; the parameter
counts follow from the shapes; the per-block stochastic-depth probabilities are 0.1 j / 17; the key map round-trips a synthetic
``features.*`` dict; ``parse_model`` resolves the backbone rows of models/backbone/convnext_tiny.yaml with ``c2 = args[0]``; a 30 x 30
input raises ValueError naming the class and the number; ``ydl_ln_supported`` answers on the host; the recorded-step paths refuse a
training model with stochastic depth.

A module's own parameters precede its children's in torch's state_dict, so ``layer_scale`` comes first in a CNBlock's keys, as in
torchvision's own; the keys and shapes are the listed ones."""
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "convnext_*.npz")))
NAMES = ["convnext_cnblock_16", "convnext_cnblock_24_keep", "convnext_down_16_32", "convnext_stem_3_16"]

# the backbone rows of models/backbone/convnext_tiny.yaml and a small head: SPPF, a 1x1 Conv, an up-sampling, the concat with the second
# row's output and a 12-channel 1x1
YAML = {"nc": 12, "depth_multiple": 1.0, "width_multiple": 1.0,
        "backbone": [[-1, 1, "convnext_tiny1", [192]], [-1, 1, "convnext_tiny2", [384]], [-1, 1, "convnext_tiny3", [768]],
                     [-1, 1, "SPPF", [64, 5]]],
        "head": [[-1, 1, "Conv", [32, 1, 1]], [-1, 1, "nn.Upsample", ["None", 2, "nearest"]], [[-1, 1], 1, "Concat", [1]],
                 [-1, 1, "Conv", [12, 1, 1]]]}


def build(z):
    """the module a fixture describes: CNBlock by its arguments (a recorded keep vector replaces the draw), the stem and a
    down-sampling layer as the rows build them"""
    import yolo_dual_amd as ydl
    from yolo_dual_amd import modules as M
    cls, args = str(z["cls"]), json.loads(str(z["args"]))
    if cls == "CNBlock":
        mod = ydl.CNBlock(*args)
        if "keep" in z.files:
            keep = torch.from_numpy(z["keep"]).float()
            mod.draw_keep = lambda N, device: keep.to(device)
        return mod
    if cls == "stem":
        return nn.Sequential(M._PatchConv2d(*args), ydl.LayerNorm2d(args[1]))
    assert cls == "down"
    return nn.Sequential(ydl.LayerNorm2d(args[0]), M._PatchConv2d(args[0], args[1], 2))


def cnblock_keys(d):
    return [("block.0.weight", (d, 1, 7, 7)), ("block.0.bias", (d,)), ("block.2.weight", (d,)), ("block.2.bias", (d,)),
            ("block.3.weight", (4 * d, d)), ("block.3.bias", (4 * d,)), ("block.5.weight", (d, 4 * d)), ("block.5.bias", (d,)),
            ("layer_scale", (d, 1, 1))]


def test_the_fixtures_are_present_small_and_carry_the_floors():
    assert [os.path.basename(f)[:-4] for f in FILES] == NAMES
    assert all(os.path.getsize(f) < 128 * 1024 for f in FILES)
    for f in FILES:
        z = np.load(f)
        for kind in ("out", "grad"):
            assert 2.0 ** -10 < float(z["floor." + kind]) < 0.1, (f, kind)
        if "layer_scale" in [str(k) for k in z["keys"]]:
            assert float(np.abs(z["p.layer_scale"]).min()) >= 0.5            # of order 1: the branch shows in the output
    assert 0.0 in np.load(os.path.join(GOLDEN, "convnext_cnblock_24_keep.npz"))["keep"]


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_modules_build_with_the_recorded_state_dict_layout(path):
    from tests.block_harness import check_state_dict_layout
    check_state_dict_layout(path, build)


def test_cnblock_and_layer_norm_state_dict_keys_and_shapes():
    import yolo_dual_amd as ydl
    blk = ydl.CNBlock(24)
    got = [(k, tuple(v.shape)) for k, v in blk.state_dict().items()]
    want = cnblock_keys(24)
    assert got == want[-1:] + want[:-1]              # torch lists a module's own parameter before its children's
    assert sum(p.numel() for p in blk.parameters()) == 8 * 24 * 24 + 58 * 24
    assert float(blk.layer_scale.max()) == pytest.approx(1e-6) and blk.block[2].eps == 1e-6
    ln = ydl.LayerNorm2d(96)
    assert [(k, tuple(v.shape)) for k, v in ln.state_dict().items()] == [("weight", (96,)), ("bias", (96,))] and ln.eps == 1e-6
    assert bool((ln.weight == 1).all()) and bool((ln.bias == 0).all())
    for bad in (12, 4, 1032):
        with pytest.raises(ValueError, match="LayerNorm2d.*multiple of 8"):
            ydl.LayerNorm2d(bad)
    with pytest.raises(ValueError, match="CNBlock.*dim"):
        ydl.CNBlock(20)
    with pytest.raises(ValueError, match="stochastic_depth_prob"):
        ydl.CNBlock(16, stochastic_depth_prob=1.0)
    for n in ("LayerNorm2d", "CNBlock", "convnext_tiny1", "convnext_tiny2", "convnext_tiny3", "convnext_key_map"):
        assert n in ydl.__all__


def _rows():
    import yolo_dual_amd as ydl
    return [ydl.convnext_tiny1(192), ydl.convnext_tiny2(384), ydl.convnext_tiny3(768)]


def test_rows_have_the_slices_of_convnext_tiny():
    rows = _rows()
    assert [sum(p.numel() for p in r.parameters()) for r in rows] == [1235040, 11112960, 15470592]
    assert sum(p.numel() for r in rows for p in r.parameters()) == 27818592
    sd = {k: tuple(v.shape) for k, v in rows[0].state_dict().items()}
    assert sd["model.0.0.weight"] == (96, 3, 4, 4) and sd["model.0.0.bias"] == (96,) and sd["model.0.1.weight"] == (96,)
    assert sd["model.2.0.weight"] == (96,) and sd["model.2.1.weight"] == (192, 96, 2, 2) and sd["model.2.1.bias"] == (192,)
    for part, n, d in ((1, 3, 96), (3, 3, 192)):
        for j in range(n):
            for k, shape in cnblock_keys(d):
                assert sd[f"model.{part}.{j}.{k}"] == shape
    assert len(sd) == 4 + 4 + 6 * 9
    for row, n, (cin, d) in ((rows[1], 9, (192, 384)), (rows[2], 3, (384, 768))):
        sd = {k: tuple(v.shape) for k, v in row.state_dict().items()}
        assert sd["model.0.0.weight"] == (cin,) and sd["model.0.1.weight"] == (d, cin, 2, 2) and len(sd) == 4 + 9 * n
        assert all(sd[f"model.1.{j}.{k}"] == shape for j in range(n) for k, shape in cnblock_keys(d))
    ps = [m.stochastic_depth_prob for r in rows for m in r.modules() if type(m).__name__ == "CNBlock"]
    assert len(ps) == 18 and all(abs(p - 0.1 * j / 17) < 1e-12 for j, p in enumerate(ps))
    import yolo_dual_amd as ydl
    assert all(m.stochastic_depth_prob == 0.0 for m in ydl.convnext_tiny2(stochastic_depth_prob=0.0).modules() if type(m).__name__ == "CNBlock")
    # torchvision's init: truncated normal 0.02 for conv and linear weights, zero biases, LayerNorm at (1, 0), layer_scale 1e-6
    r = rows[0]
    assert 0.015 < float(r.model[0][0].weight.std()) < 0.025 and 0.015 < float(r.model[2][1].weight.std()) < 0.025
    assert 0.015 < float(r.model[1][0].block[3].weight.std()) < 0.025 and bool((r.model[1][0].block[3].bias == 0).all())
    assert bool((r.model[1][0].block[0].bias == 0).all()) and float(r.model[3][2].layer_scale.max()) == pytest.approx(1e-6)
    assert float(ydl.convnext_tiny3(layer_scale=0.5).model[1][0].layer_scale.min()) == 0.5


def test_the_optimizer_groups_follow_the_reference_rule():
    """utils/torch_utils.py:318-346: every parameter named ``bias`` in the bias group, the ``weight`` of a module whose class name contains
    "Norm" in the no-decay group, everything else (layer_scale included) decayed -- read off the module tree as the optimizer does"""
    from yolo_dual_amd.optim import _is_bn
    row = _rows()[0]
    g = {"bias": [], "norm": [], "decay": []}
    for name, mod in row.named_modules():
        for pname, p in mod.named_parameters(recurse=False):
            g["bias" if pname == "bias" else "norm" if pname == "weight" and _is_bn(mod) else "decay"].append(f"{name}.{pname}")
    n_blocks = 6
    assert len(g["bias"]) == 4 * n_blocks + 4                 # dw, LayerNorm, fc1, fc2 of every block; stem and down conv + LayerNorm
    assert len(g["norm"]) == n_blocks + 2 and all(k.endswith((".block.2.weight", "model.0.1.weight", "model.2.0.weight")) for k in g["norm"])
    assert len(g["decay"]) == 4 * n_blocks + 2 and sum(k.endswith("layer_scale") for k in g["decay"]) == n_blocks
    assert sorted(sum(g.values(), [])) == sorted(k for k, _ in row.named_parameters())


def test_the_key_map_round_trips_a_synthetic_features_dict():
    import yolo_dual_amd as ydl
    rows = _rows()
    km = ydl.convnext_key_map()
    assert len(km) == sum(len(r.state_dict()) for r in rows) and all(k.startswith("features.") for k in km)
    assert km["features.0.0.weight"] == (0, "model.0.0.weight") and km["features.3.2.layer_scale"] == (0, "model.3.2.layer_scale")
    assert km["features.4.1.bias"] == (1, "model.0.1.bias") and km["features.5.8.block.5.weight"] == (1, "model.1.8.block.5.weight")
    assert km["features.6.0.weight"] == (2, "model.0.0.weight") and km["features.7.2.block.0.weight"] == (2, "model.1.2.block.0.weight")
    gen = torch.Generator().manual_seed(0)
    shapes = {k: rows[r].state_dict()[kk].shape for k, (r, kk) in km.items()}
    full = {k: torch.randn(s, generator=gen) for k, s in shapes.items()}
    full["classifier.2.weight"] = torch.randn(10, 768, generator=gen)           # not a backbone key: left out
    assert set(ydl.convnext_key_map(full)) == set(km)
    parts = [{}, {}, {}]
    for k, (r, kk) in ydl.convnext_key_map(full).items():
        parts[r][kk] = full[k]
    for r, row in enumerate(rows):
        row.load_state_dict(parts[r])                    # strict: every key present, none left over
        back = {k: v for k, v in row.state_dict().items()}
        assert all(torch.equal(back[kk], full[k]) for k, (rr, kk) in km.items() if rr == r)
    assert rows[0].model[0][0].weight.permute(0, 2, 3, 1).is_contiguous()        # the patch conv's weight stays the KRSC master


def test_parse_model_resolves_the_backbone_rows():
    import yolo_dual_amd as ydl
    torch.manual_seed(0)
    net = ydl.SegYoloModel(YAML)
    assert [type(m).__name__ for m in net.model] == ["convnext_tiny1", "convnext_tiny2", "convnext_tiny3", "SPPF", "Conv", "Upsample", "Concat",
                                                     "Conv"]
    r1, r2, r3, sppf, c4, _up, _cat, c7 = net.model
    assert r2.model[0][1].weight.shape == (384, 192, 2, 2) and r3.model[0][1].weight.shape == (768, 384, 2, 2)
    assert sppf.cv1.conv.weight.shape[1] == 768                                  # c2 = args[0]: 192 / 384 / 768 without the width gain
    assert c4.conv.weight.shape == (32, 64, 1, 1) and c7.conv.weight.shape == (12, 32 + 384, 1, 1)
    assert net.save == [1]
    assert r1.type == "models.common.convnext_tiny1" and [r.np for r in (r1, r2, r3)] == [1235040, 11112960, 15470592]
    # the kaiming pass of the yaml model left the rows' own initialisation alone; fuse() skips them
    # (kaiming_normal_ with fan_out would give 0.036 and 0.051 here)
    assert 0.015 < float(r1.model[0][0].weight.std()) < 0.025 and 0.015 < float(r1.model[2][1].weight.std()) < 0.025
    # with a width gain the rows' channels stay as written
    d = dict(YAML, width_multiple=0.25, head=[])
    d["backbone"] = YAML["backbone"][:3] + [[-1, 1, "Conv", [64, 1, 1]]]
    layers, _save = ydl.parse_model(d, [3])
    assert layers[3].conv.weight.shape == (16, 768, 1, 1)


def test_a_30x30_input_raises_value_error_naming_the_class_and_the_number():
    import yolo_dual_amd as ydl
    from yolo_dual_amd import modules as M
    from yolo_dual_amd.tape import Tape, Var

    def var(c, h, w):                                  # a placeholder Var: the layers refuse before any launch
        return Var(Tape.__new__(Tape), torch.empty(1).expand(2, c, h, w), c, False)
    with pytest.raises(ValueError, match="convnext_tiny1.*30 x 30.*8"):
        ydl.convnext_tiny1(192)._fwd(None, var(3, 30, 30))
    with pytest.raises(ValueError, match="convnext_tiny2.*5 x 4.*2"):
        ydl.convnext_tiny2(384)._fwd(None, var(192, 5, 4))
    with pytest.raises(ValueError, match=r"Conv2d\(3, 16, 4, 4\).*30 x 30.*4"):
        M._PatchConv2d(3, 16, 4)._fwd(None, var(3, 30, 30))


def test_ln_supported_answers_on_the_host():
    from yolo_dual_amd import _lib as L
    lib = L.lib()
    assert [c for c in (0, 4, 8, 12, 96, 192, 384, 768, 1024, 1032, 2048) if lib.ydl_ln_supported(c)] == [8, 96, 192, 384, 768, 1024]
    assert lib.ydl_ln_bwd_ws_bytes(30, 24) == 2 * 3 * 24 * 4 and lib.ydl_ln_bwd_ws_bytes(30, 12) == 0
    assert lib.ydl_bias_gelu_bwd_ws_bytes(30, 96) == 30 * 96 * 4 and lib.ydl_scale_res_bwd_ws_bytes(2, 100000, 8) == 1024 * 8 * 4


def test_the_recorded_step_paths_refuse_stochastic_depth_in_training():
    import yolo_dual_amd as ydl
    from yolo_dual_amd.modules import refuse_stochastic_depth
    row = ydl.convnext_tiny2(384).train()
    with pytest.raises(NotImplementedError, match="stochastic depth"):
        refuse_stochastic_depth(row, "a launch list")
    refuse_stochastic_depth(row.eval(), "a launch list")
    refuse_stochastic_depth(ydl.convnext_tiny2(384, stochastic_depth_prob=0.0).train(), "graph capture")
    import inspect
    from yolo_dual_amd import graph, replay
    assert "refuse_stochastic_depth(model" in inspect.getsource(replay.ReplayedTrainStep.__init__)
    assert "refuse_stochastic_depth(model" in inspect.getsource(graph.GraphedTrainStep.__init__)
