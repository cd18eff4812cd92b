"""CPU: the Conv activations.  ``Conv`` takes LeakyReLU(slope), Hardswish, Mish (torch's classes or those of
yolo_dual_amd.activations), AconC and FReLU; the activation classes have the reference's constructor signatures, parameter shapes and
state_dict keys (key lists and shapes recorded from the reference's own classes by tools/make_act_golden.py); a yaml's ``activation:``
key sets the default activation of every Conv of that model and of no later one; a string activation in a row's arguments is resolved
by a parser, not evaluated; what is not served is refused by name; the six streaming BatchNorm entry points without an act_param refuse
YDL_ACT_LEAKY on the host; the replay table is current."""
import ctypes
import glob
import importlib.util
import json
import os
import re

import numpy as np
import pytest

from tests.block_harness import check_state_dict_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "act_*.npz")))
NAMES = ["act_c3_leaky_32_32_n1", "act_conv_acon_16_20_k1", "act_conv_acon_16_24_k3", "act_conv_frelu_16_24_k3", "act_conv_hswish_16_24_k1",
         "act_conv_leaky_16_24_k3", "act_conv_mish_16_16_k3_s2", "act_dwconv_hswish_16_16_k3_s2"]
# 3 x 32 x 32 input -> 16 ch @ 16^2 -> 32 ch @ 8^2 -> C3 with one Bottleneck (shortcut) -> SPPF -> 12 classes
YAML = {"nc": 12, "width_multiple": 0.5, "depth_multiple": 0.33, "activation": "nn.LeakyReLU(0.1)",
        "backbone": [[-1, 1, "Conv", [32, 6, 2, 2]], [-1, 1, "Conv", [64, 3, 2]], [-1, 3, "C3", [64]], [-1, 1, "SPPF", [64, 5]]],
        "head": [[-1, 1, "Conv", [12, 1, 1]]]}


def make_act(spec):
    """the activation a fixture names: the point-wise strings go through the yaml parser, AconC(c) / FReLU(c) to the constructors"""
    import yolo_dual_amd as ydl
    m = re.match(r"^(AconC|FReLU)\((\d+)\)$", spec)
    return getattr(ydl, m.group(1))(int(m.group(2))) if m else ydl.resolve_activation(spec)


def build(z):
    """the module a fixture describes (weights not loaded)"""
    import yolo_dual_amd as ydl
    # the package's ``C3`` is the seg scripts' block; models/common.py's is ``C3Common``
    cls, args, act = getattr(ydl, {"C3": "C3Common"}.get(str(z["cls"]), str(z["cls"]))), json.loads(str(z["args"])), str(z["act"])
    if str(z["how"]) == "arg":
        return cls(*args, act=make_act(act))
    with ydl.default_activation(act):
        return cls(*args)


def test_the_fixtures_are_present_small_and_carry_the_floors():
    assert [os.path.basename(f)[:-4] for f in FILES] == NAMES
    assert all(os.path.getsize(f) < (1 << 20) for f in FILES)
    for f in FILES:
        z = np.load(f)
        assert str(z["how"]) in ("arg", "default") and str(z["cls"]) in ("Conv", "DWConv", "C3")
        for kind in ("out", "grad", "run"):
            v = float(z["floor." + kind])
            assert 2.0 ** -10 < v < 0.5, (f, kind, v)


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_state_dict_matches_the_reference_modules(path):
    check_state_dict_layout(path, build)


def test_activation_classes_have_the_reference_surface():
    import torch
    import yolo_dual_amd as ydl
    from yolo_dual_amd import activations as A
    assert sorted(A.__all__) == sorted(["SiLU", "Hardswish", "Mish", "MemoryEfficientMish", "FReLU", "AconC", "MetaAconC"])
    a = ydl.AconC(12)
    assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == {"p1": (1, 12, 1, 1), "p2": (1, 12, 1, 1), "beta": (1, 12, 1, 1)}
    assert bool((a.beta == 1).all()) and float(a.p1.detach().std()) > 0.3 and float(a.p2.detach().std()) > 0.3
    f = ydl.FReLU(12)
    assert [k for k in f.state_dict()] == ["conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"]
    assert f.conv.weight.shape == (12, 1, 3, 3) and f.conv.groups == 12 and f.conv.padding == (1, 1) and f.conv.bias is None
    m = ydl.MetaAconC(64)
    assert [k for k in m.state_dict()] == ["p1", "p2", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    assert m.fc1.weight.shape == (16, 64, 1, 1) and m.fc2.weight.shape == (64, 16, 1, 1)
    x = torch.linspace(-4, 4, 33)
    assert torch.allclose(ydl.Mish()(x), torch.nn.Mish()(x)) and torch.allclose(ydl.Hardswish()(x), torch.nn.Hardswish()(x))
    assert torch.allclose(ydl.MemoryEfficientMish()(x), torch.nn.Mish()(x)) and torch.allclose(ydl.SiLU()(x), torch.nn.SiLU()(x))
    c = ydl.Conv(16, 24, 3, 1, act=ydl.AconC(24))
    assert [k for k in c.state_dict() if k.startswith("act.")] == ["act.p1", "act.p2", "act.beta"]
    c = ydl.Conv(16, 24, 3, 1, act=ydl.FReLU(24))
    assert [k for k in c.state_dict() if k.startswith("act.")] == ["act.conv.weight", "act.bn.weight", "act.bn.bias", "act.bn.running_mean",
                                                                   "act.bn.running_var", "act.bn.num_batches_tracked"]


def test_act_code_accepts_every_form():
    import torch.nn as nn
    import yolo_dual_amd as ydl
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.modules import _act_code
    assert (L.ACT_NONE, L.ACT_SILU, L.ACT_RELU, L.ACT_LEAKY, L.ACT_HSWISH, L.ACT_MISH) == (0, 1, 2, 3, 4, 5)
    for act, code in ((True, 1), (nn.SiLU(), 1), (ydl.SiLU(), 1), (False, 0), (None, 0), (nn.Identity(), 0), (nn.ReLU(), 2),
                      (nn.Hardswish(), 4), (ydl.Hardswish(), 4), (nn.Mish(), 5), (ydl.Mish(), 5), (ydl.MemoryEfficientMish(), 5),
                      (ydl.AconC(8), L.ACT_ACON), (ydl.FReLU(8), L.ACT_FRELU)):
        assert _act_code(act) == code and not hasattr(_act_code(act), "param"), act
    for slope in (0.0, 0.01, 0.1, 0.99):
        c = _act_code(nn.LeakyReLU(slope))
        assert c == L.ACT_LEAKY and isinstance(c, int) and c.param == pytest.approx(slope) and c in (L.ACT_LEAKY,) and c not in (0, 1)
    assert L.act_key(_act_code(nn.LeakyReLU(0.1))) != L.act_key(_act_code(nn.LeakyReLU(0.2)))

    class Named(nn.Module):             # matched on type, not on the name
        pass
    Named.__name__ = "SiLU"
    for bad, word in ((nn.LeakyReLU(1.5), "LeakyReLU"), (nn.LeakyReLU(-0.1), "LeakyReLU"), (nn.LeakyReLU(1.0), "LeakyReLU"),
                      (ydl.MetaAconC(16), "MetaAconC"), (nn.GELU(), "GELU"), (nn.Tanh(), "SiLU/ReLU/Identity"), (Named(), "not supported")):
        with pytest.raises(NotImplementedError, match=word):
            _act_code(bad)
    with pytest.raises(NotImplementedError, match="FReLU"):
        ydl.FReLU(16, 5)
    with pytest.raises(NotImplementedError, match="MetaAconC"):
        ydl.Conv(16, 16, 1, 1, act=ydl.MetaAconC(16))
    # sibling 1x1 convolutions of a CSP block fuse only when code AND parameter agree
    assert ydl.Conv(8, 8, act=nn.LeakyReLU(0.1)).act_code.param == pytest.approx(0.1)


def _conv_acts(model):
    import yolo_dual_amd as ydl
    return [m.act for m in model.modules() if isinstance(m, ydl.Conv)]


def test_yaml_activation_key_sets_every_conv_and_is_restored():
    import torch.nn as nn
    import yolo_dual_amd as ydl
    m = ydl.SegYoloModel(YAML)
    acts = _conv_acts(m)
    inner = _conv_acts(m.model[2]) + _conv_acts(m.model[3])
    assert len(acts) == 10 and len(inner) == 7                     # stem, down-sampler, C3 (cv1-3 + 2 in the Bottleneck), SPPF (2), head
    assert all(isinstance(a, nn.LeakyReLU) and a.negative_slope == pytest.approx(0.1) for a in acts), acts
    assert all(c.act_code == 3 and c.act_code.param == pytest.approx(0.1) for c in m.modules() if isinstance(c, ydl.Conv))
    assert isinstance(ydl.Conv.default_act, nn.SiLU)                # restored: a deliberate deviation from the reference
    plain = dict(YAML)
    del plain["activation"]
    assert all(isinstance(a, nn.SiLU) for a in _conv_acts(ydl.SegYoloModel(plain)))
    assert isinstance(ydl.Conv(8, 8).act, nn.SiLU) and ydl.Conv(8, 8).act_code == 1
    with pytest.raises(RuntimeError, match="boom"):
        with ydl.default_activation("nn.Mish()"):
            assert isinstance(ydl.Conv(8, 8).act, nn.Mish) and isinstance(ydl.DWConv(8, 8, 3).act, nn.Mish)
            assert isinstance(ydl.Conv(8, 8, act=nn.ReLU()).act, nn.ReLU) and isinstance(ydl.SimConv(8, 8, 3, 1).act, nn.ReLU)
            raise RuntimeError("boom")
    assert isinstance(ydl.Conv.default_act, nn.SiLU)
    with ydl.default_activation("Hardswish()"):
        d = ydl.DCNv2(8, 8, 3)
        assert isinstance(d.act, ydl.Hardswish) and d.act_code == 4
    assert isinstance(ydl.DCNv2(8, 8, 3).act, nn.SiLU)


def test_string_activation_in_a_row_is_resolved():
    import torch.nn as nn
    import yolo_dual_amd as ydl
    cfg = {"nc": 4, "backbone": [[-1, 1, "Conv", [16, 3, 2, None, 1, "nn.ReLU()"]], [-1, 1, "Conv", [16, 3, 1, "None", 1, "nn.LeakyReLU(0.2)"]],
                                 [-1, 1, "Conv", [16, 1, 1, None, 1, "Mish()"]]],
           "head": [[-1, 1, "nn.Upsample", [None, 2, "nearest"]], [-1, 1, "Conv", [4, 1, 1]]]}
    m = ydl.SegYoloModel(cfg)
    assert isinstance(m.model[0].act, nn.ReLU) and isinstance(m.model[1].act, nn.LeakyReLU) and m.model[1].act.negative_slope == 0.2
    assert isinstance(m.model[2].act, ydl.Mish) and isinstance(m.model[4].act, nn.SiLU)
    for spec, cls in (("nn.SiLU()", nn.SiLU), ("nn.Identity()", nn.Identity), (" nn.LeakyReLU( 0.1 ) ", nn.LeakyReLU), ("LeakyReLU(0.3)", nn.LeakyReLU),
                      ("MemoryEfficientMish()", ydl.MemoryEfficientMish), ("nn.Hardswish()", nn.Hardswish), ("SiLU()", ydl.SiLU)):
        assert type(ydl.resolve_activation(spec)) is cls, spec


@pytest.mark.parametrize("spec,word", [("os.system('x')", "activation"), ("__import__('os').system('x')", "activation"),
                                       ("nn.LeakyReLU(__import__('os'))", "activation"), ("nn.LeakyReLU(True)", "activation"),
                                       ("nn.SiLU", "activation"), ("nn.GELU()", "activation"), ("nn.LeakyReLU(0.1, 2, 3)", "activation"),
                                       ("AconC(16)", "activation"), ("FReLU(16, 5)", "activation"), (3, "activation"),
                                       ("MetaAconC(16)", "MetaAconC"), ("nn.LeakyReLU(1.5)", "LeakyReLU")])
def test_what_is_not_served_is_refused_by_name(spec, word):
    import yolo_dual_amd as ydl
    with pytest.raises(NotImplementedError, match=word):
        ydl.resolve_activation(spec)
    with pytest.raises(NotImplementedError, match=word):
        ydl.SegYoloModel(dict(YAML, activation=spec))
    import torch.nn as nn
    assert isinstance(ydl.Conv.default_act, nn.SiLU)


def test_entry_points_without_a_parameter_refuse_leaky_on_the_host():
    from yolo_dual_amd import _lib as L
    lib = L.lib()
    assert sorted(L.BN_ACT_ARG) == sorted(["ydl_bn_act_fwd", "ydl_bn_act_fwd_sums", "ydl_bn_act_bwd", "ydl_bn_act_bwd_sums",
                                           "ydl_bn_act_bwd_apply_sums", "ydl_bn_act_bwd_reduce_sums"])
    for name, k in L.BN_ACT_ARG.items():
        argtypes = L.SIGNATURES[name][1]
        assert argtypes[k] is ctypes.c_int and L.SIGNATURES[name + "_p"][1] == argtypes[:k + 1] + [ctypes.c_float] + argtypes[k + 1:]
        args = [None if t is ctypes.c_void_p else 0 for t in argtypes]
        args[k] = L.ACT_LEAKY
        assert getattr(lib, name)(*args) != 0                       # refused before any argument is looked at: nothing is launched
        msg = lib.ydl_last_error().decode()
        assert "YDL_ACT_LEAKY" in msg and name + "_p" in msg, msg


def test_call_act_routes_only_parametrised_codes_to_the_siblings(monkeypatch):
    from yolo_dual_amd import _lib as L
    seen = []
    monkeypatch.setattr(L, "call", lambda name, *a: seen.append((name, a)))
    args = list(range(14))
    args[8] = L.ACT_SILU
    L.call_act("ydl_bn_act_fwd", *args)
    args[8] = L.ActCode(L.ACT_LEAKY, 0.25)
    L.call_act("ydl_bn_act_fwd", *args)
    assert seen[0] == ("ydl_bn_act_fwd", tuple(range(8)) + (1,) + tuple(range(9, 14)))
    assert seen[1] == ("ydl_bn_act_fwd_p", tuple(range(8)) + (3, 0.25) + tuple(range(9, 14)))
    assert type(seen[1][1][8]) is int


def test_replay_table_is_current_and_has_the_new_entry_points():
    spec = importlib.util.spec_from_file_location("gen_replay", os.path.join(ROOT, "tools", "gen_replay.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    table = open(os.path.join(ROOT, "yolo_dual_amd", "csrc", "replay_table.inc")).read()
    assert table == gen.generate()
    names = re.findall(r'^    "(ydl_\w+)",$', table, flags=re.M)
    new = ["ydl_bn_act_fwd_p", "ydl_bn_act_bwd_p", "ydl_bn_act_fwd_sums_p", "ydl_bn_act_bwd_sums_p", "ydl_bn_act_bwd_apply_sums_p",
           "ydl_bn_act_bwd_reduce_sums_p", "ydl_acon_fwd", "ydl_acon_bwd", "ydl_max2_fwd", "ydl_max2_bwd"]
    assert names[-len(new):] == new                                  # appended: the earlier rows keep their indices
    assert names.index("ydl_bn_act_fwd") < names.index("ydl_bn_act_bwd") < names.index("ydl_bn_act_fwd_p")
