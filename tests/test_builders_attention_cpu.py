"""CPU: ``parse_model`` resolves AttentionConv / AttentionStem (models/yolo.py:318-329) with the reference's parameter names and
shapes, the constructors refuse what the HIP path does not implement, and ``smart_optimizer`` groups the new parameters the way the
reference's does (utils/torch_utils.py:318-333: ``bias`` -> no decay, BatchNorm ``weight`` -> no decay, everything else -> decay)."""
import glob
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
YAML = {"nc": 12, "width_multiple": 0.25, "depth_multiple": 0.33,
        "backbone": [[-1, 1, "Conv", [64, 6, 2, 2]], [-1, 3, "AttentionConv", [512, 3, 1, 1]]],
        "head": [[-1, 1, "AttentionStem", [256, 3, 1, 1]], [-1, 1, "Conv", [12, 1, 1]]]}


def test_parse_model_builds_the_attention_rows():
    import yolo_dual_amd as ydl
    seq, save = ydl.parse_model(YAML, [3])
    ac, st = seq[1], seq[2]
    assert type(ac) is ydl.AttentionConv and type(st) is ydl.AttentionStem      # the depth gain brings n = 3 down to 1: no Sequential
    assert (ac.in_channels, ac.out_channels, st.in_channels, st.out_channels) == (16, 128, 128, 64)
    assert (ac.kernel_size, ac.stride, ac.padding, st.kernel_size, st.stride, st.padding, st.m) == (3, 1, 1, 3, 1, 1, 4)
    assert ac.type == "models.common.AttentionConv" and st.type == "models.common.AttentionStem"
    assert seq[3].conv.weight.shape == (12, 64, 1, 1)
    assert {k: tuple(v.shape) for k, v in ac.state_dict().items()} == {
        "rel_h": (64, 1, 1, 3, 1), "rel_w": (64, 1, 1, 1, 3), "key_conv.weight": (128, 16, 1, 1), "query_conv.weight": (128, 16, 1, 1),
        "value_conv.weight": (128, 16, 1, 1)}


def test_depth_above_one_is_a_sequential_of_identical_layers():
    import torch.nn as nn
    import yolo_dual_amd as ydl
    seq, _ = ydl.parse_model(dict(YAML, depth_multiple=1.0), [3])
    assert isinstance(seq[1], nn.Sequential) and len(seq[1]) == 3
    # models/yolo.py:369 builds every copy with the same (c1, c2, ...): only c1 == c2 would chain, and 16 != 128 — as in the reference
    assert all(type(b) is ydl.AttentionConv and (b.in_channels, b.out_channels) == (16, 128) for b in seq[1])
    assert seq[1].type == "models.common.AttentionConv"


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "attn_*.npz"))), ids=lambda p: os.path.basename(p)[:-4])
def test_state_dict_matches_the_reference_modules(path):
    import yolo_dual_amd as ydl
    z = np.load(path)
    c1, c2, ks, s, p, g, m = (int(v) for v in z["args"])
    mod = ydl.AttentionStem(c1, c2, ks, s, p, g, m) if m else ydl.AttentionConv(c1, c2, ks, s, p, g)
    want = [(str(k), tuple(z["p." + str(k)].shape)) for k in z["keys"]]
    assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == want
    mod.load_state_dict({k: __import__("torch").from_numpy(z["p." + k]).float() for k, _ in want})


def test_what_the_hip_path_does_not_implement_is_refused():
    import yolo_dual_amd as ydl
    for cls in (ydl.AttentionConv, ydl.AttentionStem):
        with pytest.raises(NotImplementedError, match="stride"):
            cls(8, 16, 3, 2, 1)
        with pytest.raises(NotImplementedError, match="padding"):
            cls(8, 16, 3, 1, 0)
        with pytest.raises(NotImplementedError, match="kernel_size"):
            cls(8, 16, 4, 1, 1)
        with pytest.raises(NotImplementedError, match="kernel_size"):
            cls(8, 16, 9, 1, 4)
        with pytest.raises(NotImplementedError, match="bias"):
            cls(8, 16, 3, 1, 1, bias=True)
    with pytest.raises(NotImplementedError, match="padding"):
        ydl.AttentionStem(8, 16, 3)                 # the reference's own default padding=0 cannot run its forward
    with pytest.raises(NotImplementedError, match="odd out_channels"):
        ydl.AttentionConv(8, 15, 3, 1, 1)
    ydl.AttentionStem(8, 15, 3, 1, 1)               # no channel halves in the Stem


def test_reset_parameters_follows_the_reference():
    import torch
    import yolo_dual_amd as ydl
    torch.manual_seed(0)
    m = ydl.AttentionStem(64, 256, 3, 1, 1)
    # kaiming_normal_(fan_out, relu) on [256, 64, 1, 1]: std = sqrt(2 / 256); N(0, 1) on the embeddings
    for w in [m.key_conv.weight, m.query_conv.weight] + [v.weight for v in m.value_conv]:
        assert abs(float(w.detach().std()) / (2 / 256) ** 0.5 - 1) < 0.05
    assert abs(float(m.emb_a.detach().std()) - 1) < 0.15 and abs(float(m.emb_mix.detach().std()) - 1) < 0.15
    # the yaml models' kaiming pass (leaky_relu gain) leaves the layer's own initialisation alone
    net = ydl.SegYoloModel(YAML)
    assert abs(float(net.model[1].key_conv.weight.detach().std()) / (2 / 128) ** 0.5 - 1) < 0.08


def test_smart_optimizer_groups():
    import yolo_dual_amd as ydl
    net = ydl.SegYoloModel(YAML)
    opt = ydl.smart_optimizer(net, "SGD", lr=0.01, momentum=0.9, decay=5e-4)
    bias, decay, bn = ({id(p) for p in g["params"]} for g in opt.param_groups)
    assert opt.param_groups[1]["weight_decay"] == 5e-4 and opt.param_groups[2]["weight_decay"] == 0.0
    ac, st = net.model[1], net.model[2]
    new = [ac.rel_h, ac.rel_w, ac.key_conv.weight, ac.query_conv.weight, ac.value_conv.weight, st.emb_a, st.emb_b, st.emb_mix,
           st.key_conv.weight, st.query_conv.weight] + [v.weight for v in st.value_conv]
    assert all(id(p) in decay and id(p) not in bias and id(p) not in bn for p in new)
    assert id(net.model[0].bn.weight) in bn and id(net.model[0].bn.bias) in bias
    # the arena views keep every new parameter's shape and values
    assert ac.rel_h.shape == (64, 1, 1, 3, 1) and st.emb_mix.shape == (4, 64) and ac.rel_h.grad.shape == ac.rel_h.shape
