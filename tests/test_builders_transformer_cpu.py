"""CPU: ``parse_model`` resolves C3TR (models/yolo.py:319,327: ``n`` inserted as for C3) and TransformerBlock with the reference's
module tree, parameter names and shapes; head dimensions the HIP attention kernels do not serve are refused; ``smart_optimizer``
groups the new parameters the way the reference's loop does (utils/torch_utils.py:322-329: a parameter NAMED ``bias`` -> no decay,
BatchNorm ``weight`` -> no decay, everything else -> decay, so ``ma.in_proj_bias`` decays)."""
import glob
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "tr_*.npz")))
YAML = {"nc": 12, "width_multiple": 0.25, "depth_multiple": 0.33,
        "backbone": [[-1, 1, "Conv", [64, 6, 2, 2]], [-1, 3, "C3TR", [512]]],
        "head": [[-1, 1, "Conv", [12, 1, 1]]]}
LAYER_KEYS = ["q.weight", "k.weight", "v.weight", "ma.in_proj_weight", "ma.in_proj_bias", "ma.out_proj.weight", "ma.out_proj.bias",
              "fc1.weight", "fc2.weight"]


def test_parse_model_builds_the_c3tr_row():
    import yolo_dual_amd as ydl
    seq, _save = ydl.parse_model(YAML, [3])
    blk = seq[1]
    assert type(blk) is ydl.C3TR and blk.type == "models.common.C3TR"
    assert type(blk.m) is ydl.TransformerBlock and len(blk.m.tr) == 1 and blk.m.conv is None      # n = 3 -> max(round(3 * 0.33), 1)
    assert (blk.cv1.conv.weight.shape, blk.cv3.conv.weight.shape) == ((64, 16, 1, 1), (128, 128, 1, 1))
    assert list(blk.m.state_dict().keys()) == ["linear.weight", "linear.bias"] + ["tr.0." + k for k in LAYER_KEYS]
    sd = blk.m.state_dict()
    assert tuple(sd["tr.0.ma.in_proj_weight"].shape) == (192, 64) and tuple(sd["tr.0.ma.in_proj_bias"].shape) == (192,)
    assert blk.m.tr[0].num_heads == 4
    deep, _ = ydl.parse_model(dict(YAML, depth_multiple=1.0), [3])
    assert type(deep[1]) is ydl.C3TR and len(deep[1].m.tr) == 3


def test_parse_model_takes_a_transformer_block_row_as_written():
    import yolo_dual_amd as ydl
    y = dict(YAML, backbone=[[-1, 1, "Conv", [64, 6, 2, 2]], [-1, 1, "TransformerBlock", [16, 16, 2, 2]]], head=[[-1, 1, "Conv", [12, 1, 1]]])
    seq, _ = ydl.parse_model(y, [3])
    assert type(seq[1]) is ydl.TransformerBlock and len(seq[1].tr) == 2 and seq[2].conv.weight.shape == (12, 16, 1, 1)


def _module(z):
    import yolo_dual_amd as ydl
    return getattr(ydl, str(z["cls"]))(*(int(a) for a in z["args"]))


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_state_dict_matches_the_reference_modules(path):
    import torch
    z = np.load(path)
    mod = _module(z)
    want = [(str(k), tuple(z["p." + str(k)].shape)) for k in z["keys"]]
    assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == want
    mod.load_state_dict({k: torch.from_numpy(z["p." + k]) for k, _ in want})


def test_there_are_four_fixtures():
    assert len(FILES) == 4


def test_initialisation_follows_nn_multihead_attention():
    import torch
    import yolo_dual_amd as ydl
    torch.manual_seed(0)
    layer = ydl.TransformerLayer(64, 4)
    ma = layer.ma
    assert float(ma.in_proj_bias.detach().abs().max()) == 0.0 and float(ma.out_proj.bias.detach().abs().max()) == 0.0
    bound = (6.0 / (192 + 64)) ** 0.5                    # xavier_uniform_ on [3c, c]
    w = ma.in_proj_weight.detach()
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.95 * bound
    assert float(layer.q.weight.detach().abs().max()) <= 1 / 8 + 1e-6          # nn.Linear's default: U(-1/sqrt(in), 1/sqrt(in))
    # the yaml models' kaiming pass leaves all of it alone
    net = ydl.SegYoloModel(YAML)
    t = net.model[1].m.tr[0]
    assert float(t.ma.in_proj_weight.detach().abs().max()) <= (6.0 / (192 + 64)) ** 0.5 and float(t.ma.in_proj_bias.detach().abs().max()) == 0.0


@pytest.mark.parametrize("c,heads", [(16, 4), (544, 4), (48, 4)])
def test_head_dimensions_the_kernels_do_not_serve_are_refused(c, heads):
    import yolo_dual_amd as ydl
    with pytest.raises(NotImplementedError, match="multiples of 8 between 8 and 128"):      # d = 4, 136, 12
        ydl.TransformerLayer(c, heads)
    with pytest.raises(NotImplementedError, match="multiples of 8 between 8 and 128"):
        ydl.TransformerBlock(c, c, heads, 1)
    if heads == 4 and c != 48:
        with pytest.raises(NotImplementedError, match="multiples of 8 between 8 and 128"):
            ydl.C3TR(2 * c, 2 * c, 1)


def test_smart_optimizer_groups():
    import yolo_dual_amd as ydl
    net = ydl.SegYoloModel(YAML)
    opt = ydl.smart_optimizer(net, "SGD", lr=0.01, momentum=0.9, decay=5e-4)
    bias, decay, bn = ({id(p) for p in g["params"]} for g in opt.param_groups)
    assert opt.param_groups[1]["weight_decay"] == 5e-4 and opt.param_groups[2]["weight_decay"] == 0.0
    m = net.model[1].m
    t = m.tr[0]
    for p in (t.ma.in_proj_bias, t.ma.in_proj_weight, t.q.weight, t.k.weight, t.v.weight, t.ma.out_proj.weight, t.fc1.weight,
              t.fc2.weight, m.linear.weight):
        assert id(p) in decay and id(p) not in bias and id(p) not in bn
    for p in (t.ma.out_proj.bias, m.linear.bias):
        assert id(p) in bias and id(p) not in decay
    assert t.ma.in_proj_bias.shape == (192,) and t.ma.in_proj_bias.grad.shape == (192,)
