"""CPU: the Ghost family (models/common.py:67-70 DWConv, :199-204 C3Ghost, :253-279 GhostConv / GhostBottleneck) has the reference's
constructor signatures and state_dict layout (key lists and shapes recorded from the reference's own classes by
tools/make_ghost_golden.py), ``parse_model`` resolves the four rows (models/yolo.py:317-329: width gain on c2, ``n`` inserted for
C3Ghost only), the constructors refuse what the HIP path does not implement, and ``smart_optimizer`` groups the new parameters as the
reference's does (utils/torch_utils.py:318-333)."""
import glob
import os

import pytest

from tests.block_harness import check_state_dict_layout

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "ghost_*.npz")))
# 3 x 32 x 32 input -> 16 ch @ 16^2 -> GhostConv 32 ch @ 8^2 -> C3Ghost (half widths 8 and 4: both GhostConv paths) -> stride-2
# GhostBottleneck 64 ch @ 4^2 -> DWConv -> 12 classes
YAML = {"nc": 12, "width_multiple": 0.5, "depth_multiple": 0.33,
        "backbone": [[-1, 1, "Conv", [32, 6, 2, 2]], [-1, 1, "GhostConv", [64, 3, 2]], [-1, 3, "C3Ghost", [64]],
                     [-1, 1, "GhostBottleneck", [128, 3, 2]], [-1, 1, "DWConv", [128, 3, 1]]],
        "head": [[-1, 1, "Conv", [12, 1, 1]]]}


def build(z):
    """the module a fixture describes (weights not loaded)"""
    import yolo_dual_amd as ydl
    cls, args = str(z["cls"]), [int(v) for v in z["args"]]
    kw = {} if int(z["act"]) else {"act": False}
    return getattr(ydl, cls)(*args, **kw)


def test_the_six_fixtures_are_present():
    assert len(FILES) == 6 and all(os.path.getsize(f) < 100000 for f in FILES)


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_state_dict_matches_the_reference_modules(path):
    _z, _mod, want = check_state_dict_layout(path, build)
    dw = [k for k, s in want if k.endswith("conv.weight") and len(s) == 4 and s[1] == 1 and s[0] > 1]
    assert dw, "every Ghost fixture holds at least one depth-wise weight [C,1,k,k]"


def test_shortcut_keys_only_at_stride_two():
    import yolo_dual_amd as ydl
    k1 = list(ydl.GhostBottleneck(16, 16, 3, 1).state_dict())
    k2 = list(ydl.GhostBottleneck(16, 32, 3, 2).state_dict())
    assert not any(k.startswith("shortcut") or k.startswith("conv.1.") for k in k1)
    assert "shortcut.0.conv.weight" in k2 and "shortcut.1.bn.running_var" in k2 and "conv.1.conv.weight" in k2
    assert "conv.0.cv1.conv.weight" in k1 and "conv.2.cv2.bn.weight" in k1


def test_parse_model_builds_the_ghost_rows():
    import torch.nn as nn
    import yolo_dual_amd as ydl
    seq, save = ydl.parse_model(YAML, [3])
    gc, c3, gb, dw = seq[1], seq[2], seq[3], seq[4]
    assert [type(m) for m in (gc, c3, gb, dw)] == [ydl.GhostConv, ydl.C3Ghost, ydl.GhostBottleneck, ydl.DWConv]
    # width gain 0.5 on every c2 but the class count; c1 from the previous row
    assert gc.cv1.conv.weight.shape == (16, 16, 3, 3) and gc.cv1.conv.stride == (2, 2) and gc.cv2.conv.weight.shape == (16, 1, 5, 5)
    assert c3.cv1.conv.weight.shape == (16, 32, 1, 1) and c3.cv3.conv.weight.shape == (32, 32, 1, 1)
    # n inserted for C3Ghost only: 3 x 0.33 -> one GhostBottleneck(16, 16) inside, no Sequential of C3Ghosts
    assert len(c3.m) == 1 and type(c3.m[0]) is ydl.GhostBottleneck and c3.m[0].conv[0].cv1.conv.weight.shape == (4, 16, 1, 1)
    assert gb.s == 2 and gb.shortcut[0].conv.weight.shape == (32, 1, 3, 3) and gb.shortcut[0].conv.stride == (2, 2)
    assert gb.shortcut[1].conv.weight.shape == (64, 32, 1, 1) and gb.conv[1].conv.weight.shape == (32, 1, 3, 3)
    assert dw.conv.weight.shape == (64, 1, 3, 3) and dw.conv.groups == 64
    assert seq[5].conv.weight.shape == (12, 64, 1, 1)
    assert [m.type for m in (gc, c3, gb, dw)] == ["models.common." + n for n in ("GhostConv", "C3Ghost", "GhostBottleneck", "DWConv")]
    seq, _ = ydl.parse_model(dict(YAML, depth_multiple=1.0), [3])
    assert type(seq[2]) is ydl.C3Ghost and len(seq[2].m) == 3 and not isinstance(seq[3], nn.Sequential)


def test_what_the_hip_path_does_not_implement_is_refused():
    import yolo_dual_amd as ydl
    with pytest.raises(NotImplementedError, match="c2=16"):
        ydl.DWConv(8, 16, 3, 1)                      # g = gcd = 8 = c1 but c2 differs: a grouped, not a depth-wise, convolution
    with pytest.raises(NotImplementedError, match="c1=12"):
        ydl.DWConv(12, 8, 3, 1)
    with pytest.raises(NotImplementedError, match="d=2"):
        ydl.DWConv(8, 8, 3, 1, 2)
    with pytest.raises(NotImplementedError, match="g=2"):
        ydl.GhostConv(8, 16, 1, 1, 2)
    with pytest.raises(NotImplementedError, match="s=3"):
        ydl.Conv(8, 8, 3, 3, None, 8)                # depth-wise: stride 1 or 2
    with pytest.raises(NotImplementedError, match="groups"):
        ydl.Conv(8, 16, 3, 1, None, 4)               # 1 < g < C stays refused
    with pytest.raises(NotImplementedError):
        ydl.Conv(8, 8, 3, 1, None, 8, 2)             # dilation
    assert ydl.Conv(8, 8, 3, 2, None, 8).depthwise and ydl.DWConv(8, 8, 5, 2).conv.stride == (2, 2)


def test_smart_optimizer_groups():
    import torch.nn as nn
    import yolo_dual_amd as ydl
    net = ydl.SegYoloModel(YAML)
    opt = ydl.smart_optimizer(net, "SGD", lr=0.01, momentum=0.9, decay=5e-4)
    bias, decay, bn = ({id(p) for p in g["params"]} for g in opt.param_groups)
    assert opt.param_groups[1]["weight_decay"] == 5e-4 and opt.param_groups[2]["weight_decay"] == 0.0
    n = 0
    for name, mod in net.named_modules():
        if isinstance(mod, nn.Conv2d):
            assert id(mod.weight) in decay and id(mod.weight) not in bn and id(mod.weight) not in bias, name
            n += 1
        elif isinstance(mod, nn.BatchNorm2d):
            assert id(mod.weight) in bn and id(mod.bias) in bias and id(mod.weight) not in decay, name
    assert n == len([k for k in net.state_dict() if k.endswith("conv.weight")]) and n == 19
    dw = net.model[4].conv.weight
    assert dw.shape == (64, 1, 3, 3) and dw.grad.shape == dw.shape
