"""CPU: the dilated family (models/common.py:47-64 Conv with d > 1, :1336-1361 ASPP, :1366-1384 BasicConv, :1386-1425 RFB) has the
reference's constructor signatures and state_dict layout (key lists and shapes recorded from the reference's own classes by
tools/make_dilated_golden.py), ``parse_model`` resolves the ASPP and RFB rows (models/yolo.py:317-326: width gain on c2), and the
constructors refuse what the HIP path does not implement."""
import glob
import os

import pytest

from tests.block_harness import build_from_json as build, check_state_dict_layout

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "dil_*.npz")))
# 3 x 32 x 32 input -> 16 ch @ 16^2 -> 32 ch @ 8^2 -> RFB 64 ch (inter-plane widths 4, 6 and 8) -> dilated Conv 32 ch -> ASPP 32 ch
# (branches written into the concat buffer) -> ASPP 12 classes (12-channel branches: the copy path).  The ASPP rows come last: a
# bias in front of a train-mode BatchNorm has an exactly zero gradient, and the GPU test wants every parameter moved.
YAML = {"nc": 12, "width_multiple": 0.5, "depth_multiple": 0.33,
        "backbone": [[-1, 1, "Conv", [32, 6, 2, 2]], [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "RFB", [128]],
                     [-1, 1, "Conv", [64, 3, 1, "None", 1, 2]], [-1, 1, "ASPP", [64]]],
        "head": [[-1, 1, "ASPP", [12]]]}


def test_the_four_fixtures_are_present():
    assert [os.path.basename(f) for f in FILES] == ["dil_aspp_16_8.npz", "dil_basic_12_16_d3.npz", "dil_conv_16_24_d2.npz",
                                                    "dil_rfb_64_32.npz"]


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_state_dict_matches_the_reference_modules(path):
    import torch
    _z, mod, _want = check_state_dict_layout(path, build)
    dil = [m for m in mod.modules() if isinstance(m, torch.nn.Conv2d) and m.dilation[0] > 1]
    assert dil and all(m.padding == m.dilation and m.weight.shape[2:] == (3, 3) for m in dil)
    for m in dil:                                   # KRSC master: the weight of the 1x1 GEMM over the column buffer as it is
        assert m.weight.detach().permute(0, 2, 3, 1).is_contiguous()


def test_both_constructor_forms_of_a_dilated_conv():
    import torch.nn as nn
    import yolo_dual_amd as ydl
    for c in (ydl.Conv(16, 24, 3, 1, None, 1, 2), ydl.Conv(16, 24, 3, 1, None, 1, 2, True), ydl.Conv(16, 24, 3, 1, 2, 1, 2, nn.ReLU())):
        assert c.d == 2 and c.conv.dilation == (2, 2) and c.conv.padding == (2, 2) and c.conv.weight.shape == (24, 16, 3, 3)
    assert isinstance(ydl.Conv(16, 24, 3, 1, None, 1, 2, False).act, nn.Identity)
    assert ydl.Conv(16, 24, 3, 1, None, 1, True).d == 1             # seven-argument seg-script form: the 7th is ``act``
    bc = ydl.BasicConv(12, 16, 3, padding=3, dilation=3, relu=False)
    assert (bc.bn.eps, bc.bn.momentum, bc.relu) == (1e-5, 0.01, None) and bc.d == 3
    assert isinstance(ydl.BasicConv(8, 8, (3, 3), padding=(1, 1)).relu, nn.ReLU)
    nb = ydl.BasicConv(12, 16, 3, padding=3, dilation=3, relu=False, bn=False)
    assert list(nb.state_dict()) == ["conv.weight", "conv.bias"] and nb.bn is None and nb.conv.dilation == (3, 3)


def test_parse_model_builds_the_aspp_and_rfb_rows():
    import yolo_dual_amd as ydl
    net = ydl.SegYoloModel(YAML)
    rfb, dc, aspp, last = net.model[2], net.model[3], net.model[4], net.model[5]
    assert [type(m) for m in (aspp, rfb, dc, last)] == [ydl.ASPP, ydl.RFB, ydl.Conv, ydl.ASPP]
    # width gain 0.5 on c2 (not on the class count); c1 from the previous row
    assert last.atrous_block18.weight.shape == (12, 32, 3, 3) and last.conv_1x1_output.weight.shape == (12, 60, 1, 1)
    assert aspp.atrous_block1.weight.shape == (32, 32, 1, 1) and aspp.conv_1x1_output.weight.shape == (32, 160, 1, 1)
    assert [(m.weight.shape, m.dilation, m.padding) for m in (aspp.atrous_block6, aspp.atrous_block12, aspp.atrous_block18)] == \
        [((32, 32, 3, 3), (d, d), (d, d)) for d in (6, 12, 18)]
    assert rfb.inter_planes == 4 and rfb.ConvLinear.conv.weight.shape == (64, 24, 1, 1) and rfb.shortcut.conv.weight.shape == (64, 32, 1, 1)
    assert [br[-1].conv.dilation for br in (rfb.branch0, rfb.branch1, rfb.branch2)] == [(2, 2), (3, 3), (5, 5)]
    assert rfb.branch2[1].conv.weight.shape == (6, 4, 3, 3) and rfb.branch2[2].conv.weight.shape == (8, 6, 3, 3)
    assert dc.conv.weight.shape == (32, 64, 3, 3) and dc.conv.dilation == (2, 2)
    assert [m.type for m in (aspp, rfb)] == ["models.common.ASPP", "models.common.RFB"]


def test_what_the_hip_path_does_not_implement_is_refused():
    import yolo_dual_amd as ydl
    for args in ((8, 8, 3, 2, None, 1, 2), (8, 8, 5, 1, None, 1, 2), (8, 8, 3, 1, 1, 1, 2), (8, 8, 1, 1, None, 1, 3)):
        with pytest.raises(NotImplementedError, match="g=1, s=1, k=3"):      # the message names the supported set
            ydl.Conv(*args)
    with pytest.raises(NotImplementedError):
        ydl.Conv(8, 8, 3, 1, None, 8, 2)                 # dilated depth-wise
    with pytest.raises(NotImplementedError, match="groups"):
        ydl.Conv(8, 16, 3, 1, None, 4, 2)
    with pytest.raises(NotImplementedError, match="fuse"):
        ydl.Conv(8, 8, 3, 1, None, 1, 2).fuse()          # never an undilated convolution in its place
    with pytest.raises(NotImplementedError, match="stride"):
        ydl.RFB(64, 32, stride=2)
    with pytest.raises(NotImplementedError, match="groups"):
        ydl.RFB(64, 32, groups=2)
    with pytest.raises(NotImplementedError, match="groups"):
        ydl.BasicConv(8, 8, 3, padding=1, groups=2)
    with pytest.raises(NotImplementedError, match="g=1, s=1, k=3"):
        ydl.BasicConv(8, 8, 3, stride=2, padding=2, dilation=2)
    assert ydl.RFB(64, 32, vision=2, map_reduce=4).branch2[-1].conv.dilation == (6, 6)
