"""CPU: grouped convolution with 1 < groups < channels.  ``Conv(g > 1)`` is a served case under one rule (c1/g and c2/g multiples of
16, k in {1, 3}, s = 1, p = k // 2, d = 1) and ``SPPCSPC_group`` (models/common.py:1451-1468) has the reference's constructor signature
and state_dict layout (key lists and shapes recorded from the reference's own classes by tools/make_gconv_golden.py); ``parse_model``
resolves the row, Bottleneck / C3 hand their ``g`` through, everything outside the rule is refused by name, and the library's host-side
query ``ydl_gconv_supported`` draws the same line as the constructor."""
import ctypes
import glob
import os

import numpy as np
import pytest

from tests.block_harness import build_from_json as build, check_state_dict_layout

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "gconv_*.npz")))
# 3 x 32 x 32 input -> 16 ch @ 16^2 -> 64 ch @ 8^2 -> SPPCSPC_group (64 -> 64: 16 channels per group, cv5 64 -> 16) -> C3 whose Bottleneck
# has a 3x3 with g = 2 (32 -> 32) -> 12 classes
YAML = {"nc": 12, "width_multiple": 0.5, "depth_multiple": 0.33,
        "backbone": [[-1, 1, "Conv", [32, 6, 2, 2]], [-1, 1, "Conv", [128, 3, 2]], [-1, 1, "SPPCSPC_group", [128]],
                     [-1, 1, "C3", [128, True, 2]]],
        "head": [[-1, 1, "Conv", [12, 1, 1]]]}

# (c1, c2, k, s, p, g) -> served
CASES = [((32, 96, 3, 1, None, 2), True), ((64, 64, 1, 1, None, 4), True), ((256, 64, 1, 1, None, 4), True),
         ((32, 32, 3, 2, None, 2), False), ((32, 32, 5, 1, None, 2), False), ((24, 24, 3, 1, None, 2), False),
         ((8, 16, 3, 1, None, 4), False), ((32, 32, 3, 1, 0, 2), False)]


def test_the_two_fixtures_are_present_and_small():
    assert [os.path.basename(f) for f in FILES] == ["gconv_conv_32_96_g2_k3.npz", "gconv_sppcspc_group_64_64.npz"]
    assert all(os.path.getsize(f) < (1 << 20) for f in FILES)
    assert [str(np.load(f)["cls"]) for f in FILES] == ["Conv", "SPPCSPC_group"]


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_state_dict_matches_the_reference_modules(path):
    check_state_dict_layout(path, build)


def test_constructor_forms():
    import torch.nn as nn
    import yolo_dual_amd as ydl
    m = ydl.SPPCSPC_group(64, 64)
    assert m.k == (5, 9, 13) and m.c_ == 64
    assert all(c.conv.groups == 4 and c.grouped and not c.depthwise and isinstance(c.act, nn.SiLU)
               for c in (m.cv1, m.cv2, m.cv3, m.cv4, m.cv5, m.cv6, m.cv7))
    assert m.cv5.conv.weight.shape == (64, 64, 1, 1) and m.cv3.conv.weight.shape == (64, 16, 3, 3) and m.cv7.conv.weight.shape == (64, 32, 1, 1)
    assert sum(p.numel() for p in m.parameters()) == 28544
    # n, shortcut and g are accepted and unused, as in the reference: the convolutions keep g = 4
    assert ydl.SPPCSPC_group(64, 64, 3, True, 2, 0.5, (3, 7, 15)).cv1.conv.groups == 4
    c = ydl.Conv(32, 96, 3, 1, None, 2)
    assert c.conv.groups == 2 and c.grouped and c.conv.weight.shape == (96, 16, 3, 3) and c.conv.padding == (1, 1)
    assert c.conv.weight.permute(0, 2, 3, 1).is_contiguous()            # KRSC master [c2][k*k][c1/g]
    # groups = 1 and depth-wise are what they were
    assert not ydl.Conv(32, 32, 3).grouped and ydl.Conv(32, 32, 3, 1, None, 32).depthwise and not ydl.Conv(32, 32, 3, 1, None, 32).grouped
    # the blocks that hand g to a Conv
    assert ydl.Bottleneck(32, 32, True, 2, 1.0).cv2.conv.groups == 2
    assert ydl.C2f(64, 64, 1, False, 2).m[0].conv.weight.shape == (32, 16, 3, 3)


def test_parse_model_builds_the_grouped_rows():
    import yolo_dual_amd as ydl
    net = ydl.SegYoloModel(YAML)
    grp, c3, last = net.model[2], net.model[3], net.model[4]
    assert [type(m) for m in (grp, c3, last)] == [ydl.SPPCSPC_group, ydl.C3Common, ydl.Conv]
    assert grp.type == "models.common.SPPCSPC_group"
    # width gain 0.5 on c2, c1 from the previous row, no n inserted
    assert grp.cv1.conv.weight.shape == (64, 16, 1, 1) and grp.cv5.conv.weight.shape == (64, 64, 1, 1)
    assert grp.cv3.conv.weight.shape == (64, 16, 3, 3) and grp.cv7.conv.weight.shape == (64, 32, 1, 1)
    assert len(c3.m) == 1 and c3.m[0].cv2.conv.weight.shape == (32, 16, 3, 3) and c3.m[0].cv2.conv.groups == 2 and c3.m[0].add
    assert c3.cv1.conv.groups == 1 and last.conv.weight.shape == (12, 64, 1, 1)
    rep = ydl.parse_model({"nc": 12, "backbone": [[-1, 1, "Conv", [64, 3, 2]], [-1, 2, "SPPCSPC_group", [64]]], "head": []}, [3])[0][1]
    assert len(rep) == 2 and all(type(m) is ydl.SPPCSPC_group for m in rep)


def test_what_lies_outside_the_served_set_is_refused():
    import yolo_dual_amd as ydl
    for args in ((32, 32, 3, 2, None, 2), (32, 32, 5, 1, None, 2), (24, 24, 3, 1, None, 2), (32, 32, 3, 1, 0, 2), (32, 32, 3, 1, None, 2, 2)):
        with pytest.raises(NotImplementedError, match="groups"):
            ydl.Conv(*args)
    with pytest.raises(NotImplementedError, match="groups"):
        ydl.SPPCSPC_group(32, 32)                      # 8 channels per group
    with pytest.raises(NotImplementedError, match="grouped"):
        ydl.Conv(32, 96, 3, 1, None, 2).fuse()
    # the model-level fuse() skips grouped Convs the way it skips depth-wise ones
    from yolo_dual_amd.models import _YamlSegModel
    net = ydl.SegYoloModel(YAML)
    _YamlSegModel.fuse(net)                            # the loop of the yaml segmentation models, over this module tree
    assert getattr(net.model[2].cv1, "_fused", None) is None and net.model[4]._fused is not None


def test_the_library_query_agrees_with_the_constructor():
    import yolo_dual_amd as ydl
    from yolo_dual_amd import _lib as L
    for (c1, c2, k, s, p, g), served in CASES:
        try:
            ydl.Conv(c1, c2, k, s, p, g)
            made = True
        except NotImplementedError:
            made = False
        assert made == served, (c1, c2, k, s, p, g)
        pad = k // 2 if p is None else p
        H = W = 12
        Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        for dt in (L.YDL_F32, L.YDL_BF16):
            geom = L.ConvGeom(2, H, W, c1, Ho, Wo, c2, k, s, pad, c1, c2, 0)
            gp = ctypes.byref(geom)
            assert L.lib().ydl_gconv_supported(gp, g, dt) == int(served), (c1, c2, k, s, p, g, dt)
            assert (L.lib().ydl_gconv_fwd_block_m(gp, g, dt) > 0) == served
            assert (L.lib().ydl_gconv_fwd_stats_ws_bytes(gp, g, dt) > 0) == served
            assert (L.lib().ydl_gconv_wgrad_ws_bytes(gp, g, dt) > 0) == served
    geom = L.ConvGeom(2, 12, 12, 64, 12, 12, 64, 3, 1, 1, 64, 64, 0)
    assert L.lib().ydl_gconv_supported(ctypes.byref(geom), 1, L.YDL_BF16) == 0          # groups = 1 is ydl_conv_fwd
    geom.ldw = 640
    assert L.lib().ydl_gconv_supported(ctypes.byref(geom), 4, L.YDL_BF16) == 0
    # a launch outside the served set is an error with a message, on the host, before anything is enqueued
    geom = L.ConvGeom(2, 12, 12, 24, 12, 12, 24, 3, 1, 1, 24, 24, 0)
    assert L.lib().ydl_gconv_fwd(ctypes.byref(geom), 2, L.YDL_BF16, None, None, None, None, None) != 0
    assert b"multiples of 16" in L.lib().ydl_last_error()
