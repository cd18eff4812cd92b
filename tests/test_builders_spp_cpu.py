"""CPU: the SPP pyramid family (models/common.py:191-197 C3SPP, :1275-1286 SPP, :1292-1330 SimConv / SimSPPF, :1430-1448 SPPCSPC,
:1473-1492 SimCSPSPPF) has the reference's constructor signatures and state_dict layout (key lists and shapes recorded from the
reference's own classes by tools/make_spp_golden.py), ``parse_model`` resolves the rows (models/yolo.py:317-326: width gain on c2, no
``n`` inserted, a yaml list passed through as ``k``), and the constructors refuse what the HIP path does not implement."""
import glob
import os

import numpy as np
import pytest

from tests.block_harness import build_from_json as build, check_state_dict_layout

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "spp_*.npz")))
# 3 x 32 x 32 input -> 16 ch @ 16^2 -> 32 ch @ 8^2 -> SPP -> SPPCSPC -> SimSPPF -> SimCSPSPPF -> C3SPP with two pools (all 32 ch; the
# hidden widths are 16 and 32) -> 12 classes
YAML = {"nc": 12, "width_multiple": 0.5, "depth_multiple": 0.33,
        "backbone": [[-1, 1, "Conv", [32, 6, 2, 2]], [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "SPP", [64]], [-1, 1, "SPPCSPC", [64]],
                     [-1, 1, "SimSPPF", [64, 5]], [-1, 1, "SimCSPSPPF", [64]], [-1, 1, "C3SPP", [64, [3, 5]]]],
        "head": [[-1, 1, "Conv", [12, 1, 1]]]}


def test_the_five_fixtures_are_present_and_small():
    assert [os.path.basename(f) for f in FILES] == ["spp_16_16.npz", "spp_c3_16_16_k35.npz", "spp_cspc_16_16.npz", "spp_sim_16_16.npz",
                                                    "spp_simcsp_16_16.npz"]
    # 128 KB each, except the SPPCSPC case: on its 2 x 16 x 20 x 13 input the four activation arrays (x, out, grad_out, grad_x: 8320
    # incompressible float32 values each) are 133 KB by themselves and the parameters and their gradients another 60 KB, so that
    # file (196 KB) is held to the 1 MiB cap for a committed file only
    sizes = {os.path.basename(f): os.path.getsize(f) for f in FILES}
    assert all(v < (1 << 20 if n == "spp_cspc_16_16.npz" else 128 * 1024) for n, v in sizes.items()), sizes
    assert [str(np.load(f)["cls"]) for f in FILES] == ["SPP", "C3SPP", "SPPCSPC", "SimSPPF", "SimCSPSPPF"]


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_state_dict_matches_the_reference_modules(path):
    check_state_dict_layout(path, build)


def test_constructor_forms():
    import torch.nn as nn
    import yolo_dual_amd as ydl
    assert ydl.SPP(16, 16, k=[5, 9, 13]).k == (5, 9, 13) == ydl.SPP(16, 16).k == ydl.SPPCSPC(16, 16).k
    assert ydl.SPP(16, 24, (3,)).cv2.conv.weight.shape == (24, 16, 1, 1)          # c_ * (len(k) + 1) input channels
    assert ydl.C3SPP(16, 16, [3, 5]).m.k == (3, 5) and ydl.C3SPP(16, 16).m.cv2.conv.weight.shape == (8, 16, 1, 1)
    sc = ydl.SimConv(8, 16, 3, 2)
    assert sc.conv.padding == (1, 1) and sc.conv.stride == (2, 2) and sc.conv.bias is None and isinstance(sc.act, nn.ReLU)
    assert ydl.SimConv(8, 16, 5, 1).conv.padding == (2, 2) and ydl.SimConv(8, 16, 1, 1).conv.padding == (0, 0)
    ss = ydl.SimSPPF(16, 24)
    assert ss.k == 5 and isinstance(ss.cv1, ydl.SimConv) and isinstance(ss.cv2.act, nn.ReLU) and ss.cv2.conv.weight.shape == (24, 32, 1, 1)
    # n, shortcut and g are accepted and unused, as in the reference
    a, b = ydl.SPPCSPC(16, 16, 3, True, 4, 0.5, (3, 7, 15)), ydl.SimCSPSPPF(16, 16, 3, True, 4, 0.5, 7)
    assert a.k == (3, 7, 15) and b.k == 7
    for m in (a, b):
        assert all(c.conv.groups == 1 for c in (m.cv1, m.cv2, m.cv3, m.cv4, m.cv5, m.cv6, m.cv7)) and isinstance(m.cv1.act, nn.SiLU)


def test_parse_model_builds_the_pyramid_rows():
    import yolo_dual_amd as ydl
    net = ydl.SegYoloModel(YAML)
    spp, cspc, sim, simcsp, c3, last = (net.model[i] for i in range(2, 8))
    assert [type(m) for m in (spp, cspc, sim, simcsp, c3, last)] == [ydl.SPP, ydl.SPPCSPC, ydl.SimSPPF, ydl.SimCSPSPPF, ydl.C3SPP, ydl.Conv]
    # width gain 0.5 on c2 (not on the class count); c1 from the previous row
    assert spp.cv1.conv.weight.shape == (16, 32, 1, 1) and spp.cv2.conv.weight.shape == (32, 64, 1, 1) and spp.k == (5, 9, 13)
    assert cspc.cv1.conv.weight.shape == (32, 32, 1, 1) and cspc.cv5.conv.weight.shape == (32, 128, 1, 1)
    assert cspc.cv7.conv.weight.shape == (32, 64, 1, 1) and cspc.cv3.conv.weight.shape == (32, 32, 3, 3)
    assert sim.k == 5 and sim.cv2.conv.weight.shape == (32, 64, 1, 1)
    assert simcsp.k == 5 and simcsp.cv6.conv.weight.shape == (32, 32, 3, 3)
    assert c3.m.k == (3, 5) and c3.cv1.conv.weight.shape == (16, 32, 1, 1) and c3.m.cv2.conv.weight.shape == (16, 24, 1, 1)
    assert last.conv.weight.shape == (12, 32, 1, 1)
    assert [m.type for m in (spp, cspc, sim, simcsp, c3)] == ["models.common." + n for n in ("SPP", "SPPCSPC", "SimSPPF", "SimCSPSPPF", "C3SPP")]
    # none of them is in the n-insertion set: n > 1 repeats the construction
    rep = ydl.parse_model({"nc": 12, "backbone": [[-1, 1, "Conv", [32, 3, 2]], [-1, 2, "C3SPP", [32, [3, 5]]]], "head": []}, [3])[0][1]
    assert len(rep) == 2 and all(type(m) is ydl.C3SPP and m.m.k == (3, 5) and len(m.m.k) == 2 for m in rep)


def test_what_the_hip_path_does_not_implement_is_refused():
    import yolo_dual_amd as ydl
    with pytest.raises(NotImplementedError, match="groups"):
        ydl.SPPCSPC_group(16, 16)
    with pytest.raises(NotImplementedError, match="groups"):
        ydl.SegYoloModel({"nc": 12, "backbone": [[-1, 1, "Conv", [32, 3, 2]], [-1, 1, "SPPCSPC_group", [32]]], "head": []})
    with pytest.raises(NotImplementedError, match="groups"):
        ydl.SimConv(8, 8, 3, 1, groups=2)
    with pytest.raises(NotImplementedError, match="bias"):
        ydl.SimConv(8, 8, 3, 1, bias=True)
    with pytest.raises(NotImplementedError, match="groups"):
        ydl.C3SPP(16, 16, (5, 9, 13), 1, True, 2)
    for make in (lambda: ydl.SPP(8, 8, (4,)), lambda: ydl.SPPCSPC(8, 8, k=(5, 8, 13)), lambda: ydl.SimSPPF(8, 8, 4),
                 lambda: ydl.SimCSPSPPF(8, 8, k=6), lambda: ydl.C3SPP(16, 16, (5, 6))):
        with pytest.raises(NotImplementedError, match="odd"):          # an even k with padding k // 2 changes the output size
            make()
