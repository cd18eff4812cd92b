"""CPU: the yaml builders construct the deformable blocks natively when asked (``deformable=True``) with the reference's
parameter names and shapes; the default still refuses them."""
import os

import pytest
import yaml

CFG = os.path.join(os.path.dirname(__file__), "..", "yolo_dual_amd", "cfg")
# 3 x 32 x 32 -> 32 ch @ 16^2 -> C3_DCN with two DCNv2 bottlenecks (64 ch) -> 12 classes
YAML = {"nc": 12, "depth_multiple": 1.0, "width_multiple": 1.0,
        "backbone": [[-1, 1, "Conv", [32, 3, 2]], [-1, 2, "C3_DCN", [64]]], "head": [[-1, 1, "Conv", [12, 1, 1]]]}


def _cfg(name):
    return yaml.safe_load(open(os.path.join(CFG, name)))


def _block_keys(prefix, c, inner):
    """one inner DCN block: Sequential(Conv(c, c, 3, act=False), Conv(c, 18, 3), DeformConv2d(c, c, 3, padding=1, bias=False),
    Sequential(BatchNorm2d(c), SiLU)) — unet-lite/yolo5-seg/seg_diceloss_yolov5.py:449-454, yolov8/seg_diceloss_yolov8.py:436-446"""
    bn = lambda p, n: [(f"{p}.weight", (n,)), (f"{p}.bias", (n,)), (f"{p}.running_mean", (n,)), (f"{p}.running_var", (n,)),
                       (f"{p}.num_batches_tracked", ())]
    return ([(f"{prefix}.{inner}.0.conv.weight", (c, c, 3, 3))] + bn(f"{prefix}.{inner}.0.bn", c) +
            [(f"{prefix}.{inner}.1.conv.weight", (18, c, 3, 3))] + bn(f"{prefix}.{inner}.1.bn", 18) +
            [(f"{prefix}.{inner}.2.weight", (c, c, 3, 3))] + bn(f"{prefix}.{inner}.3.0", c))


def _conv_keys(prefix, c1, c2, k):
    return [(f"{prefix}.conv.weight", (c2, c1, k, k)), (f"{prefix}.bn.weight", (c2,)), (f"{prefix}.bn.bias", (c2,)),
            (f"{prefix}.bn.running_mean", (c2,)), (f"{prefix}.bn.running_var", (c2,)), (f"{prefix}.bn.num_batches_tracked", ())]


def test_yolov5seg_native_c3_dcn():
    import yolo_dual_amd as ydl
    m = ydl.YOLOv5Seg(_cfg("yolov5_seg.yaml"), deformable=True)
    assert [type(m.backbone[i]).__name__ for i in (4, 6, 8)] == ["C3_DCN"] * 3
    # C3_DCN(c1=256, c2=256): cv1, cv2, cv3 then m (seg_diceloss_yolov5.py:431-456), n = 1 (the yaml number is ignored)
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("backbone.4.")}
    want = (_conv_keys("backbone.4.cv1", 256, 128, 1) + _conv_keys("backbone.4.cv2", 256, 128, 1) +
            _conv_keys("backbone.4.cv3", 256, 256, 1) + _block_keys("backbone.4.m", 128, 0))
    assert list(sd.items()) == want


def test_yolov8seg_native_c2f_dcn():
    import yolo_dual_amd as ydl
    m = ydl.YOLOv8Seg(_cfg("yolov8_seg.yaml"), deformable=True)
    assert [type(m.backbone[i]).__name__ for i in (4, 6, 8)] == ["C2f_DCN"] * 3
    # C2f_DCN(c1=256, c2=256): cv1 (c1 -> 2c), cv2 ((2+n)c -> c2), m (yolov8/seg_diceloss_yolov8.py:417-447)
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("backbone.4.")}
    want = (_conv_keys("backbone.4.cv1", 256, 256, 1) + _conv_keys("backbone.4.cv2", 384, 256, 1) +
            _block_keys("backbone.4.m", 128, 0))
    assert list(sd.items()) == want


def test_default_still_refuses_dcn_rows():
    import yolo_dual_amd as ydl
    with pytest.raises(NotImplementedError, match="parity unpinned"):
        ydl.YOLOv5Seg(_cfg("yolov5_seg.yaml"))
    with pytest.raises(NotImplementedError, match="parity unpinned"):
        ydl.YOLOv8Seg(_cfg("yolov8_seg.yaml"))


def test_weight_groups_rejected():
    import yolo_dual_amd as ydl
    with pytest.raises(NotImplementedError, match="groups"):
        ydl.DeformConv2d(8, 8, 3, padding=1, groups=2)


def test_parse_model_resolves_c3_dcn_to_the_common_dcnv2_block():
    """models/yolo.py:321,327: C3_DCN gets (c1, c2) and n inserted; models/common.py:1629-1711: DCNv2 with a zero-initialised
    biased conv_offset_mask (27 = 3 * 3 * 3 channels) and a zero bias"""
    import yolo_dual_amd as ydl
    d = YAML
    with pytest.raises(NotImplementedError, match="outside the segmentation hot path"):
        ydl.parse_model(d, [3])
    seq, _ = ydl.parse_model(d, [3], deformable=True)
    blk = seq[1]
    assert type(blk).__name__ == "C3_DCNCommon" and len(blk.m) == 2
    sd = {k: tuple(v.shape) for k, v in blk.state_dict().items() if k.startswith("m.0.")}
    want = ([("m.0.cv1.conv.weight", (32, 32, 1, 1))] +
            [(f"m.0.cv1.bn.{n}", (32,)) for n in ("weight", "bias", "running_mean", "running_var")] + [("m.0.cv1.bn.num_batches_tracked", ())] +
            [("m.0.cv2.weight", (32, 32, 3, 3)), ("m.0.cv2.bias", (32,)), ("m.0.cv2.conv_offset_mask.weight", (27, 32, 3, 3)),
             ("m.0.cv2.conv_offset_mask.bias", (27,))] +
            [(f"m.0.cv2.bn.{n}", (32,)) for n in ("weight", "bias", "running_mean", "running_var")] + [("m.0.cv2.bn.num_batches_tracked", ())])
    assert list(sd.items()) == want
    # the model-level kaiming pass keeps DCNv2's initialisation (models/common.py:1681-1690)
    m = ydl.SegYoloModel(d, deformable=True)
    for b in m.model[1].m:
        dc = b.cv2
        assert float(dc.conv_offset_mask.weight.detach().abs().max()) == 0.0
        assert float(dc.conv_offset_mask.bias.detach().abs().max()) == 0.0 and float(dc.bias.detach().abs().max()) == 0.0
        assert float(dc.weight.detach().abs().max()) <= 1 / (32 * 9) ** 0.5


def test_train_seg_dcn_flag_builds_native_blocks():
    import train_seg
    import yolo_dual_amd as ydl
    cfg = os.path.join(CFG, "yolov5_seg.yaml")
    m, _ = train_seg.build_model(train_seg.parse_opt(["--cfg", cfg, "--dcn", "native"]))
    assert isinstance(m.backbone[4], ydl.C3_DCN)
    m, _ = train_seg.build_model(train_seg.parse_opt(["--cfg", cfg]))
    assert type(m.backbone[4]) is ydl.C3
