"""GPU: train_seg.py --dcn native trains the yaml's C3_DCN rows natively for one tiny epoch (training, validation in eval mode,
checkpoint with the reference's keys, intersect-load into a fresh native model)."""
import os

import pytest

pytestmark = pytest.mark.gpu


def test_train_cli_dcn_native(tmp_path):
    import train_seg
    import yolo_dual_amd as ydl
    sd = str(tmp_path / "run")
    args = ["--cfg", os.path.join(os.path.dirname(__file__), "..", "yolo_dual_amd", "cfg", "yolov5_seg.yaml"), "--batch-size", "2",
            "--imgsz", "64", "--steps-per-epoch", "3", "--save-dir", sd, "--epochs", "1", "--dcn", "native"]
    fit = train_seg.train(train_seg.parse_opt(args))
    assert 0.0 <= fit <= 1.0
    m = train_seg.build_model(train_seg.parse_opt(args))[0]
    assert isinstance(m.backbone[4], ydl.C3_DCN)
    n, tot = ydl.load_weights(m, os.path.join(sd, "best.pt"))
    assert n == tot and any(k.endswith("m.0.2.weight") for k in m.state_dict())
    ydl.set_compute_dtype("bf16")
