"""GPU: train_seg.py --augment puts AugmentGPU in front of the letterbox; without the flag (or with an empty plan) nothing changes."""
import math

import pytest

pytestmark = pytest.mark.gpu

ARGS = ["--arch", "resnet18", "--batch-size", "4", "--imgsz", "64", "--steps-per-epoch", "4", "--epochs", "1", "--raw-size", "200x150",
        "--nosave", "--dtype", "f32"]


def test_train_cli_with_augmentations(tmp_path):
    import train_seg
    import yolo_dual_amd as ydl
    from yolo_dual_amd import _lib as L
    seen = []
    rec = L.call

    def spy(name, *a):
        seen.append(name)
        return rec(name, *a)
    L.call = spy
    try:
        fit = train_seg.train(train_seg.parse_opt(ARGS + ["--augment", "--save-dir", str(tmp_path / "a")]))
    finally:
        L.call = rec
        ydl.set_compute_dtype("bf16")
    assert 0.0 <= fit <= 1.0
    assert math.isfinite(train_seg.LAST_RUN["loss"]) and math.isfinite(train_seg.LAST_RUN["param_sum"])
    assert any(n.startswith("ydl_aug_") for n in seen)          # 16 samples with the default probabilities: the stage ran


def test_augment_needs_raw_size(capsys):
    import train_seg
    with pytest.raises(SystemExit):
        train_seg.parse_opt(["--augment", "--imgsz", "64"])
    assert "--raw-size" in capsys.readouterr().err


def test_empty_plan_equals_run_without_the_flag(tmp_path, monkeypatch):
    import train_seg
    import yolo_dual_amd as ydl
    from yolo_dual_amd import data
    try:
        train_seg.train(train_seg.parse_opt(ARGS + ["--save-dir", str(tmp_path / "p")]))
        plain = dict(train_seg.LAST_RUN)
        monkeypatch.setattr(data, "draw_augmentations", lambda *a, **k: [])
        train_seg.train(train_seg.parse_opt(ARGS + ["--augment", "--save-dir", str(tmp_path / "e")]))
        empty = dict(train_seg.LAST_RUN)
    finally:
        ydl.set_compute_dtype("bf16")
    assert empty["param_sum"] == plain["param_sum"] and empty["param_abs_sum"] == plain["param_abs_sum"]
    assert empty["loss"] == plain["loss"]
