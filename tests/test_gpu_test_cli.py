"""GPU: test_seg.py in process — a checkpoint saved from a random-init model, one synthetic 64 x 64 batch (metrics block, pictures
of the source size), and a --source / --labels directory whose pictures come back at each source's own size."""
import os

import numpy as np
import pytest
import torch

from tests import predict_ref as R

pytestmark = pytest.mark.gpu


def _checkpoint(tmp_path, arch):
    import argparse
    import train_seg
    import yolo_dual_amd as ydl
    torch.manual_seed(5)
    model, _ = train_seg.build_model(argparse.Namespace(arch=arch, cfg="", imgsz=64, dcn="substitute"))
    path = str(tmp_path / "random.pt")
    ydl.save_checkpoint(path, model.state_dict())
    return path


def test_cli_on_a_synthetic_batch(tmp_path, capsys):
    import test_seg
    from PIL import Image
    import yolo_dual_amd as ydl
    weights = _checkpoint(tmp_path, "yolov5")
    out_dir = tmp_path / "out"
    try:
        res = test_seg.main(["--weights", weights, "--arch", "yolov5", "--imgsz", "64", "--batch-size", "2", "--batches", "1",
                             "--visualize-num", "2", "--save-dir", str(out_dir)])
    finally:
        ydl.set_compute_dtype("bf16")
    text = capsys.readouterr().out
    assert "entries match" in text
    for key in ("mIoU:", "Accuracy:", "IoU per class:", "Accuracy per class:"):
        assert key in text, key
    assert sorted(k for k in res if k not in ("files", "samples")) == ["Accuracy", "Class_Accuracy", "IoU", "mIoU"]
    assert 0.0 <= res["mIoU"] <= 1.0 and 0.0 <= res["Accuracy"] <= 1.0 and len(res["IoU"]) == 12 and res["samples"] == 2
    names = sorted(os.path.basename(f) for f in res["files"])
    assert names == sorted(f"synthetic_0_{i}_{k}.png" for i in (0, 1) for k in ("colour", "difference", "overlay"))
    for f in res["files"]:
        im = Image.open(f)
        assert im.size == (64, 64) and im.mode == "RGB"


def test_cli_on_a_directory_writes_pictures_of_the_source_size(tmp_path, capsys):
    import test_seg
    import train_seg
    import argparse
    from PIL import Image
    import yolo_dual_amd as ydl
    weights = _checkpoint(tmp_path, "resnet18")
    src, lab, out_dir = tmp_path / "images", tmp_path / "labels", tmp_path / "out"
    src.mkdir()
    lab.mkdir()
    rs = np.random.RandomState(9)
    sizes = {"a": (100, 37), "b": (37, 100)}
    for stem, (w, h) in sizes.items():
        Image.fromarray(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(src / f"{stem}.png")
        Image.fromarray(rs.randint(0, 12, size=(h, w)).astype(np.uint8)).save(lab / f"{stem}.png")
    pal = tmp_path / "pal.npz"
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_render.npz"))
    np.savez(pal, palette=g["palette"], names=g["names"])
    try:
        res = test_seg.main(["--weights", weights, "--arch", "resnet18", "--imgsz", "64", "--batch-size", "2", "--dtype", "f32",
                             "--source", str(src), "--labels", str(lab), "--palette", str(pal), "--save-dir", str(out_dir)])
        # the same prediction through the public functions, drawn by the CPU restatement
        model, _ = train_seg.build_model(argparse.Namespace(arch="resnet18", cfg="", imgsz=64, dcn="substitute"))
        ydl.load_weights(model, weights)
        model = model.cuda().eval()
        lb = ydl.LetterboxGPU(64, num_classes=12)
        for stem, (w, h) in sizes.items():
            x, _ = lb(np.array(Image.open(src / f"{stem}.png")))
            labels = ydl.predict_labels(model, x.unsqueeze(0))[0].cpu().numpy()
            want = R.colorize(R.unletterbox(labels, w, h, 64), g["palette"])
            got = np.array(Image.open(out_dir / f"{stem}_colour.png"))
            assert got.shape == (h, w, 3) and np.array_equal(got, want)
    finally:
        ydl.set_compute_dtype("bf16")
    text = capsys.readouterr().out
    assert "class 0 (sky)" in text and "mIoU:" in text
    assert len(res["files"]) == 6
    for f in res["files"]:
        stem = os.path.basename(f).split("_")[0]
        assert Image.open(f).size == sizes[stem]
