"""CPU: tests/predict_ref.py, the restatement the prediction kernels are held to, equals the recordings of the reference's own code
(tests/golden/predict_*.npz, tools/make_predict_golden.py) exactly, its nearest rule equals F.interpolate, and its comparisons
notice a wrong answer."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import predict_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


def test_pictures_equal_the_reference_recordings():
    g = _load("predict_render.npz")
    pal = g["palette"]
    assert pal.shape == (12, 3) and pal.dtype == np.uint8 and len(g["names"]) == 12
    for c in (0, 1):
        gt, pred = g[f"c{c}/gt"], g[f"c{c}/pred"]
        assert pred.max() >= len(pal)                       # labels the table lacks are part of the recording
        assert np.array_equal(R.colorize(pred, pal), g[f"c{c}/colour"])
        assert np.array_equal(R.difference(gt, pred, pal), g[f"c{c}/difference"])


def test_metrics_equal_the_reference_recording():
    g = _load("predict_metrics.npz")
    nc = int(g["nc"])
    m = R.SegmentationMetrics(nc)
    for p, t in zip(g["pred"], g["target"]):
        m.update(p, t)
    assert np.array_equal(m.confusion_matrix, g["matrix"])
    r = m.get_metrics()
    assert sorted(r) == ["Accuracy", "Class_Accuracy", "IoU", "mIoU"]
    for k in r:
        assert np.array_equal(np.asarray(r[k]), g[k]), k        # float64, same formulas: bit for bit
    assert g["matrix"][9].sum() == 0 and r["IoU"][9] == 0.0     # the class that never occurs: 0 / 1e-10, not NaN


def test_class_weights_equal_the_reference_recording():
    g = _load("predict_weights.npz")
    nc = int(g["nc"])
    masks = [g[f"mask_{i}"] for i in range(6)]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = R.class_weights(masks, nc)
    assert len(w) == 2                                           # the masks holding label nc and label -1
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), g["weights"])


def _pairs():
    out = set()
    for (_y0, _x0, hc, wc), (Ho, Wo) in R.RESIZE_CASES:
        out |= {(hc, Ho), (wc, Wo)}
    for w, h in R.UNLETTERBOX_CASES:
        _y, _x, nh, nw = R.letterbox_box(w, h, R.UNLETTERBOX_S)
        out |= {(nh, h), (nw, w)}
    return sorted(out)


@pytest.mark.parametrize("n_in,n_out", _pairs())
def test_nearest_rule_equals_interpolate(n_in, n_out):
    src = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in)
    want = F.interpolate(src, size=(1, n_out), mode="nearest").reshape(-1).long().numpy()
    assert np.array_equal(R.nearest_index(n_in, n_out), want)


def test_resize_equals_interpolate_on_the_box():
    rs = np.random.RandomState(3)
    canvas = rs.randint(0, 12, size=(2, 16, 16)).astype(np.uint8)
    for (y0, x0, hc, wc), (Ho, Wo) in R.RESIZE_CASES:
        box = torch.from_numpy(canvas[:, y0:y0 + hc, x0:x0 + wc]).float().unsqueeze(1)
        want = F.interpolate(box, size=(Ho, Wo), mode="nearest").squeeze(1).to(torch.uint8).numpy()
        assert np.array_equal(R.labels_resize(canvas, (y0, x0, hc, wc), Ho, Wo), want)


def test_letterbox_box_matches_the_product_geometry():
    from yolo_dual_amd import letterbox_geometry
    for w, h in R.UNLETTERBOX_CASES + [(64, 64), (640, 480)]:
        new_w, new_h, pl, pt = letterbox_geometry(w, h, R.UNLETTERBOX_S)
        assert R.letterbox_box(w, h, R.UNLETTERBOX_S) == (pt, pl, new_h, new_w)


def test_argmax_rule():
    x = torch.tensor([1.0, float("nan"), 3.0, float("nan")]).reshape(1, 4, 1, 1)
    assert R.argmax_labels(x).item() == 1
    assert R.argmax_labels(torch.full((1, 5, 1, 1), float("-inf"))).item() == 0
    assert R.argmax_labels(torch.tensor([2.0, 7.0, 7.0]).reshape(1, 3, 1, 1)).item() == 1
    assert R.argmax_labels(torch.zeros(1, 3, 2, 2), rep=(1, 3)).shape == (1, 2, 6)


def test_overlay_rounds_half_to_even():
    pal = np.array([[0, 1, 2], [255, 255, 255]], np.uint8)
    img = np.array([3.0 / 255, 4.0 / 255, 254.9 / 255], np.float32).reshape(3, 1, 1)
    base = (img.reshape(3) * np.float32(255)).astype(np.uint8)                 # truncation: 254.9 -> 254
    assert base.tolist() == [3, 4, 254]
    assert R.overlay(img, np.array([[0]], np.uint8), pal).reshape(3).tolist() == [2, 2, 128]      # 1.5 -> 2, 2.5 -> 2, 128
    assert R.overlay(img, np.array([[0]], np.uint8), pal, bgr=True).reshape(3).tolist() == [127, 2, 2]     # (254+0)/2, 2.5 -> 2, 2.5 -> 2
    assert R.overlay(img, np.array([[7]], np.uint8), pal).reshape(3).tolist() == [2, 2, 127]      # label beyond the palette: black


def test_comparisons_reject_a_wrong_answer():
    g = _load("predict_render.npz")
    pal, gt, pred = g["palette"], g["c0/gt"], g["c0/pred"]
    bad = pred.copy()
    bad[4, 6] = (bad[4, 6] + 1) % 12
    assert not np.array_equal(R.colorize(bad, pal), g["c0/colour"])            # one flipped label
    assert not np.array_equal(R.difference(gt, bad, pal), g["c0/difference"])
    off = pal.copy()
    off[3, 1] += 1
    assert (pred == 3).any() and not np.array_equal(R.colorize(pred, off), g["c0/colour"])       # one colour off by one
    m = _load("predict_metrics.npz")
    p = m["pred"].copy()
    keep = np.argwhere((m["target"] >= 0) & (m["target"] < 12))[0]
    p[tuple(keep)] = (p[tuple(keep)] + 1) % 12
    assert not np.array_equal(R.confusion(p, m["target"], 12), R.confusion(m["pred"], m["target"], 12))
