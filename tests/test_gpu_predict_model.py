"""GPU: yolo_dual_amd.predict on whole models.  predict_labels equals model(x).argmax(1) without running the softmax or the NCHW
export, the metrics built from its labels equal a numpy recomputation, and the un-letterbox equals tests/predict_ref.py."""
import functools
import os

import numpy as np
import pytest
import torch
import yaml

from tests import predict_ref as R
from tests.launch_trace import launch_trace

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "yolo_dual_amd", "cfg")
FAMILIES = ["YOLOv5Seg", "YOLOv8Seg", "ResNet18Seg"]
S, NC = 64, 12


def _cfg(name, swap):
    cfg = yaml.safe_load(open(os.path.join(CFG, name)))
    for sec in ("backbone", "head"):
        for l in cfg[sec]:
            l[2] = swap.get(l[2], l[2])
    return cfg


def _model(family):
    import yolo_dual_amd as ydl
    torch.manual_seed(3)
    if family == "ResNet18Seg":
        return ydl.ResNet18Seg({"nc": NC}).cuda().eval()
    cfg = _cfg("yolov5_seg.yaml", {"C3_DCN": "C3"}) if family == "YOLOv5Seg" else _cfg("yolov8_seg.yaml", {"C2f_DCN": "C2f"})
    m = getattr(ydl, family)(cfg)
    m.img_size = [S, S]
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _case(family, mode):
    """one forward each way per (family, dtype), shared by the tests below and left unchanged"""
    import yolo_dual_amd as ydl
    ydl.set_compute_dtype(mode)
    try:
        m = _model(family)
        g = torch.Generator().manual_seed(11)
        x = torch.rand(2, 3, S, S, generator=g).cuda()
        t = torch.randint(0, NC, (2, S, S), generator=g).cuda()
        with torch.no_grad():
            out = m(x)
        trace = launch_trace(lambda: ydl.predict_labels(m, x))
        labels = ydl.predict_labels(m, x)
        with torch.no_grad():
            model_trace = launch_trace(lambda: m(x))
        torch.cuda.synchronize()
    finally:
        ydl.set_compute_dtype("bf16")
    return m, x, t, out, labels, trace, model_trace


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("family", FAMILIES)
def test_predict_labels_equal_argmax_of_the_model_output(family, mode):
    m, x, t, out, labels, _, _ = _case(family, mode)
    assert out.shape == (2, NC, S, S) and out.dtype == torch.float32
    assert labels.shape == (2, S, S) and labels.dtype == torch.uint8 and labels.is_cuda
    assert not m.training
    out, labels = out.cpu(), labels.cpu()
    want = out.argmax(1)
    differ = labels.long() != want
    top2 = out.topk(2, dim=1).values
    tie = top2[:, 0] == top2[:, 1]
    share = float(differ.float().mean())
    print(f"{family} {mode}: {int(differ.sum())} of {differ.numel()} labels differ from model(x).argmax(1) ({100 * share:.4f} %), "
          f"{int(tie.sum())} pixels with tied top-2 probabilities, {len(torch.unique(want))} classes predicted")
    assert not bool((differ & ~tie).any())            # argmax before the softmax may differ only where the probabilities tie
    assert share <= 1e-3


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("family", FAMILIES)
def test_no_softmax_and_no_nchw_export_after_the_last_convolution(family, mode):
    _, _, _, _, _, trace, model_trace = _case(family, mode)
    names = [op[0] for op in trace if op[0] != "edge"]
    convs = [i for i, n in enumerate(names) if "conv" in n and "fwd" in n]
    # YOLOv8Seg's Upsample rows emit 256 x 256 whatever the input: its Softmax is followed by a bilinear resize to img_size, and the
    # labels come from the launch that does softmax, resize and argmax in one
    exit_launch = "ydl_softmax_resize_labels" if family == "YOLOv8Seg" else "ydl_argmax_labels"
    assert convs and sum(n in ("ydl_argmax_labels", "ydl_softmax_resize_labels") for n in names) == 1
    tail = names[convs[-1] + 1:]
    assert exit_launch in tail and "ydl_resize_fwd" not in tail[tail.index(exit_launch):]
    assert "ydl_softmax_fwd" not in tail and "ydl_nhwc_to_nchw" not in tail, tail
    # what model(x) runs there, for contrast: the yaml models end in the softmax that writes NCHW, ResNet18Seg in the NCHW export
    mnames = [op[0] for op in model_trace if op[0] != "edge"]
    mconvs = [i for i, n in enumerate(mnames) if "conv" in n and "fwd" in n]
    mtail = mnames[mconvs[-1] + 1:]
    assert ("ydl_nhwc_to_nchw" if family == "ResNet18Seg" else "ydl_softmax_fwd") in mtail
    assert names[:convs[-1] + 1] == mnames[:mconvs[-1] + 1]          # the same forward up to there
    if family != "ResNet18Seg":
        assert "ydl_softmax_fwd" not in names
    if family == "YOLOv5Seg":
        op = [o for o in trace if o[0] == "ydl_argmax_labels"][0]
        assert op[4] == 1 and (op[11], op[12]) != (1, 1)            # NHWC rows at the stored resolution, replication in the store


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("family", FAMILIES)
def test_metrics_from_labels(family, mode):
    import yolo_dual_amd as ydl
    _, _, t, out, labels, _, _ = _case(family, mode)
    want_labels = out.cpu().argmax(1).numpy()
    tn = t.cpu().numpy()
    sm = ydl.SegmentationMetrics(NC)
    sm.update(labels, t)
    sm.update(labels[1], t[1].to(torch.uint8))                     # one image, uint8 target: accumulates
    ref = R.SegmentationMetrics(NC)
    ref.update(want_labels, tn)
    ref.update(want_labels[1], tn[1])
    assert np.array_equal(sm.confusion_matrix.cpu().numpy(), ref.confusion_matrix)
    got, want = sm.get_metrics(), ref.get_metrics()
    assert sorted(got) == ["Accuracy", "Class_Accuracy", "IoU", "mIoU"]
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    a, b = ydl.ConfusionMatrix(NC, ignore_index=NC - 1), ydl.ConfusionMatrix(NC, ignore_index=NC - 1)
    a.process_labels(labels, t)
    b.process_batch(out, t)
    assert np.array_equal(a.matrix.cpu().numpy(), R.confusion(want_labels, tn, NC, NC - 1))
    assert torch.equal(a.matrix, b.matrix)
    assert a.compute_iou() == b.compute_iou()


def test_argmax_labels_of_strided_scores():
    import yolo_dual_amd as ydl
    _, _, _, out, _, _, _ = _case("ResNet18Seg", "f32")
    assert torch.equal(ydl.argmax_labels(out).cpu().long(), out.cpu().argmax(1))
    nhwc = out.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert torch.equal(ydl.argmax_labels(nhwc.bfloat16()).cpu().long(), nhwc.bfloat16().float().cpu().argmax(1))
    part = out[:, 2:9, 1::2, ::3]
    assert torch.equal(ydl.argmax_labels(part).cpu().long(), part.cpu().argmax(1))
    with pytest.raises(RuntimeError, match="GPU only"):
        ydl.argmax_labels(out.cpu())


@pytest.mark.parametrize("w,h", R.UNLETTERBOX_CASES)
def test_unletterbox_of_a_prediction(w, h):
    import yolo_dual_amd as ydl
    m, _, _, _, _, _, _ = _case("ResNet18Seg", "f32")
    rs = np.random.RandomState(w)
    img = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    mask = rs.randint(0, NC, size=(h, w)).astype(np.uint8)
    lb = ydl.LetterboxGPU(R.UNLETTERBOX_S, num_classes=NC)
    x, tm = lb(img, mask)
    ydl.set_compute_dtype("f32")
    try:
        labels = ydl.predict_labels(m, x.unsqueeze(0))[0]
    finally:
        ydl.set_compute_dtype("bf16")
    for lab in (labels, tm.to(torch.uint8)):
        got = ydl.unletterbox_labels(lab, w, h, R.UNLETTERBOX_S)
        assert got.shape == (h, w) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), R.unletterbox(lab.cpu().numpy(), w, h, R.UNLETTERBOX_S))
    both = ydl.unletterbox_labels(torch.stack([labels, tm.to(torch.uint8)]), w, h, R.UNLETTERBOX_S)
    assert both.shape == (2, h, w) and torch.equal(both[1], ydl.unletterbox_labels(tm.to(torch.uint8), w, h, R.UNLETTERBOX_S))


def test_class_weights_and_pictures_through_the_public_functions(caplog):
    import yolo_dual_amd as ydl
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(golden, "predict_weights.npz"))
    masks = [g[f"mask_{i}"] for i in range(6)]
    masks[1] = torch.from_numpy(masks[1]).to(torch.uint8).cuda()         # a device uint8 mask among host int64 arrays
    with caplog.at_level("WARNING", logger="yolo_dual_amd"):
        w = ydl.label_class_weights(masks, int(g["nc"]))
    assert w.dtype == torch.float32 and np.array_equal(w.numpy(), g["weights"])
    assert sum("skipped" in r.message for r in caplog.records) == 2
    r = np.load(os.path.join(golden, "predict_render.npz"))
    pal = torch.from_numpy(r["palette"])
    gt, pred = torch.from_numpy(r["c0/gt"]).cuda(), torch.from_numpy(r["c0/pred"]).cuda()
    assert np.array_equal(ydl.colorize(pred, pal).cpu().numpy(), r["c0/colour"])
    assert np.array_equal(ydl.difference(gt, pred, pal).cpu().numpy(), r["c0/difference"])
    img = torch.rand(3, *pred.shape, generator=torch.Generator().manual_seed(1))
    for bgr in (False, True):
        got = ydl.overlay(img.cuda(), pred, pal, bgr=bgr)
        assert np.array_equal(got.cpu().numpy(), R.overlay(img.numpy(), r["c0/pred"], r["palette"], bgr))
