"""GPU: AugmentGPU (csrc/augment.hip) is byte for byte Pillow: each op alone and whole-sample chains against the fixtures the
reference's own classes wrote (tests/golden/aug_*.npz), each op against the numpy restatement (tests/aug_ref.py) at 960x720 and at
odd sizes, and ``lb(*aug(...))`` against the fixture's final float image and int64 mask.  The rotation and contrast cases are the
ones that fail when hipcc is allowed to contract a + b*c into an FMA."""
import glob
import os
import random

import numpy as np
import pytest
import torch

from tests import aug_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SAMPLES = sorted(glob.glob(os.path.join(GOLD, "aug_sample_*.npz")))


def _params(op, p):
    return tuple(int(v) for v in p[:4]) if op == "crop" else tuple(float(v) for v in p[:{"fliplr": 0, "flipud": 0}.get(op, 1)])


def _plan(d):
    return [(R.OPS[int(k)], _params(R.OPS[int(k)], p)) for k, p in zip(d["plan_ops"], d["plan_params"])]


def _eq(t, a):
    return t.is_cuda and torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(a)))


@pytest.mark.parametrize("op", R.OPS)
def test_single_op_equals_fixture(op):
    import yolo_dual_amd as ydl
    aug = ydl.AugmentGPU()
    d = np.load(os.path.join(GOLD, f"aug_op_{op}.npz"))
    for c in (0, 1):
        img, mask = d[f"c{c}/img"], d[f"c{c}/mask"]
        oi, om = aug(img, mask, [(op, _params(op, d[f"c{c}/params"]))])
        assert oi.dtype == torch.uint8 and om.dtype == torch.uint8
        assert _eq(oi, d[f"c{c}/out_img"]), op
        assert _eq(om, d[f"c{c}/out_mask"]), op


@pytest.mark.parametrize("path", SAMPLES, ids=[os.path.basename(p)[:-4] for p in SAMPLES])
def test_whole_sample_equals_fixture(path):
    """the recorded plan on the GPU, then the GPU letterbox: the reference's __getitem__ after decoding, bit for bit"""
    import yolo_dual_amd as ydl
    d = np.load(path)
    w, h, S, nc = (int(v) for v in d["meta"])
    aug, lb = ydl.AugmentGPU(), ydl.LetterboxGPU(S, num_classes=nc)
    plan = aug.plan(w, h, random.Random(int(d["seed"])))
    assert plan == _plan(d)
    ai, am = aug(d["img"], d["mask"], plan)
    assert _eq(ai, d["aug_img"]) and _eq(am, d["aug_mask"])
    oi, om = lb(*aug(torch.from_numpy(d["img"]).cuda(), torch.from_numpy(d["mask"]).cuda(), plan))
    assert oi.dtype == torch.float32 and om.dtype == torch.int64
    assert _eq(oi, d["out_img"]) and _eq(om, d["out_mask"])


def _cases(rnd, w, h):
    out = [("fliplr", ()), ("flipud", ())]
    out += [("rotation", (a,)) for a in (rnd.uniform(-15, 15), rnd.uniform(-15, 15), -89.5, 37.25, 0.0, 1e-3, 1e-14, -1e-20)]
    out += [("brightness", (f,)) for f in (0.7, 1.3, 1.0, rnd.uniform(0.7, 1.3), rnd.uniform(0.7, 1.3))]
    out += [("contrast", (f,)) for f in (0.7, 1.3, rnd.uniform(0.7, 1.3), rnd.uniform(0.7, 1.3))]
    out += [("blur", (r,)) for r in (0.5, 2.0, rnd.uniform(0.5, 2.0), 5.0)]
    for s in (0.7, 1.0, rnd.uniform(0.7, 1.0), rnd.uniform(0.7, 1.0)):
        nw, nh = max(1, int(w * s)), max(1, int(h * s))
        out.append(("crop", (rnd.randint(0, w - nw), rnd.randint(0, h - nh), nw, nh)))
    out.append(("crop", (0, h // 3, w, max(1, h // 2))))            # only the vertical pass
    out.append(("crop", (w // 3, 0, max(1, w // 2), h)))            # only the horizontal pass
    return out


@pytest.mark.parametrize("w,h", [(960, 720), (101, 67), (33, 51), (7, 5), (1, 9), (9, 1), (257, 3)])
def test_each_op_equals_restatement(w, h):
    import yolo_dual_amd as ydl
    aug = ydl.AugmentGPU()
    rs, rnd = np.random.RandomState(w * 1000 + h), random.Random(w + h)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    mask = rs.randint(0, 12, (h, w)).astype(np.uint8)
    for op, params in _cases(rnd, w, h):
        ri, rm = R.apply_op(img, mask, op, params)
        oi, om = aug(img, mask, [(op, params)])
        nd = int((oi.cpu().numpy() != ri).sum()), int((om.cpu().numpy() != rm).sum())
        assert nd == (0, 0), (op, params, nd)


def test_chain_equals_restatement_at_full_size():
    """all seven ops in a row at 960x720: the ping-pong between the scratch buffers loses nothing, and a second sample reuses them"""
    import yolo_dual_amd as ydl
    aug = ydl.AugmentGPU()
    rs = np.random.RandomState(77)
    for seed in (1, 2):
        img = rs.randint(0, 256, (720, 960, 3)).astype(np.uint8)
        mask = rs.randint(0, 12, (720, 960)).astype(np.uint8)
        plan = aug.plan(960, 720, random.Random(seed)) or []
        plan = [("contrast", (1.21,)), ("rotation", (-7.3,)), ("blur", (1.3,)), ("crop", (50, 40, 768, 576)), ("fliplr", ()),
                ("brightness", (0.83,)), ("flipud", ())] + plan
        ri, rm = R.apply_plan(img, mask, plan)
        oi, om = aug(img, mask, plan)
        assert _eq(oi, ri) and _eq(om, rm)


def test_mask_untouched_and_empty_plan_is_identity():
    import yolo_dual_amd as ydl
    aug = ydl.AugmentGPU()
    rs = np.random.RandomState(3)
    img = torch.from_numpy(rs.randint(0, 256, (70, 100, 3)).astype(np.uint8)).cuda()
    mask = torch.from_numpy(rs.randint(0, 12, (70, 100)).astype(np.uint8)).cuda()
    img0, mask0 = img.clone(), mask.clone()
    for op, p in (("brightness", (1.2,)), ("contrast", (0.8,)), ("blur", (1.0,))):
        oi, om = aug(img, mask, [(op, p)])
        assert torch.equal(om, mask0) and om.data_ptr() == mask.data_ptr()     # not touched, not copied
        assert not torch.equal(oi, img0)
    oi, om = aug(img, mask, [])
    assert torch.equal(oi, img0) and torch.equal(om, mask0)
    oi, om = aug(img.cpu().numpy(), mask.cpu().numpy(), [])
    assert oi.is_cuda and om.is_cuda and torch.equal(oi, img0) and torch.equal(om, mask0)
    oi, om = aug(img, mask, [("rotation", (0.0,)), ("crop", (0, 0, 100, 70))])    # Pillow: copies
    assert torch.equal(oi, img0) and torch.equal(om, mask0)
    assert torch.equal(img, img0) and torch.equal(mask, mask0)                  # the inputs are never written


def test_crop_tables_survive_cache_eviction():
    """a table cache far smaller than the crop key space: every crop evicts, and the tables of the call in flight must still be the
    right ones (they are held by the caller, not by the cache); the big default cache holds every key of a long run"""
    import yolo_dual_amd as ydl
    from yolo_dual_amd import data as D
    aug = ydl.AugmentGPU()
    assert aug._tables.capacity >= 4 * (960 - int(960 * 0.7) + 720 - int(720 * 0.7) + 2)
    aug._tables = D._DeviceTables(aug.device, 2)
    rs, rnd = np.random.RandomState(12), random.Random(12)
    w, h = 61, 45
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    mask = rs.randint(0, 12, (h, w)).astype(np.uint8)
    for _ in range(40):
        s = rnd.uniform(0.7, 1.0)
        nw, nh = max(1, int(w * s)), max(1, int(h * s))
        box = (rnd.randint(0, w - nw), rnd.randint(0, h - nh), nw, nh)
        oi, om = aug(img, mask, [("crop", box)])
        ri, rm = R.apply_op(img, mask, "crop", box)
        assert _eq(oi, ri) and _eq(om, rm), box
        assert len(aug._tables) <= 2
    lb = ydl.LetterboxGPU(32)
    lb._tables = D._DeviceTables(lb.device, 1)
    oi, om = lb(img, mask)
    ri, rm = R.letterbox(img, mask, 32)
    assert _eq(oi, ri) and _eq(om, rm)


def test_bad_arguments_raise():
    import yolo_dual_amd as ydl
    aug = ydl.AugmentGPU()
    img = np.zeros((8, 10, 3), np.uint8)
    mask = np.zeros((8, 10), np.uint8)
    with pytest.raises(TypeError):
        aug(img.astype(np.float32), mask, [])
    with pytest.raises(TypeError):
        aug(img, mask.astype(np.int64), [])
    with pytest.raises(TypeError):
        aug(img[..., 0], mask, [])
    with pytest.raises(ValueError, match="sizes differ"):
        aug(img, np.zeros((8, 9), np.uint8), [])
    with pytest.raises(ValueError, match="RGB"):
        aug(np.zeros((8, 10, 4), np.uint8), mask, [])
    with pytest.raises(ValueError, match="90"):
        aug(img, mask, [("rotation", (90.0,))])
    with pytest.raises(ValueError, match="90"):
        aug(img, mask, [("rotation", (-120.0,))])
    with pytest.raises(ValueError, match="90"):
        ydl.AugmentGPU({"degrees": 90})
    with pytest.raises(ValueError, match="crop box"):
        aug(img, mask, [("crop", (5, 0, 6, 8))])
    with pytest.raises(ValueError, match="unknown"):
        aug(img, mask, [("solarize", ())])


def test_entry_points_validate_on_the_host():
    """the C entry points refuse in-place calls and boxes that leave the image before any launch"""
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.tape import _p, _stream
    a = torch.zeros(8 * 10 * 3, dtype=torch.uint8, device="cuda")
    b = torch.zeros_like(a)
    with pytest.raises(L.YdlError, match="distinct"):
        L.call("ydl_aug_brightness", _p(a), _p(a), 8, 10, 1.1, _stream())
    with pytest.raises(L.YdlError, match="crop box"):
        L.call("ydl_aug_crop_mask", _p(a), 8, 10, 4, 0, 7, 8, _p(b), _p(a), _p(a), _stream())
    with pytest.raises(L.YdlError, match="size"):
        L.call("ydl_aug_flip", _p(a), _p(b), 8, 40000, 1, 1, _stream())
