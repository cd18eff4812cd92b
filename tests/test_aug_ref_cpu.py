"""CPU: the numpy restatement of the seven augmentations (tests/aug_ref.py) equals what the reference's own classes produced with
Pillow (tests/golden/aug_*.npz, written by tools/make_aug_golden.py) byte for byte; ``draw_augmentations`` consumes ``random`` as
the reference does; where Pillow imports, the restatement equals Pillow itself over random sizes and parameters."""
import glob
import os
import random

import numpy as np
import pytest

from tests import aug_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SAMPLES = sorted(glob.glob(os.path.join(GOLD, "aug_sample_*.npz")))


def _plan(d):
    out = []
    for k, p in zip(d["plan_ops"], d["plan_params"]):
        op = R.OPS[int(k)]
        n = {"fliplr": 0, "flipud": 0, "crop": 4}.get(op, 1)
        out.append((op, tuple(int(v) for v in p[:4]) if op == "crop" else tuple(float(v) for v in p[:n])))
    return out


def _case_params(op, p):
    return tuple(int(v) for v in p) if op == "crop" else tuple(float(v) for v in p[:{"fliplr": 0, "flipud": 0}.get(op, 1)])


def test_fixture_set_exercises_every_op():
    """read off the recorded plans: every op fires at least twice over the whole-sample fixtures, one sample applies four or more"""
    assert len(SAMPLES) >= 4
    count = {op: 0 for op in R.OPS}
    longest = 0
    for f in SAMPLES:
        plan = _plan(np.load(f))
        longest = max(longest, len(plan))
        for op, _ in plan:
            count[op] += 1
    assert all(v >= 2 for v in count.values()), count
    assert longest >= 4


@pytest.mark.parametrize("op", R.OPS)
def test_single_op_equals_fixture(op):
    d = np.load(os.path.join(GOLD, f"aug_op_{op}.npz"))
    for c in (0, 1):
        img, mask = d[f"c{c}/img"], d[f"c{c}/mask"]
        oi, om = R.apply_op(img, mask, op, _case_params(op, d[f"c{c}/params"]))
        assert oi.dtype == np.uint8 and om.dtype == np.uint8
        assert np.array_equal(oi, d[f"c{c}/out_img"])
        assert np.array_equal(om, d[f"c{c}/out_mask"])
        if op in ("brightness", "contrast", "blur"):
            assert np.array_equal(d[f"c{c}/out_mask"], mask)
        assert not np.array_equal(oi, img)


@pytest.mark.parametrize("path", SAMPLES, ids=[os.path.basename(p)[:-4] for p in SAMPLES])
def test_whole_sample_equals_fixture(path):
    d = np.load(path)
    w, h, S, nc = (int(v) for v in d["meta"])
    ai, am = R.apply_plan(d["img"], d["mask"], _plan(d))
    assert np.array_equal(ai, d["aug_img"]) and np.array_equal(am, d["aug_mask"])
    oi, om = R.letterbox(ai, am, S, nc)
    assert oi.dtype == np.float32 and om.dtype == np.int64
    assert np.array_equal(oi, d["out_img"]) and np.array_equal(om, d["out_mask"])


@pytest.mark.parametrize("path", SAMPLES, ids=[os.path.basename(p)[:-4] for p in SAMPLES])
def test_draw_augmentations_follows_the_reference(path):
    """same plan under the fixture's seed, and ``random`` left in the recorded state; both for the package's draw and aug_ref's"""
    from yolo_dual_amd.data import draw_augmentations
    d = np.load(path)
    w, h = int(d["meta"][0]), int(d["meta"][1])
    hyp = {"fliplr": float(d["hyp"][0]), "flipud": float(d["hyp"][1]), "degrees": float(d["hyp"][2])}
    for draw, hy in ((draw_augmentations, hyp), (draw_augmentations, None), (R.draw_plan, hyp)):     # (draw_plan: same text, kept in step)
        rng = random.Random(int(d["seed"]))
        plan = draw(hy, w, h, rng)
        assert plan == _plan(d)
        assert np.array_equal(np.array(rng.getstate()[1], np.uint32), d["state_after"])
    random.seed(int(d["seed"]))                               # the module-level generator is the default
    assert draw_augmentations(hyp, w, h) == _plan(d)
    assert np.array_equal(np.array(random.getstate()[1], np.uint32), d["state_after"])


def test_draw_augmentations_hyp_and_tiny_images():
    from yolo_dual_amd.data import draw_augmentations
    always = draw_augmentations({"fliplr": 1.0, "flipud": 1.0, "degrees": 0}, 1, 1, random.Random(3))
    ops = [op for op, _ in always]
    assert "fliplr" in ops and "flipud" in ops
    for op, p in always:
        if op == "rotation":
            assert p == (0.0,) or p == (-0.0,)
        if op == "crop":
            assert p == (0, 0, 1, 1)
    never = [op for s in range(50) for op, _ in draw_augmentations({"fliplr": 0.0, "flipud": 0.0}, 9, 7, random.Random(s))]
    assert "fliplr" not in never and "flipud" not in never and "crop" in never


def test_aug_ref_equals_pillow():
    """random sizes (odd, non-square, tiny), angles of both signs, radii and factors across their ranges: zero differing bytes"""
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance, ImageFilter, ImageOps
    rs, rnd = np.random.RandomState(5), random.Random(11)
    sizes = [(72, 96), (33, 51), (5, 7), (101, 67), (1, 9), (9, 1), (3, 3), (2, 31), (64, 64)]
    for (H, W) in sizes:
        a = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        m = rs.randint(0, 12, (H, W)).astype(np.uint8)
        im, mk = Image.fromarray(a), Image.fromarray(m)
        assert np.array_equal(np.array(ImageOps.mirror(im)), R.fliplr(a)) and np.array_equal(np.array(ImageOps.mirror(mk)), R.fliplr(m))
        assert np.array_equal(np.array(ImageOps.flip(im)), R.flipud(a)) and np.array_equal(np.array(ImageOps.flip(mk)), R.flipud(m))
        for t in range(10):
            ang = rnd.uniform(-15, 15) if t < 7 else rnd.uniform(-89, 89)
            f = (0.7, 1.3, 1.0)[t] if t < 3 else rnd.uniform(0.7, 1.3)
            rad = (0.5, 2.0)[t] if t < 2 else rnd.uniform(0.5, 2.0)
            s = rnd.uniform(0.7, 1.0)
            nw, nh = max(1, int(W * s)), max(1, int(H * s))
            x1, y1 = rnd.randint(0, W - nw), rnd.randint(0, H - nh)
            box = (x1, y1, x1 + nw, y1 + nh)
            pairs = {
                "rotate image": (im.rotate(ang, resample=Image.BILINEAR), R.rotate_image(a, ang)),
                "rotate mask": (mk.rotate(ang, resample=Image.NEAREST), R.rotate_mask(m, ang)),
                "brightness": (ImageEnhance.Brightness(im).enhance(f), R.brightness(a, f)),
                "contrast": (ImageEnhance.Contrast(im).enhance(f), R.contrast(a, f)),
                "blur": (im.filter(ImageFilter.GaussianBlur(radius=rad)), R.gaussian_blur(a, rad)),
                "crop image": (im.crop(box).resize((W, H), Image.BILINEAR), R.crop_image(a, x1, y1, nw, nh)),
                "crop mask": (mk.crop(box).resize((W, H), Image.NEAREST), R.crop_mask(m, x1, y1, nw, nh)),
            }
            for name, (pil, ref) in pairs.items():
                assert int((np.array(pil) != ref).sum()) == 0, (name, H, W, ang, f, rad, box)


def test_host_side_parameters_equal_aug_ref():
    """A consistency check, not an independent one: yolo_dual_amd.data builds the matrices, fixed-point entries and box weights it
    hands to the kernels with the same few lines as aug_ref (as draw_augmentations mirrors draw_plan), so this only catches the two
    drifting apart.  What pins the arithmetic is Pillow: the fixtures its own run wrote and the direct comparison above."""
    from yolo_dual_amd import data as D
    rnd = random.Random(2)
    for _ in range(200):
        w, h, ang = rnd.randint(1, 2000), rnd.randint(1, 2000), rnd.uniform(-89.9, 89.9) % 360.0
        assert D._rotate_matrix(w, h, ang) == R.rotate_matrix(w, h, ang)
        assert D._rotate_fixed(D._rotate_matrix(w, h, ang)) == R.rotate_fixed(w, h, ang)
        rad = rnd.uniform(0.5, 2.0)
        assert D._box_weights(rad) == R.box_weights(R.box_radius(rad))


def test_sizes_are_required():
    from yolo_dual_amd.data import draw_augmentations
    with pytest.raises(TypeError):
        draw_augmentations({})


def test_angles_whose_sine_rounds_to_zero_are_copies_in_pillow():
    """|angle| tiny, or a tiny negative angle that ``% 360`` turns into 360.0: Image.rotate's matrix is the identity and both
    resampling paths return the source bytes, which is what AugmentGPU assumes when it skips such a rotation"""
    pytest.importorskip("PIL")
    from PIL import Image
    from yolo_dual_amd import data as D
    rs = np.random.RandomState(9)
    a = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    m = rs.randint(0, 12, (37, 53)).astype(np.uint8)
    for ang in (1e-14, -1e-14, -1e-20, 3e-15):
        mt = D._rotate_matrix(53, 37, ang % 360.0)
        assert mt[1] == 0.0 and mt[3] == 0.0 and mt[0] == 1.0 and mt[4] == 1.0 and mt[2] == 0.0 and mt[5] == 0.0
        assert np.array_equal(np.array(Image.fromarray(a).rotate(ang, resample=Image.BILINEAR)), a)
        assert np.array_equal(np.array(Image.fromarray(m).rotate(ang, resample=Image.NEAREST)), m)
        assert np.array_equal(R.rotate_image(a, ang), a) and np.array_equal(R.rotate_mask(m, ang), m)
