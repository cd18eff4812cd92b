#!/usr/bin/env python3
"""Dev-time generator of tests/golden/aug_*.npz: the reference's OWN augmentation classes and dataset methods, run with Pillow.

    python tools/make_aug_golden.py --reference <checkout of the reference project>

Nothing of the reference is copied: the line ranges of unet-lite/yolo5-seg/seg_diceloss_yolov5.py that hold the seven
augmentation classes + get_augmentations (:75-185) and _apply_augmentations / _resize_and_pad (:320-349) are exec'd in a namespace
whose ``random`` is a spy around ``random.Random(seed)``: it logs every draw, and the recorded plan is read off that log (which op
fired with which parameters), not recomputed.  Only inputs, plans, generator states and Pillow's outputs are written.

  aug_op_<op>.npz      the op alone (its class with p = 1), two cases: c<k>/img, mask, params[4], out_img, out_mask
  aug_sample_<n>.npz   a whole sample with augment=True: img, mask, seed, hyp, plan_ops, plan_params, state_after (the Mersenne
                       Twister state after the draw), aug_img / aug_mask (after _apply_augmentations), out_img / out_mask (after
                       _resize_and_pad and the conversion of __getitem__, :315-316), meta = (w, h, img_size, num_classes)

Seeds of the whole samples are searched so that, over the set, every op fires at least twice and one sample applies four or more."""
import argparse
import os
import random
import sys

import numpy as np
import torch
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
OPS = ("fliplr", "flipud", "rotation", "brightness", "contrast", "blur", "crop")
CLASSES = ("RandomHorizontalFlip", "RandomVerticalFlip", "RandomRotation", "RandomBrightness", "RandomContrast", "RandomGaussianBlur",
           "RandomCrop")
NC = 12


class SpyRandom:
    def __init__(self, seed):
        self.rng, self.log = random.Random(seed), []

    def _do(self, name, *args, **kw):
        r = getattr(self.rng, name)(*args, **kw)
        self.log.append((name, args, r))
        return r

    def random(self):
        return self._do("random")

    def uniform(self, a, b):
        return self._do("uniform", a, b)

    def randint(self, a, b):
        return self._do("randint", a, b)

    def sample(self, population, k):
        return self._do("sample", population, k=k)


def load_reference(ref, spy):
    path = os.path.join(ref, "unet-lite", "yolo5-seg", "seg_diceloss_yolov5.py")
    lines = open(path, encoding="utf-8").read().split("\n")
    ns = dict(Image=Image, ImageEnhance=ImageEnhance, ImageFilter=ImageFilter, ImageOps=ImageOps, np=np, torch=torch, random=spy)
    exec(compile("\n".join(lines[75 - 1:185]), path, "exec"), ns)
    exec(compile("class _DS:\n" + "\n".join(lines[320 - 1:349]), path, "exec"), ns)
    return ns


def read_plan(log, w, h):
    """the plan the logged draws amount to: sample() gives the order, each op's random() the decision, the rest its parameters"""
    it = iter(log)
    name, _args, order = next(it)
    assert name == "sample"
    plan = []
    for a in order:
        name, _args, r = next(it)
        assert name == "random"
        if not r < a.p:
            continue
        op = OPS[CLASSES.index(type(a).__name__)]
        if op in ("fliplr", "flipud"):
            plan.append((op, ()))
        elif op == "crop":
            (_n0, _a0, _scale), (_n1, a1, x1), (_n2, a2, y1) = next(it), next(it), next(it)
            plan.append((op, (x1, y1, w - a1[1], h - a2[1])))          # randint(0, w - new_w): the box size from the call itself
        else:
            plan.append((op, (next(it)[2],)))
    assert next(it, None) is None
    return plan


def sample_inputs(seed, w, h):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8), rs.randint(0, NC, size=(h, w)).astype(np.uint8)


def pack_plan(plan):
    ops = np.array([OPS.index(op) for op, _ in plan], np.int64)
    params = np.zeros((len(plan), 4), np.float64)
    for i, (_, p) in enumerate(plan):
        params[i, :len(p)] = p
    return ops, params


def gen_ops(ref):
    for k, op in enumerate(OPS):
        arrs = {}
        for c, (w, h) in enumerate([(100, 70), (45, 61)]):
            spy = SpyRandom(4000 + 10 * k + c)
            ns = load_reference(ref, spy)
            img, mask = sample_inputs(4100 + 10 * k + c, w, h)
            aug = ns[CLASSES[k]](p=1.0)
            oi, om = aug(Image.fromarray(img), Image.fromarray(mask))
            plan = read_plan([("sample", (), [aug])] + spy.log, w, h)
            assert len(plan) == 1 and plan[0][0] == op
            arrs.update({f"c{c}/img": img, f"c{c}/mask": mask, f"c{c}/params": pack_plan(plan)[1][0], f"c{c}/out_img": np.array(oi),
                         f"c{c}/out_mask": np.array(om)})
        np.savez_compressed(os.path.join(OUT, f"aug_op_{op}.npz"), **arrs)
        print("aug_op_" + op, {c: arrs[f"c{c}/params"].tolist() for c in (0, 1)})


def run_sample(ref, seed, w, h, S):
    spy = SpyRandom(seed)
    ns = load_reference(ref, spy)
    img, mask = sample_inputs(5000 + seed, w, h)
    ds = ns["_DS"]()
    ds.img_size, ds.augment, ds.augmentations = S, True, ns["get_augmentations"]({})
    ai, am = ds._apply_augmentations(Image.fromarray(img).convert("RGB"), Image.fromarray(mask))
    plan = read_plan(spy.log, w, h)
    pi, pm = ds._resize_and_pad(ai, am)
    out_i = torch.from_numpy(np.array(pi)).permute(2, 0, 1).float() / 255.0
    out_m = torch.from_numpy(np.array(pm)).long()
    state = np.array(spy.rng.getstate()[1], np.uint32)
    ops, params = pack_plan(plan)
    return plan, dict(img=img, mask=mask, seed=np.array(seed), hyp=np.array([0.5, 0.2, 15.0]), plan_ops=ops, plan_params=params,
                      state_after=state, aug_img=np.array(ai), aug_mask=np.array(am), out_img=out_i.numpy(), out_mask=out_m.numpy(),
                      meta=np.array([w, h, S, NC]))


def gen_samples(ref, n_max=8):
    sizes = [(100, 70, 64), (70, 100, 64), (97, 71, 96), (64, 64, 64)]
    need = {op: 2 for op in OPS}
    need_four, kept, seed = True, [], 0
    while (need_four or any(v > 0 for v in need.values())) and seed < 10000:
        w, h, S = sizes[len(kept) % len(sizes)]
        plan, arrs = run_sample(ref, seed, w, h, S)
        useful = any(need[op] > 0 for op, _ in plan) or (need_four and len(plan) >= 4)
        if useful and len(plan) >= 2:
            for op, _ in plan:
                need[op] -= 1
            need_four = need_four and len(plan) < 4
            kept.append((seed, plan, arrs))
        seed += 1
    assert len(kept) <= n_max and not need_four and all(v <= 0 for v in need.values()), (len(kept), need)
    for i, (seed, plan, arrs) in enumerate(kept):
        np.savez_compressed(os.path.join(OUT, f"aug_sample_{i}.npz"), **arrs)
        print(f"aug_sample_{i}: seed {seed}", [op for op, _ in plan])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference project")
    a = ap.parse_args()
    gen_ops(a.reference)
    gen_samples(a.reference)
