#!/usr/bin/env python3
"""The post-model tail of a validation batch, old against new, from the same stored scores, at BASELINE config 2's validation shape
(16 x 640^2, 12 classes, bf16: scores stored NHWC at 160^2 with the lazy nearest x4 pending):

  parent tail   what model(x) runs after the last convolution, ydl_softmax_fwd writing f32 NCHW probabilities at 640^2, then
                ConfusionMatrix.process_batch (ydl_confusion_matrix on them and the int64 targets)
  new tail      Tape.export_labels (ydl_argmax_labels, replication folded into the store) + ConfusionMatrix.process_labels
                (ydl_confusion_labels)

and the v8 family's exit (scores at 256^2, bilinear resize to 640^2): ydl_softmax_fwd + ydl_resize_fwd + ydl_nhwc_to_nchw against
ydl_softmax_resize_labels.  The groups alternate within every round, every round takes the next of --rotate operand sets and starts
behind a 1 GiB fill, so nothing is served from the 256 MB Infinity Cache and no launch latency sits inside an event pair.  Both tails
must give the same confusion matrix, and the new one must be faster than the parent's by more than the spread (max - min over the
timed rounds) of the two: the tool exits 1 otherwise.  The render, resize and histogram kernels are reported against their byte
floors at 640^2 (un-letterbox: 640 x 480 interior -> 960 x 720), without a threshold.

    python tools/predict_bench.py [--rounds 30] [--rotate 4] [--log profiles/predict_bench.log]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from yolo_dual_amd import _lib as L                      # noqa: E402
from yolo_dual_amd.tape import _p, _stream               # noqa: E402

COPY_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--size", type=int, default=160, help="stored height = width of the scores")
    ap.add_argument("--rep", type=int, default=4, help="pending nearest replication (output = size * rep)")
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=4)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = "cuda"
    N, C, h, r = a.bs, a.classes, a.size, a.rep
    S, ld = h * r, (C + 7) // 8 * 8
    dt, es = L.YDL_BF16, 2
    st = _stream()
    pal = torch.randint(0, 256, (C, 3), dtype=torch.uint8, device=dev)
    h8 = 256                                          # the v8 family's fixed Upsample size
    ldp = (C + 3) // 4 * 4
    sets = []
    for _ in range(a.rotate):
        # scores with the spatial coherence of a real prediction: 8 x 8 blobs of a favoured class plus noise
        fav = torch.randint(0, C, (N, h // 8 + 1, h // 8 + 1), device=dev).repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :h, :h]
        x = torch.randn(N, h, h, ld, device=dev)
        x.scatter_add_(3, fav.unsqueeze(-1), torch.full((N, h, h, 1), 4.0, device=dev))
        t = fav.repeat_interleave(r, 1).repeat_interleave(r, 2).contiguous()
        t[torch.rand(N, S, S, device=dev) < 0.1] = C - 1
        sets.append(dict(
            x=x.to(torch.bfloat16), t=t, p=torch.empty(N, C, S, S, device=dev), labels=torch.empty(N, S, S, dtype=torch.uint8, device=dev),
            m_old=torch.zeros(C, C, dtype=torch.int64, device=dev), m_new=torch.zeros(C, C, dtype=torch.int64, device=dev),
            x8=(torch.randn(N, h8, h8, ld, device=dev) * 3).to(torch.bfloat16), p8=torch.zeros(N, h8, h8, ldp, device=dev),
            y8=torch.empty(N, S, S, ldp, device=dev), img=torch.rand(N, 3, S, S, device=dev),
            rgb=torch.empty(N, S, S, 3, dtype=torch.uint8, device=dev), un=torch.empty(N, 720, 960, dtype=torch.uint8, device=dev),
            counts=torch.zeros(C + 1, dtype=torch.int64, device=dev)))

    def parent_tail(s):
        L.call("ydl_softmax_fwd", dt, _p(s["x"]), ld, _p(s["p"]), *s["p"].stride(), N, h, h, C, r, r, st)
        L.call("ydl_confusion_matrix", _p(s["p"]), *s["p"].stride(), _p(s["t"]), N, C, S, S, C - 1, _p(s["m_old"]), st)

    def new_tail(s):
        L.call("ydl_argmax_labels", dt, _p(s["x"]), h * h * ld, 1, h * ld, ld, N, C, h, h, r, r, _p(s["labels"]), S * S, S, st)
        L.call("ydl_confusion_labels", _p(s["labels"]), S * S, S, _p(s["t"]), 1, S * S, S, N, S, S, C, C - 1, _p(s["m_new"]), st)

    def parent_v8(s):
        L.call("ydl_softmax_fwd", dt, _p(s["x8"]), ld, _p(s["p8"]), h8 * h8 * ldp, 1, h8 * ldp, ldp, N, h8, h8, C, 1, 1, st)
        L.call("ydl_resize_fwd", L.YDL_F32, L.RESIZE_BILINEAR, _p(s["p8"]), ldp, _p(s["y8"]), ldp, N, h8, h8, S, S, C, 0.0, 0.0, st)
        L.call("ydl_nhwc_to_nchw", L.YDL_F32, _p(s["y8"]), ldp, _p(s["p"]), N, C, S, S, 0, st)

    def new_v8(s):
        L.call("ydl_softmax_resize_labels", dt, _p(s["x8"]), ld, N, C, h8, h8, S, S, _p(s["labels"]), S * S, S, st)

    def render(mode):
        def fn(s):
            L.call("ydl_labels_render", mode, _p(s["labels"]), _p(s["labels"]), _p(s["img"]), _p(pal), C, _p(s["rgb"]), N, S, S, 0, st)
        return fn

    def unletterbox(s):
        L.call("ydl_labels_resize", _p(s["labels"]), S * S, S, N, S // 8, 0, S * 3 // 4, S, _p(s["un"]), 720 * 960, 960, 720, 960, st)

    def bincount(s):
        L.call("ydl_label_bincount", _p(s["t"]), 1, N * S * S, C, _p(s["counts"]), st)

    px, px8 = N * S * S, N * h8 * h8
    groups = [
        ("parent tail", parent_tail, N * h * h * ld * es + 2 * px * C * 4 + px * 8),
        ("new tail", new_tail, N * h * h * ld * es + 2 * px + px * 8),
        ("parent v8 exit", parent_v8, px8 * ld * es + 2 * px8 * ldp * 4 + 2 * px * ldp * 4 + px * C * 4),
        ("new v8 exit", new_v8, px8 * ld * es + px),
        ("render colour", render(0), px * 4),
        ("render difference", render(1), px * 5),
        ("render overlay", render(2), px * 16),
        ("un-letterbox", unletterbox, N * (S * 3 // 4) * S + N * 720 * 960),
        ("bincount int64", bincount, px * 8),
    ]
    # same results first (and every set holds labels before a render group meets it)
    for s in sets:
        parent_tail(s)
        new_tail(s)
        torch.cuda.synchronize()
        assert torch.equal(s["m_old"], s["m_new"]), "the two tails disagree on the confusion matrix"
        assert int(s["m_new"].sum()) > 0
        lab = s["labels"].clone()
        parent_v8(s)
        new_v8(s)
        torch.cuda.synchronize()
        same = float((s["labels"].long() == s["p"].argmax(1)).float().mean())
        assert same == 1.0, f"v8 exit: {same:.6f} of the labels equal the argmax of the three-launch result"
        s["labels"].copy_(lab)
    times = {n: [] for n, _, _ in groups}
    head = torch.empty(1 << 28, device=dev)
    for it in range(a.warmup + a.rounds):
        head.zero_()
        evs = []
        order = groups if it % 2 == 0 else groups[::-1]            # neither side always runs first
        for j, (name, fn, _) in enumerate(order):
            s = sets[(it + j) % a.rotate]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(s)
            e1.record()
            evs.append((name, e0, e1))
        torch.cuda.synchronize()
        if it >= a.warmup:
            for name, e0, e1 in evs:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    lines = [f"predict_bench: N={N} stored {h}x{h} rep {r}x{r} -> {S}x{S}, C={C}, bf16 scores, int64 targets; v8 exit {h8}^2 -> {S}^2; "
             f"{a.rounds} rounds over {a.rotate} operand sets, us per group (events around the group's launches)"]
    med = {}
    for name, _, nbytes in groups:
        v = times[name]
        med[name] = statistics.median(v)
        tbs = nbytes / (med[name] * 1e-6) / 1e12
        lines.append(f"  {name:18s} median {med[name]:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}   moves {nbytes / 1e6:7.1f} MB = "
                     f"{nbytes / 1e6 / COPY_TBS:6.1f} us at copy rate; {tbs:.2f} TB/s = {100 * tbs / COPY_TBS:.0f} % of copy rate")
    ok = True
    for old, new in (("parent tail", "new tail"), ("parent v8 exit", "new v8 exit")):
        spread = (max(times[old]) - min(times[old])) + (max(times[new]) - min(times[new]))
        gain = med[old] - med[new]
        bytes_ratio = [b for n, _, b in groups if n == old][0] / [b for n, _, b in groups if n == new][0]
        lines.append(f"  {old} / {new}: time {med[old] / med[new]:.2f}x (bytes {bytes_ratio:.2f}x); median gain {gain:.1f} us against a "
                     f"spread of {spread:.1f} us: {'faster by more than the spread' if gain > spread else 'NOT separated from the spread'}")
        ok = ok and gain > spread
    out = "\n".join(lines)
    print(out)
    if a.log:
        with open(a.log, "w") as f:
            f.write(out + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
