#!/usr/bin/env python3
"""Per-kernel A/B of the replicated prediction tail at the bench shape (16 x 160^2 stored pixels, 12 classes, rep 4 x 4, bf16):
the unfused launches (ydl_softmax_fwd at the stored resolution, ydl_seg_loss_rep_fwd | ydl_seg_loss_rep_bwd, ydl_softmax_bwd) against
the fused pair (ydl_seg_tail_fwd | ydl_seg_tail_bwd).  The four groups alternate within every round and every round takes the next of
--rotate operand sets (together far larger than the 256 MB Infinity Cache), so neither side is served from cache.  Event timing of a
group includes its launch gaps; the forward groups include the two merge launches.  Byte floors: forward = logits + labels + counts
(72 MB at the default shape), backward = logits + counts + dx (33 MB), against the 6.29 TB/s of a plain copy.

    python tools/seg_tail_bench.py [--rounds 40] [--rotate 8] [--log profiles/seg_tail_bench.log]"""
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
    ap.add_argument("--size", type=int, default=160, help="stored height = width")
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--rep", type=int, default=4)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=8)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    dev = "cuda"
    N, C, h, r = a.bs, a.classes, a.size, a.rep
    w, ld = h, (C + 7) // 8 * 8
    tdt, dt = (torch.bfloat16, L.YDL_BF16) if a.dtype == "bf16" else (torch.float32, L.YDL_F32)
    es = 2 if a.dtype == "bf16" else 4
    nws = L.lib().ydl_seg_loss_ws_floats(N, C)
    nb = L.lib().ydl_seg_tail_count_bytes(N, C, h, w, r, r)
    cw = torch.tensor([1, 2, 25, 2, 10, 3, 25, 10, 5, 15, 25, 1], dtype=torch.float32, device=dev)[:C].contiguous() if C <= 12 else None
    g = torch.ones(1, device=dev)
    sets = []
    for _ in range(a.rotate):
        sets.append(dict(
            x=(torch.randn(N, h, w, ld, device=dev) * 3).to(tdt), t=torch.randint(0, C, (N, h * r, w * r), device=dev),
            plow=torch.empty(N, C, h, w, device=dev), dlow=torch.empty(N, C, h, w, device=dev),
            dx=torch.empty(N, h, w, ld, device=dev, dtype=tdt), counts=torch.empty(max(nb, 16), dtype=torch.uint8, device=dev),
            ws=torch.empty(nws, device=dev), losses=torch.empty(3, device=dev)))
    st = _stream()
    k, ls, eps = L.LOSS_DICE, 0.0, 1e-6

    def unfused_fwd(s):
        ps = s["plow"].stride()
        L.call("ydl_softmax_fwd", dt, _p(s["x"]), ld, _p(s["plow"]), *ps, N, h, w, C, 1, 1, st)
        L.call("ydl_seg_loss_rep_fwd", _p(s["plow"]), *ps, _p(s["t"]), _p(cw), k, ls, eps, N, C, h, w, r, r, _p(s["ws"]), _p(s["losses"]), st)

    def unfused_bwd(s):
        ps = s["plow"].stride()
        L.call("ydl_seg_loss_rep_bwd", _p(s["plow"]), *ps, _p(s["t"]), _p(cw), k, ls, eps, N, C, h, w, r, r, _p(s["ws"]), _p(g),
               _p(s["dlow"]), st)
        L.call("ydl_softmax_bwd", dt, _p(s["plow"]), _p(s["dlow"]), *ps, _p(s["dx"]), ld, N, h, w, C, 1, 1, st)

    def fused_fwd(s):
        L.call("ydl_seg_tail_fwd", dt, _p(s["x"]), ld, _p(s["t"]), _p(cw), k, ls, eps, N, C, h, w, r, r, _p(s["ws"]), _p(s["losses"]),
               _p(s["counts"]), st)

    def fused_bwd(s):
        L.call("ydl_seg_tail_bwd", dt, _p(s["x"]), ld, _p(s["counts"]), _p(s["t"]), _p(cw), ls, N, C, h, w, r, r, _p(s["ws"]), _p(g),
               _p(s["dx"]), ld, st)

    groups = [("unfused fwd", unfused_fwd), ("fused fwd", fused_fwd), ("unfused bwd", unfused_bwd), ("fused bwd", fused_bwd)]
    times = {n: [] for n, _ in groups}
    for s in sets:                  # every set holds probabilities, counts and merged sums before a backward group meets it
        unfused_fwd(s)
        fused_fwd(s)
    head = torch.empty(1 << 28, device=dev)       # 1 GiB fill in front of every round: the host gets ahead of the GPU (no launch
    for it in range(a.warmup + a.rounds):         # latency inside the event pairs) and the cache holds none of the operands
        head.zero_()
        evs = []
        for j, (name, fn) in enumerate(groups):
            s = sets[(it * len(groups) + j) % a.rotate]     # a group never meets the set its neighbour has just pulled into the cache
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(s)
            e1.record()
            evs.append((name, e0, e1))
        torch.cuda.synchronize()
        if it >= a.warmup:
            for name, e0, e1 in evs:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    npix = N * h * w
    floors = {"fused fwd": npix * ld * es + npix * r * r * 8 + nb, "fused bwd": npix * ld * es * 2 + nb}
    lines = [f"seg_tail_bench: N={N} stored {h}x{w} C={C} rep {r}x{r} {a.dtype}, {a.rounds} rounds over {a.rotate} operand sets, us per group"]
    for name, _ in groups:
        v = times[name]
        line = f"  {name:12s} median {statistics.median(v):7.1f}  min {min(v):7.1f}  max {max(v):7.1f}"
        if name in floors:
            mb = floors[name] / 1e6
            tbs = floors[name] / (statistics.median(v) * 1e-6) / 1e12
            line += f"   byte floor {mb:.1f} MB = {mb / COPY_TBS:.1f} us at copy rate; {tbs:.2f} TB/s = {100 * tbs / COPY_TBS:.0f} % of copy rate"
        lines.append(line)
    for d in ("fwd", "bwd"):
        lines.append(f"  {d}: fused / unfused = {statistics.median(times['fused ' + d]) / statistics.median(times['unfused ' + d]):.2f}")
    out = "\n".join(lines)
    print(out)
    if a.log:
        with open(a.log, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
