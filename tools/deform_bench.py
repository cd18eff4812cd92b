#!/usr/bin/env python3
"""Deformable-convolution kernels on one MI355X: per-layer time of ydl_deform_gather and ydl_deform_bwd at the C3_DCN layer
shapes of config 2 (640^2, bs 16) and config 4 (1024^2, bs 8), offsets N(0, sigma^2) px, bf16 and f32, each beside its byte floor
(algorithmic bytes / 6.3 TB/s); the share of grad_input adds the window backward sends to global atomics (counted on the host
from the same offsets); and the whole training step of config 2 with native C3_DCN blocks against the substituted C3 model
through ReplayedTrainStep.

    python tools/deform_bench.py [--quick] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
LAYERS = {"cfg2": (16, [(128, 80), (256, 40), (512, 20)]), "cfg4": (8, [(128, 128), (256, 64), (512, 32)])}


def _time(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3       # us


def global_share(off, H, W, C):
    """fraction of grad_input f32 adds of deform_bwd_window_kernel that go to global memory (out-of-window corners + window
    flush, one add per non-zero in-image cell and channel) for 3x3 / s1 / p1 offsets off [N, H, W, 18] (f32, host)"""
    import torch
    N = off.shape[0]
    T, R = 8, 2
    E = T + 2 + 2 * R
    ho = torch.arange(H).view(1, H, 1, 1)
    wo = torch.arange(W).view(1, 1, W, 1)
    k = torch.arange(9)
    y = ho - 1 + (k // 3).view(1, 1, 1, 9) + off[..., 0::2]
    x = wo - 1 + (k % 3).view(1, 1, 1, 9) + off[..., 1::2]
    h0, w0 = torch.floor(y).long(), torch.floor(x).long()
    wh0 = (ho // T) * T - 1 - R
    ww0 = (wo // T) * T - 1 - R
    tid = ((torch.arange(N).view(N, 1, 1, 1) * ((H + T - 1) // T) + ho // T) * ((W + T - 1) // T) + wo // T).expand_as(h0)
    total = out = 0
    keys = []
    for dy in (0, 1):
        for dx in (0, 1):
            h, w = h0 + dy, w0 + dx
            valid = (h >= 0) & (h < H) & (w >= 0) & (w < W)
            inside = (h - wh0 >= 0) & (h - wh0 < E) & (w - ww0 >= 0) & (w - ww0 < E)
            total += int(valid.sum())
            out += int((valid & ~inside).sum())
            sel = valid & inside
            keys.append(tid[sel] * (H * W) + h[sel] * W + w[sel])
    flush = int(torch.cat(keys).unique().numel())         # window cells that received an add: one flush atomic each
    return (out + flush) / max(total, 1), out / max(total, 1), flush / max(total, 1)


def layer_rows(dtypes, sigmas, reps):
    import torch
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.tape import _p, _stream, round_up
    rows = []
    for cfg, (N, layers) in LAYERS.items():
        for C, H in layers:
            for dname in dtypes:
                tdt = torch.bfloat16 if dname == "bf16" else torch.float32
                dt = L.YDL_BF16 if dname == "bf16" else L.YDL_F32
                es = 2 if dname == "bf16" else 4
                x = torch.randn(N, H, H, C, device="cuda").to(tdt)
                ldc = round_up(9 * C, 8)
                col = torch.empty(N * H * H, ldc, dtype=tdt, device="cuda")
                gin = torch.zeros(N, H, H, C, device="cuda")
                goff = torch.empty(N * H * H, 18, device="cuda")
                for sg in sigmas:
                    off = torch.zeros(N, H, H, 24, device="cuda")
                    off[..., :18] = sg * torch.randn(N, H, H, 18, device="cuda")
                    off = off.to(tdt)
                    geo = (N, H, H, C, H, H, 3, 3, 1, 1, 1, 1, 1, 1, 1)
                    fg = lambda: L.call("ydl_deform_gather", dt, _p(x), C, _p(off), 24, None, 0, 0, _p(col), ldc, 0, *geo, _stream())
                    bw = lambda: L.call("ydl_deform_bwd", dt, _p(x), C, _p(off), 24, None, 0, 0, _p(col), ldc, _p(gin), _p(goff), None,
                                        *geo, _stream())
                    t_f = _time(fg, reps)
                    t_b = _time(bw, reps)
                    kname = L.last_kernel(4)
                    npix = N * H * H
                    # gather: x once + offsets read, col written; backward: dcol + x + offsets read, grad_input (f32) read-modify-
                    # written once, grad_offset (f32) written
                    b_f = npix * C * es + npix * 18 * es + npix * 9 * C * es
                    b_b = npix * 9 * C * es + npix * C * es + npix * 18 * es + 2 * npix * C * 4 + npix * 18 * 4
                    row = {"cfg": cfg, "C": C, "HW": H, "N": N, "dtype": dname, "sigma": sg,
                           "gather_us": round(t_f, 1), "gather_MB": round(b_f / 1e6, 1), "gather_floor_us": round(b_f / HBM * 1e6, 1),
                           "gather_frac_of_hbm": round(b_f / HBM * 1e6 / t_f, 3),
                           "bwd_us": round(t_b, 1), "bwd_MB": round(b_b / 1e6, 1), "bwd_floor_us": round(b_b / HBM * 1e6, 1),
                           "bwd_frac_of_hbm": round(b_b / HBM * 1e6 / t_b, 3), "bwd_kernel": kname}
                    if dname == "bf16" and cfg == "cfg2" and C == 128:
                        tot, o, f = global_share(off[..., :18].float().cpu(), H, H, C)
                        row.update(global_share=round(tot, 3), out_of_window=round(o, 4), flush=round(f, 3))
                    print(json.dumps(row), flush=True)
                    rows.append(row)
                del x, col, gin, goff
                torch.cuda.empty_cache()
    return rows


def step_rate(native: bool, steps: int):
    import torch
    import yaml
    import yolo_dual_amd as ydl
    from oracle.fill import fill_state_dict
    from yolo_dual_amd.replay import ReplayedTrainStep
    ydl.set_compute_dtype("bf16")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "yolo_dual_amd", "cfg", "yolov5_seg.yaml")))
    if not native:
        for sec in ("backbone", "head"):
            for l in cfg[sec]:
                l[2] = {"C3_DCN": "C3"}.get(l[2], l[2])
    m = ydl.YOLOv5Seg(cfg, deformable=native)
    sd = m.state_dict()
    fill_state_dict(sd, 1, bn_stats=False)
    m.load_state_dict(sd)
    m.img_size = [640, 640]
    m = m.cuda().train()
    crit = ydl.SegmentationLoss(12, 0.0, torch.ones(12), "dice", sync=False)
    opt = ydl.FlatSGDEMA(m, lr=0.01, momentum=0.937, weight_decay=5e-4 * 16 / 64.0)
    g = torch.Generator("cuda").manual_seed(0)
    x = torch.rand(16, 3, 640, 640, device="cuda", generator=g)
    t = torch.randint(0, 12, (16, 640, 640), device="cuda", generator=g)
    r = ReplayedTrainStep(m, crit, opt, x, t, warmup=2)
    for _ in range(3):
        r.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        r.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"model": "cfg2 native C3_DCN" if native else "cfg2 substituted C3", "ms_per_step": round(dt * 1e3, 2),
            "images_per_s": round(16 / dt, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="bf16, sigma 0.5 only")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    dtypes = ["bf16"] if a.quick else ["bf16", "f32"]
    sigmas = [0.5] if a.quick else [0.0, 0.5, 2.0]
    res = {"layers": layer_rows(dtypes, sigmas, a.reps)}
    if not a.no_step:
        res["step"] = [step_rate(False, a.steps), step_rate(True, a.steps)]
        print(json.dumps(res["step"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
