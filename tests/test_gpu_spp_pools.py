"""GPU: the one-launch parallel pooling pyramid (ydl_spp_pool_fwd / _bwd, csrc/spp.hip) through the C ABI against the route it
replaces, three ydl_maxpool_fwd(x -> yi, ki, 1, ki / 2) calls and ydl_maxpool_bwd(dy1, idx1, accumulate), (dy2, idx2, 1), (dy3, idx3, 1):
y1..3, idx1..3 and dx bit for bit, in f32 and bf16, accumulate 0 and 1, twice with the same bits.

* planes: 20 x 20 (two passes of the 256 threads over it), 9 x 7 with 12 channels (C % 8 != 0: what lies beyond the padded channel
  count stays unwritten), 1 x 1, 3 x 20, and one case with x, y and dx as channel slices of wider buffers (ld 40 and 72);
* window sizes (5, 9, 13) and (3, 7, 15): every window overhangs the small planes;
* integer-valued data (x in [-3, 3], dy in {-1, 0, 1}): ties everywhere, every sum exact, so in f32 y and dx also equal
  tests/spp_ref.py (pinned to ATen by tests/test_spp_ref_cpu.py) exactly; a random-normal case; a NaN-bearing input;
* ydl_spp_pool_supported is 0 for an even k, for k > 15 and for a plane too large for LDS, where the launchers return an error."""
import ctypes

import numpy as np
import pytest
import torch

from tests import spp_ref

pytestmark = pytest.mark.gpu

# name -> (N, C, H, W, ld of the x / dx buffers, their channel offset, ld of the y / dy buffer, channel offsets of the three slices)
CASES = {
    "2x16x20x20": (2, 16, 20, 20, 16, 0, 48, (0, 16, 32)),
    "2x12x9x7": (2, 12, 9, 7, 16, 0, 48, (0, 16, 32)),
    "1x8x1x1": (1, 8, 1, 1, 8, 0, 24, (0, 8, 16)),
    "1x8x3x20": (1, 8, 3, 20, 8, 0, 24, (0, 8, 16)),
    "slices_2x16x9x7": (2, 16, 9, 7, 40, 8, 72, (16, 32, 48)),
}


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _draw(kind, case, tdt, seed):
    """(x buffer, dy buffer, dx buffer) in NHWC with the case's row lengths; what lies outside the slices is a sentinel"""
    N, C, H, W, ldx, cx, ldy, cys = CASES[case]
    gen = torch.Generator("cuda").manual_seed(seed)

    def rnd(ld, lo, hi):
        if kind == "int":
            return torch.randint(lo, hi + 1, (N, H, W, ld), device="cuda", generator=gen).to(tdt)
        return torch.randn(N, H, W, ld, device="cuda", generator=gen).to(tdt)
    x, dy, dx = rnd(ldx, -3, 3), rnd(ldy, -1, 1), rnd(ldx, -2, 2)
    if kind == "nan":
        hit = torch.rand(N, H, W, ldx, device="cuda", generator=gen) < 0.1
        x[hit] = float("nan")
    return x, dy, dx


def _run(fused, dt, tdt, case, ks, x, dy, dx0, acc):
    from yolo_dual_amd import _lib as L
    N, C, H, W, ldx, cx, ldy, cys = CASES[case]
    es = x.element_size()
    Cp = -(-C // (16 // es)) * (16 // es)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, c=0: ctypes.c_void_p(t.data_ptr() + c * es)
    y = torch.full((N, H, W, ldy), 77.0, device="cuda", dtype=tdt)
    idx = [torch.full((N * H * W * Cp,), 255, device="cuda", dtype=torch.uint8) for _ in ks]
    dx = dx0.clone()
    if fused:
        L.call("ydl_spp_pool_fwd", dt, P(x, cx), ldx, P(y, cys[0]), P(y, cys[1]), P(y, cys[2]), ldy, P(idx[0]), P(idx[1]), P(idx[2]),
               N, H, W, C, *ks, st)
        L.call("ydl_spp_pool_bwd", dt, P(dy, cys[0]), P(dy, cys[1]), P(dy, cys[2]), ldy, P(idx[0]), P(idx[1]), P(idx[2]),
               P(dx, cx), ldx, acc, N, H, W, C, *ks, st)
    else:
        for i, k in enumerate(ks):
            L.call("ydl_maxpool_fwd", dt, P(x, cx), ldx, P(y, cys[i]), ldy, P(idx[i]), N, H, W, H, W, C, k, 1, k // 2, st)
        for i, k in enumerate(ks):
            L.call("ydl_maxpool_bwd", dt, P(dy, cys[i]), ldy, P(idx[i]), P(dx, cx), ldx, acc if i == 0 else 1,
                   N, H, W, H, W, C, k, 1, k // 2, st)
    torch.cuda.synchronize()
    return y, idx, dx


def _compare(a, b):
    (ya, ia, da), (yb, ib, db) = a, b
    assert torch.equal(_bits(ya), _bits(yb))
    for u, v in zip(ia, ib):
        assert torch.equal(u, v)
    assert torch.equal(_bits(da), _bits(db))


@pytest.mark.parametrize("ks", [(5, 9, 13), (3, 7, 15)], ids=lambda k: "k" + "_".join(map(str, k)))
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_launch_equals_three_pools_on_tied_data(dtype, case, ks):
    from yolo_dual_amd import _lib as L
    tdt, dt = (torch.bfloat16, L.YDL_BF16) if dtype == "bf16" else (torch.float32, L.YDL_F32)
    N, C, H, W, ldx, cx, ldy, cys = CASES[case]
    assert L.lib().ydl_spp_pool_supported(dt, H, W, C, *ks) == 1
    x, dy, dx0 = _draw("int", case, tdt, 7)
    V = 16 // x.element_size()
    Cp = -(-C // V) * V
    nchw = lambda t, c: t[..., c:c + C].permute(0, 3, 1, 2).double().cpu().numpy()
    if dtype == "f32":                                                        # exact data: the float64 statement, to the bit
        ref = spp_ref.spp_fwd(nchw(x, cx), ks)
        dref = spp_ref.spp_bwd([nchw(dy, c) for c in cys], [c for _y, c in ref], ks)
    for acc in (0, 1):
        got = _run(True, dt, tdt, case, ks, x, dy, dx0, acc)
        _compare(got, _run(False, dt, tdt, case, ks, x, dy, dx0, acc))
        _compare(got, _run(True, dt, tdt, case, ks, x, dy, dx0, acc))           # twice: the same bits
        y, idx, dx = got
        # nothing outside the slices' padded channels is written
        keep = torch.ones(ldy, dtype=torch.bool, device="cuda")
        for c in cys:
            keep[c:c + Cp] = False
        assert bool((y[..., keep] == 77.0).all())
        keep = torch.ones(ldx, dtype=torch.bool, device="cuda")
        keep[cx:cx + Cp] = False
        assert torch.equal(dx[..., keep], dx0[..., keep])
        if dtype == "f32":
            for c, (yr, _cr) in zip(cys, ref):
                assert np.array_equal(nchw(y, c), yr)
            assert np.array_equal(nchw(dx, cx), dref + nchw(dx0, cx) if acc else dref)      # integers: the order of the sum is free


@pytest.mark.parametrize("kind", ["normal", "nan"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_launch_equals_three_pools_on_random_and_nan_data(dtype, kind):
    from yolo_dual_amd import _lib as L
    tdt, dt = (torch.bfloat16, L.YDL_BF16) if dtype == "bf16" else (torch.float32, L.YDL_F32)
    case, ks = "2x16x20x20", (13, 5, 9)                                       # any order
    x, dy, dx0 = _draw(kind, case, tdt, 11)
    for acc in (0, 1):
        got = _run(True, dt, tdt, case, ks, x, dy, dx0, acc)
        _compare(got, _run(False, dt, tdt, case, ks, x, dy, dx0, acc))
    if kind == "nan":                                                         # a window that holds a NaN yields NaN, no other does
        y = got[0]
        xn = torch.isnan(x).permute(0, 3, 1, 2).float()
        for i, k in enumerate(ks):
            want = torch.nn.functional.max_pool2d(xn, k, 1, k // 2) > 0
            assert torch.equal(torch.isnan(y[..., 16 * i:16 * i + 16]).permute(0, 3, 1, 2), want)


def test_supported_answers_from_the_window_sizes_and_the_lds_footprint():
    from yolo_dual_amd import _lib as L
    lib = L.lib()
    for dt in (L.YDL_F32, L.YDL_BF16):
        assert lib.ydl_spp_pool_supported(dt, 20, 20, 256, 5, 9, 13) == 1
        assert lib.ydl_spp_pool_supported(dt, 20, 20, 256, 15, 3, 7) == 1
        for ks in ((4, 9, 13), (5, 9, 17), (5, 16, 13), (1, 5, 9), (5, 9, -3)):
            assert lib.ydl_spp_pool_supported(dt, 20, 20, 256, *ks) == 0, ks
        size = 8
        while size <= 1024 and lib.ydl_spp_pool_supported(dt, size, size, 8, 5, 9, 13):
            size *= 2
        assert size <= 1024, "a 1024 x 1024 plane cannot fit LDS"
        # there the launchers refuse before anything is launched (no buffers are handed over)
        null = ctypes.c_void_p(0)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.ydl_spp_pool_fwd(dt, null, 8, null, null, null, 8, null, null, null, 1, size, size, 8, 5, 9, 13, st)
        assert rc != 0 and b"ydl_spp_pool_supported" in lib.ydl_last_error()
        rc = lib.ydl_spp_pool_bwd(dt, null, null, null, 8, null, null, null, null, 8, 0, 1, size, size, 8, 5, 9, 13, st)
        assert rc != 0 and b"ydl_spp_pool_supported" in lib.ydl_last_error()
        rc = lib.ydl_spp_pool_fwd(dt, null, 8, null, null, null, 8, null, null, null, 1, 20, 20, 8, 4, 9, 13, st)
        assert rc != 0 and b"ydl_spp_pool_supported" in lib.ydl_last_error()


@pytest.mark.parametrize("live", [(0, 1, 2), (1,), (0, 2)], ids=lambda v: "live" + "".join(map(str, v)))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_tape_routes_a_pyramid_whose_slices_are_not_all_consumed(dtype, live):
    """Tape.spp_pools inside a region whose output is the concat of some of the three pooled slices: with all three the backward
    is the one launch, with a dead slice it runs pool by pool through ydl_maxpool_bwd on the index planes of the one-launch
    forward.  Integer data: output and input gradient equal ATen's exactly, in either dtype."""
    import torch.nn.functional as F
    import yolo_dual_amd as ydl
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.modules import YdlModule
    ks, C = (5, 9, 13), 16
    calls = []

    class Pyramid(YdlModule):
        def _fwd(self, tape, x):
            cat = tape.new(x.N, 3 * C, x.H, x.W)
            outs = tape.spp_pools(x, ks, [cat.slice(i * C, (i + 1) * C) for i in range(3)])
            return tape.concat([outs[i] for i in live])          # a buffer of its own: the region's output is never a slice

    ydl.set_compute_dtype(dtype)
    real_call = L.call
    try:
        L.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
        gen = torch.Generator("cuda").manual_seed(2)
        x = torch.randint(-3, 4, (2, C, 9, 7), device="cuda", generator=gen).float().requires_grad_(True)
        g = torch.randint(-1, 2, (2, len(live) * C, 9, 7), device="cuda", generator=gen).float()
        out = Pyramid().cuda().train()(x)
        out.backward(g)
        torch.cuda.synchronize()
    finally:
        L.call = real_call
        ydl.set_compute_dtype("bf16")
    xr = x.detach().double().requires_grad_(True)
    ref = torch.cat([F.max_pool2d(xr, ks[i], 1, ks[i] // 2) for i in live], 1)
    ref.backward(g.double())
    assert torch.equal(out.detach().double(), ref.detach()) and torch.equal(x.grad.double(), xr.grad)
    assert calls.count("ydl_spp_pool_fwd") == 1 and "ydl_maxpool_fwd" not in calls
    if len(live) == 3:
        assert calls.count("ydl_spp_pool_bwd") == 1 and "ydl_maxpool_bwd" not in calls
    else:
        assert calls.count("ydl_maxpool_bwd") == len(live) and "ydl_spp_pool_bwd" not in calls
