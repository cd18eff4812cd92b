"""CPU: the forward statistics-workspace queries of the C ABI (ydl_conv_fwd_grid_m / _block_m / _stats_ws_bytes, include/ydl.h) over
thousands of geometries, both compute dtypes, loader waves on and off.  The queries are host-only: they must agree with the launch the
dispatcher would make, so these invariants need no GPU.  The launch side of the same contract is checked on the device by
tests/test_gpu_bn_statistics.py."""
import ctypes
import os

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the spatial sizes a conv layer sees in the benchmark (640 x 640 input at batch 16: the stride-2 stem to the 32x stage)
BENCH_N, BENCH_SIZES = 16, (320, 160, 80, 40, 20)


def _lib():
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.build import build
    build(verbose=False)
    return L


def _model_layers():
    """(c1, c2, k) of every conv layer of the three model families (tests/model_shapes.py)"""
    from tests.model_shapes import resnet50_yaml_state_shapes, script_model_state_shapes
    cfgdir = os.path.join(ROOT, "yolo_dual_amd", "cfg")
    tables = []
    for name in ("yolov5_seg.yaml", "yolov8_seg.yaml"):
        cfg = yaml.safe_load(open(os.path.join(cfgdir, name)))
        for sec in ("backbone", "head"):
            for l in cfg[sec]:
                l[2] = {"C3_DCN": "C3", "C2f_DCN": "C2f"}.get(l[2], l[2])     # (the substituted blocks of the default build)
        tables.append(script_model_state_shapes(cfg))
    tables.append(resnet50_yaml_state_shapes(yaml.safe_load(open(os.path.join(cfgdir, "resnet50_seg.yaml"))))[0])
    out = set()
    for sh in tables:
        for key, shape in sh.items():
            if key.endswith("conv.weight") and len(shape) == 4 and shape[2] == shape[3]:
                c2, c1, k, _ = shape
                out.add((c1, c2, k))
    return sorted(out)


def _geom(L, N, H, W, c1, c2, k, s, ldy=None, ldw=0):
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    cp = (c1 + 7) // 8 * 8
    return L.ConvGeom(N, H, W, c1, Ho, Wo, c2, k, s, p, cp, ldy if ldy is not None else (c2 + 7) // 8 * 8, ldw)


def _geometries(L):
    gs = []
    for c1, c2, k in _model_layers():
        for H in BENCH_SIZES:
            for s in (1, 2):
                gs.append(_geom(L, BENCH_N, H, H, c1, c2, k, s))
    rs = np.random.RandomState(2024)
    chans = (3, 8, 12, 16, 24, 32, 48, 64, 72, 96, 128, 136, 152, 192, 256, 320, 384, 512, 768, 1024)
    for _ in range(2500):
        k = int(rs.choice((1, 1, 3, 3, 3, 5)))
        s = int(rs.choice((1, 1, 2)))
        c1, c2 = int(rs.choice(chans)), int(rs.choice(chans + (10, 150, 255)))
        N = int(rs.choice((1, 2, 3, 4, 8, 16)))
        if rs.rand() < 0.5:          # patch-friendly maps (multiples of 8 x 16) half of the time
            H, W = 8 * int(rs.randint(1, 41)), 16 * int(rs.randint(1, 21))
        else:
            H, W = int(rs.randint(3, 330)), int(rs.randint(3, 330))
        ldy = (c2 + 7) // 8 * 8 + 8 * int(rs.choice((0, 0, 0, 1, 16)))
        ldw = 0
        if k == 1 and rs.rand() < 0.2:   # a column block of a wider 1x1 weight matrix (the commuted concat)
            ldw = (c1 + 7) // 8 * 8 + 8 * int(rs.randint(1, 64))
        gs.append(_geom(L, N, H, W, c1, c2, k, s, ldy=ldy, ldw=ldw))
    # the thin-input stem (16-channel stride) at the benchmark's first map and a few others
    for N, H, W in ((16, 320, 320), (4, 320, 320), (13, 50, 128), (2, 48, 64), (1, 40, 48)):
        gs.append(L.ConvGeom(N, H, W, 12, H, W, 64, 3, 1, 1, 16, 64, 0))
    return gs


def _patch_form(g, dtype):
    """the patch-kernel conditions (igemm.hip halo_ok, reached from the ring dispatch): bf16 3x3 / stride 1 / pad 1, map a multiple of
    8 x 16, K rows of whole 64-channel blocks, >= 64 stored output channels"""
    return (dtype == 1 and g.k == 3 and g.s == 1 and g.p == 1 and g.Ho % 8 == 0 and g.Wo % 16 == 0 and g.Cin % 64 == 0
            and g.Cout >= 64 and g.Cout % 8 == 0 and g.ldx == g.Cin)


@pytest.mark.parametrize("loaders", [1, 0])
def test_forward_statistics_queries_describe_a_launch(loaders):
    L = _lib()
    lib = L.lib()
    geoms = _geometries(L)
    assert len(geoms) > 2500
    L.debug_set(19, loaders)
    try:
        checked = patch = 0
        for g in geoms:
            for dtype in (L.YDL_F32, L.YDL_BF16):
                gp = ctypes.byref(g)
                gm, bm = lib.ydl_conv_fwd_grid_m(gp, dtype), lib.ydl_conv_fwd_block_m(gp, dtype)
                ws = lib.ydl_conv_fwd_stats_ws_bytes(gp, dtype)
                M = g.N * g.Ho * g.Wo
                tag = ([getattr(g, f) for f, _ in L.ConvGeom._fields_], dtype, gm, bm, ws)
                if g.N * g.Hi * g.Wi * g.ldx * (4 if dtype == L.YDL_F32 else 2) >= 0xFFFFFFF0:
                    assert gm == bm == ws == 0, tag          # refused (32-bit buffer addressing): the queries say so
                    continue
                assert gm >= 1 and bm >= 1, tag
                # every pixel in exactly one row; no empty row
                assert gm * bm >= M > (gm - 1) * bm, tag
                # the rows plus ydl_bn_finalize's level-1 rows (one per 64 rows) fit the workspace
                cp = (g.Cout + 7) // 8 * 8
                assert ws >= (gm + (gm + 63) // 64) * 2 * cp * 4, tag
                # a pixel-tile height some launch path uses: ring / register-staged tiles, the point-wise kernel's 16-pixel steps,
                # the stem kernel's 64-pixel segments
                stem = dtype == 1 and g.k == 3 and g.Cin == 12 and g.ldx == 16 and g.Cout == 64
                assert bm in (64, 128, 256) or (g.k == 1 and bm % 16 == 0) or (stem and bm % 64 == 0), tag
                if _patch_form(g, dtype):
                    patch += 1
                    # the patch kernels write one row per 8 x 16 patch; the only other ring tile such a map can get with partial
                    # rows is the 64 x 128 one of small grids (fewer than 256 tiles of 128 x 128)
                    assert bm in (64, 128), tag
                    if g.Cout < 128 or ((M + 127) // 128) * ((g.Cout + 127) // 128) >= 256:
                        assert bm == 128, tag
                checked += 1
        assert patch > 100, patch
    finally:
        L.debug_set(19, -1)


def test_benchmark_layers_on_the_patch_kernel_report_its_rows():
    """the 3x3 layers of the 160 x 160 stage at batch 4 / 16 (ring ids 15 and 24 with 256-pixel tiles, then the patch kernel with
    128-pixel patches: the shapes where the queries once reported the ring tile)"""
    L = _lib()
    lib = L.lib()
    for loaders in (1, 0):
        L.debug_set(19, loaders)
        try:
            for N, c in ((4, 128), (16, 128), (16, 256)):
                g = _geom(L, N, 160, 160, c, c, 3, 1)
                M = N * 160 * 160
                assert lib.ydl_conv_fwd_block_m(ctypes.byref(g), L.YDL_BF16) == 128, (N, c, loaders)
                assert lib.ydl_conv_fwd_grid_m(ctypes.byref(g), L.YDL_BF16) == M // 128, (N, c, loaders)
        finally:
            L.debug_set(19, -1)


def test_queries_of_a_bad_geometry_are_zero():
    L = _lib()
    g = L.ConvGeom(1, 8, 8, 8, 9, 9, 8, 3, 1, 1, 8, 8, 0)     # wrong Ho / Wo
    assert L.lib().ydl_conv_fwd_grid_m(ctypes.byref(g), L.YDL_BF16) == 0
    assert L.lib().ydl_conv_fwd_stats_ws_bytes(ctypes.byref(g), L.YDL_BF16) == 0
