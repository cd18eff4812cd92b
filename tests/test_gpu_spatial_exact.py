"""The kernels of csrc/spatial.hip and the transport helpers of csrc/dcn_blocks.hip whose result is exact, through the C ABI, to the bit
against tests/spatial_ref.py: max pool (values, arg-max codes, backward), nearest resize, ydl_copy2d (vector and scalar path), the
layout conversions, the zero fills, the casts, the chunk reduction, the global max / arg-max and the global pool backward; the second
trip of every grid-stride loop; the refusals of the entry points (nothing launched).  Where a kernel adds, the data are small integers,
so every sum is exact in the storage type.  Every output is a view inside a buffer of sentinels: rows of ld == Cp, and rows two chunks
wider with the view one chunk in (an offset of 16 bytes); everything outside the documented output keeps the sentinel.  Pad channels
[C, Cp) of an input hold 77 and are asserted only where include/ydl.h documents them (zeros after ydl_nchw_to_nhwc, ydl_nchw_to_s2d
and ydl_scale_channels; merely written by the others).

The rounded kernels of the same files are in tests/test_gpu_spatial_f64.py; the measured figures of both modules are recorded there.
97 tests; with the 128 of the other module 7 s on one MI355X; the slowest 0.6 s (the 513 x 512 max pool, most of it the numpy reference).  On the commit before this
module test_global_max_of_a_plane_with_nan fails (the merge of global_pool_fwd_kernel dropped the NaN) and the misaligned calls of
test_refusals_of_misaligned_vector_operands were not refused: that test must never be run against a library without the checks."""
import ctypes

import numpy as np
import pytest
import torch

from tests import spatial_ref as R
from tests import spatial_gpu as G

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = ["f32", "bf16"]
CS = {"f32": (4, 12), "bf16": (8, 20)}
POOLS = [(2, 2, 0), (3, 2, 1), (5, 1, 2), (3, 1, 1)]
POOL_CASES = [(k, s, p, H, W) for (k, s, p) in POOLS for (H, W) in [(7, 9), (1, 5), (12, 12)] if R.pool_out(H, k, s, p) >= 1]   # 2x2 / 2 has no 1 x 5 output
NEAREST = [(4, 4, 8, 8, 0.0), (5, 6, 17, 11, 0.0), (40, 40, 20, 20, 0.0), (3, 300, 7, 33, 0.0), (10, 12, 20, 24, 1 / 2.05)]


def rng(seed):
    return np.random.RandomState(seed)


def ints(seed, shape, lo, hi):
    return rng(seed).randint(lo, hi + 1, size=shape).astype(F64)


def exact(what, buf, ref, sent=R.SENT):
    res = R.check_exact(buf.host(), dict(layout=buf.lay, ref=ref, sent=sent))
    assert R.accepted(res), (what, f"{int(res[0])} elements differ from the reference or from the sentinel")


# ---------------------------------------------------------------------------------------------------------------------------
# max pool
# ---------------------------------------------------------------------------------------------------------------------------
def _maxpool(dtype, k, s, p, N, H, W, C, wide, seed=0):
    d, tdt, es, V = G.dt(dtype)
    Cp = R.rup(C, V)
    x = ints(seed + k, (N, H, W, C), -3, 3)
    y, code = R.maxpool_ref(x, k, s, p)
    Ho, Wo = y.shape[1:3]
    xb = G.Buf(G.slice_layout(N * H * W, C, dtype, wide), tdt, x)
    yb = G.Buf(G.slice_layout(N * Ho * Wo, C, dtype, wide), tdt)
    ib = G.Buf(R.Layout(N * Ho * Wo, Cp, C, Cp), torch.uint8, sent=255)
    G.call("ydl_maxpool_fwd", d, xb.p, xb.lay.ld, yb.p, yb.lay.ld, ib.p, N, H, W, Ho, Wo, C, k, s, p, G.stream())
    G.sync()
    tag = f"maxpool {dtype} k{k} s{s} p{p} {H}x{W} C{C} wide={wide}"
    exact(tag + " values", yb, y)
    exact(tag + " codes", ib, code, 255)
    dy = ints(seed + 1, y.shape, -2, 2)
    prev = ints(seed + 2, x.shape, -4, 4)
    dyb = G.Buf(yb.lay, tdt, dy)
    for acc in (0, 1):
        dxb = G.Buf(xb.lay, tdt, prev) if acc else G.Buf(xb.lay, tdt)
        G.call("ydl_maxpool_bwd", d, dyb.p, dyb.lay.ld, ib.p, dxb.p, dxb.lay.ld, acc, N, H, W, Ho, Wo, C, k, s, p, G.stream())
        G.sync()
        exact(tag + f" backward acc={acc}", dxb, R.maxpool_bwd_ref(dy, code, H, W, k, s, p, prev if acc else None))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,s,p,H,W", POOL_CASES)
def test_max_pool_values_codes_and_backward(dtype, k, s, p, H, W):
    """ydl_maxpool_fwd / ydl_maxpool_bwd at strides 1 and 2, odd and even k, tie-dense data: the first maximum in scan order, its
    code, and the gather by ``nh % s``, ``nh / s`` of the backward, overwrite and accumulate"""
    for C in CS[dtype]:
        for wide in (False, True):
            _maxpool(dtype, k, s, p, 2, H, W, C, wide)


# ---------------------------------------------------------------------------------------------------------------------------
# nearest resize
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Hi,Wi,Ho,Wo,g", NEAREST)
def test_nearest_resize_forward_and_backward(dtype, Hi, Wi, Ho, Wo, g):
    """ydl_resize_fwd (row-walking and element-indexed kernel) and ydl_resize_bwd, mode 0: min(floor(dst * scale), in - 1) with the scale
    derived from the sizes or given (1 / 2.05 on an output that is twice the input: not the size ratio)"""
    L = G.lib()
    d, tdt, es, V = G.dt(dtype)
    N = 2
    for C in CS[dtype]:
        for wide in (False, True):
            x = ints(Hi + C, (N, Hi, Wi, C), -3, 3) + (np.arange(Hi * Wi).reshape(Hi, Wi) % 29)[None, :, :, None]
            c = R.case_bilinear(x, 0, Ho, Wo, dtype, gh=g, gw=g)
            xb = G.Buf(G.slice_layout(N * Hi * Wi, C, dtype, wide), tdt, x)
            for rows in (1, 0):
                yb = G.Buf(G.slice_layout(N * Ho * Wo, C, dtype, wide), tdt)
                L.debug_set(11, rows)
                try:
                    G.call("ydl_resize_fwd", d, 0, xb.p, xb.lay.ld, yb.p, yb.lay.ld, N, Hi, Wi, Ho, Wo, C, g, g, G.stream())
                    G.sync()
                finally:
                    L.debug_set(11, 1)
                exact(f"nearest {dtype} {Hi}x{Wi}->{Ho}x{Wo} C{C} wide={wide} rows={rows}", yb, c["ref"])
            dy = ints(Ho, (N, Ho, Wo, C), -2, 2)
            prev = ints(Wo, (N, Hi, Wi, C), -4, 4)
            dyb = G.Buf(G.slice_layout(N * Ho * Wo, C, dtype, wide), tdt, dy)
            for acc in (0, 1):
                ref = R.resize_bwd_ref(dy, c["th"], c["tw"], Hi, Wi, prev if acc else None)[0]
                assert np.abs(ref).max() <= 256, "sums must stay exact in bf16"
                dxb = G.Buf(xb.lay, tdt, prev) if acc else G.Buf(xb.lay, tdt)
                G.call("ydl_resize_bwd", d, 0, dyb.p, dyb.lay.ld, dxb.p, dxb.lay.ld, acc, N, Hi, Wi, Ho, Wo, C, g, g, G.stream())
                G.sync()
                exact(f"nearest backward {dtype} {Hi}x{Wi}<-{Ho}x{Wo} C{C} wide={wide} acc={acc}", dxb, ref)


# ---------------------------------------------------------------------------------------------------------------------------
# copy2d
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("npix", [1, 257])
def test_copy2d_vector_and_scalar_paths(dtype, npix):
    """the vector path (C, both strides and both pointers whole chunks) and the three ways into copy2d_scalar_kernel: C % V != 0, a stride
    that is no chunk multiple, a base pointer one element past a 16-byte boundary; overwrite and accumulate"""
    d, tdt, es, V = G.dt(dtype)
    cases = [("vector", 2 * V, 2 * V, 4 * V, R.LEAD, R.LEAD), ("vector, slice", 2 * V, 4 * V, 3 * V, R.LEAD + V, R.LEAD + 2 * V),
             ("C % V", 2 * V - 3, 2 * V, 2 * V, R.LEAD, R.LEAD), ("ld % V", 2 * V, 2 * V + 1, 2 * V, R.LEAD, R.LEAD),
             ("ldd % V", 2 * V, 2 * V, 2 * V + 3, R.LEAD, R.LEAD), ("source base", 2 * V, 3 * V, 2 * V, R.LEAD + 1, R.LEAD),
             ("destination base", 2 * V, 2 * V, 3 * V, R.LEAD, R.LEAD + 1)]
    for what, C, lds, ldd, lead_s, lead_d in cases:
        src = ints(C + npix, (npix, C), -2, 2)
        prev = ints(C, (npix, C), -4, 4)
        sb = G.Buf(R.Layout(npix, lds, C, lead=lead_s), tdt, src)
        for acc in (0, 1):
            lay = R.Layout(npix, ldd, C, lead=lead_d)
            db = G.Buf(lay, tdt, prev) if acc else G.Buf(lay, tdt)
            G.call("ydl_copy2d", d, sb.p, lds, db.p, ldd, npix, C, acc, G.stream())
            G.sync()
            exact(f"copy2d {dtype} {what} npix={npix} acc={acc}", db, src + prev if acc else src)


# ---------------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------------
def _vals(seed, shape):
    """float32 numbers that are NOT exact in bf16: the bf16 store must equal torch's .bfloat16()"""
    return rng(seed).randn(*shape).astype(F32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [3, 12, 20])
@pytest.mark.parametrize("H,W", [(5, 7), (17, 16)])
def test_nchw_nhwc_conversions(dtype, C, H, W):
    """ydl_nchw_to_nhwc zeroes [C, ldd) and rounds like torch; ydl_nhwc_to_nchw copies and accumulates in float32; 17 x 16 pixels need two
    CTAs per image"""
    d, tdt, es, V = G.dt(dtype)
    N = 2
    x = _vals(C + H, (N, C, H, W))
    src = torch.from_numpy(x).cuda()
    for ldd in (R.rup(C, 8), R.rup(C, 8) + 8):
        lay = R.Layout(N * H * W, ldd, C, ldd, "zero")
        ob = G.Buf(lay, tdt)
        G.call("ydl_nchw_to_nhwc", d, ctypes.c_void_p(src.data_ptr()), ob.p, ldd, N, C, H, W, G.stream())
        G.sync()
        exact(f"nchw_to_nhwc {dtype} C{C} {H}x{W} ldd={ldd}", ob, R.store(x.transpose(0, 2, 3, 1), dtype))
    xs = R.store(x.transpose(0, 2, 3, 1), dtype)
    for wide in (False, True):
        sb = G.Buf(G.slice_layout(N * H * W, C, dtype, wide), tdt, xs)
        for acc in (0, 1):
            prev = _vals(7, (N, C, H, W))
            lay = R.Layout(N * C, H * W, H * W)
            ob = G.Buf(lay, torch.float32, prev.reshape(N * C, H * W)) if acc else G.Buf(lay, torch.float32)
            G.call("ydl_nhwc_to_nchw", d, sb.p, sb.lay.ld, ob.p, N, C, H, W, acc, G.stream())
            G.sync()
            want = xs.transpose(0, 3, 1, 2)
            exact(f"nhwc_to_nchw {dtype} C{C} {H}x{W} wide={wide} acc={acc}", ob, (want + prev).astype(F32) if acc else want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,s,H,W", [(3, 2, 10, 14), (3, 2, 34, 32), (4, 2, 10, 14), (3, 4, 8, 12), (12, 2, 34, 32), (20, 1, 5, 7)])
def test_nchw_to_s2d_through_both_kernels(dtype, C, s, H, W):
    """channel (dy * s + dx) * C + c of pixel (h, w) = source pixel (s h + dy, s w + dx); C = 3 / s = 2 takes the pair-loading kernel,
    everything else the generic one; [C s s, ldd) is zero"""
    d, tdt, es, V = G.dt(dtype)
    N = 2
    x = _vals(C + s, (N, C, H, W))
    src = torch.from_numpy(x).cuda()
    Ho, Wo, Cs = H // s, W // s, C * s * s
    want = x.reshape(N, C, Ho, s, Wo, s).transpose(0, 2, 4, 3, 5, 1).reshape(N, Ho, Wo, Cs)
    for ldd in (R.rup(Cs, 8), R.rup(Cs, 8) + 8):
        ob = G.Buf(R.Layout(N * Ho * Wo, ldd, Cs, ldd, "zero"), tdt)
        G.call("ydl_nchw_to_s2d", d, ctypes.c_void_p(src.data_ptr()), ob.p, ldd, N, C, H, W, s, G.stream())
        G.sync()
        exact(f"nchw_to_s2d {dtype} C{C} s{s} {H}x{W} ldd={ldd}", ob, R.store(want, dtype))


# ---------------------------------------------------------------------------------------------------------------------------
# zero fills, casts, transport
# ---------------------------------------------------------------------------------------------------------------------------
def test_fill_zero_heads_and_tails():
    """destination offsets of 0, 1, 7 and 15 bytes from a 16-byte boundary, sizes of 0, 1, 15, 16, 17 and 4099 bytes"""
    for off in (0, 1, 7, 15):
        for size in (0, 1, 15, 16, 17, 4099):
            lay = R.Layout(1, max(size, 1), size, lead=32 + off) if size else R.Layout(0, 1, 0, lead=32 + off)
            b = G.Buf(lay, torch.uint8, sent=0xA5)
            G.call("ydl_fill_zero", b.p, size, G.stream())
            G.sync()
            host = b.host()
            assert bool((host[:lay.lead] == 0xA5).all()) and bool((host[lay.lead + size:] == 0xA5).all()), (off, size)
            assert bool((host[lay.lead:lay.lead + size] == 0).all()), (off, size)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero2d_dense_and_strided(dtype):
    d, tdt, es, V = G.dt(dtype)
    for npix, C, ld in [(1, 5, 5), (257, 12, 12), (257, 12, 20), (9, 3, 7)]:
        b = G.Buf(R.Layout(npix, ld, C), tdt)
        G.call("ydl_zero2d", d, b.p, ld, npix, C, G.stream())
        G.sync()
        exact(f"zero2d {dtype} npix={npix} C={C} ld={ld}", b, np.zeros((npix, C)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_casts_and_chunk_reduction(dtype):
    """ydl_cast_f32 (strided rows, overwrite and accumulate: float32 addition, one rounding to the storage type), ydl_cast_to_f32, and
    ydl_reduce_chunks, whose contract is the float32 sum in the fixed order r = 0, 1, ...: compared to the bit with that sum"""
    d, tdt, es, V = G.dt(dtype)
    npix, C = 37, 11
    src = _vals(1, (npix, C))
    prev = R.store(_vals(2, (npix, C)), dtype)
    sb = G.Buf(R.Layout(npix, C + 2, C), torch.float32, src)
    for acc in (0, 1):
        lay = R.Layout(npix, C + 5, C)
        db = G.Buf(lay, tdt, prev) if acc else G.Buf(lay, tdt)
        G.call("ydl_cast_f32", d, sb.p, C + 2, db.p, C + 5, npix, C, acc, G.stream())
        G.sync()
        exact(f"cast_f32 {dtype} acc={acc}", db, R.store((src + prev).astype(F32) if acc else src, dtype))
    n = 1000
    v = R.store(_vals(3, (1, n)), dtype)
    vb = G.Buf(R.Layout(1, n, n), tdt, v)
    p32 = _vals(4, (1, n))
    for acc in (0, 1):
        ob = G.Buf(R.Layout(1, n, n), torch.float32, p32) if acc else G.Buf(R.Layout(1, n, n), torch.float32)
        G.call("ydl_cast_to_f32", d, vb.p, ob.p, n, acc, G.stream())
        G.sync()
        exact(f"cast_to_f32 {dtype} acc={acc}", ob, (p32 + v).astype(F32) if acc else v)
    for nchunks in (1, 2, 8):
        ch = R.store(_vals(nchunks, (nchunks, n)) * F32(1000), dtype)
        cb = G.Buf(R.Layout(nchunks, n, n), tdt, ch)
        ob = G.Buf(R.Layout(1, n, n), torch.float32)
        G.call("ydl_reduce_chunks", d, cb.p, ob.p, n, nchunks, G.stream())
        G.sync()
        want = np.zeros(n, dtype=F32)
        for r in range(nchunks):
            want = (want + ch[r]).astype(F32)
        exact(f"reduce_chunks {dtype} nchunks={nchunks}", ob, want)


# ---------------------------------------------------------------------------------------------------------------------------
# global max, arg-max, and the backward
# ---------------------------------------------------------------------------------------------------------------------------
def tie_planes(seed, N, HW, C):
    """integers in [-3, 3]; from HW = 557 on, channel 0 holds its only maxima at pixels 300 and 556 (the same thread, 44) and channel 1
    at 260 and 9 (thread 4 finds its own first, thread 9 owns the smaller index)"""
    x = ints(seed, (N, HW, C), -3, 3)
    if HW >= 557:
        x[:, :, :2] = np.minimum(x[:, :, :2], 2)
        x[:, [300, 556], 0] = 3
        x[:, [260, 9], 1] = 3
    return x


def global_pool_call(dtype, x, wide):
    """-> (avg, max, arg-max buffers) of one ydl_global_pool_fwd call on x (N, HW, C)"""
    d, tdt, es, V = G.dt(dtype)
    N, HW, C = x.shape
    Cp = R.rup(C, V)
    xb = G.Buf(G.slice_layout(N * HW, C, dtype, wide), tdt, x, pad=0.0)
    ab, mb = G.Buf(G.slice_layout(N, C, dtype, wide), tdt), G.Buf(G.slice_layout(N, C, dtype, wide), tdt)
    ib = G.Buf(R.Layout(N, Cp, C, Cp), torch.int32, sent=-7)
    G.call("ydl_global_pool_fwd", d, xb.p, xb.lay.ld, ab.p, ab.lay.ld, mb.p, mb.lay.ld, ib.p, N, HW, C, G.stream())
    G.sync()
    return ab, mb, ib


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW", [1, 5, 255, 256, 257, 1000])
def test_global_max_and_arg_max(dtype, HW):
    """the per-thread scan (p = tid, tid + 256, ...) and the merge of the 256 partials: the first maximum in pixel order, also where the
    equal maxima sit in one thread or in two; C = 4, 12 / 8, 20 and one C that is no chunk multiple"""
    for C in CS[dtype] + (7,):
        for wide in (False, True):
            x = tie_planes(HW + C, 3, HW, C)
            avg, mx, am = R.global_pool_ref(x)
            if HW >= 557:
                assert (am[:, 0] == 300).all() and (am[:, 1] == 9).all()
            ab, mb, ib = global_pool_call(dtype, x, wide)
            tag = f"global max {dtype} HW={HW} C={C} wide={wide}"
            exact(tag, mb, mx)
            exact(tag + " arg-max", ib, am, -7)
            assert R.accepted(R.check_exact(ab.host(), dict(layout=ab.lay, ref=ab.lay.answer(ab.host())))), tag + ": sentinels around the average"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW", [1, 5, 256, 1000])
def test_global_pool_backward_exact(dtype, HW):
    """dx (+)= davg / HW + [p == arg-max] dmx, the three pointer combinations, overwrite and accumulate.  davg holds small integers times
    HW, so davg * (1 / HW) is exact where 1 / HW is: HW = 1 and 256; at the other sizes only the max branch is exact (the average
    branch with its roundings is in tests/test_gpu_spatial_f64.py)"""
    d, tdt, es, V = G.dt(dtype)
    N = 3
    for C in CS[dtype] + (7,):
        Cp = R.rup(C, V)
        x = tie_planes(HW + C, N, HW, C)
        am = R.global_pool_ref(x)[2]
        davg, dmx = ints(1, (N, C), -2, 2) * HW, ints(2, (N, C), -2, 2)
        prev = ints(3, (N, HW, C), -4, 4)
        combos = [("max", None, dmx)] + ([("avg", davg, None), ("both", davg, dmx)] if HW in (1, 256) else [])
        ib = G.Buf(R.Layout(N, Cp, C, Cp), torch.int32, am, pad=0, sent=-7)
        for what, a, m in combos:
            for wide in (False, True):
                ab = None if a is None else G.Buf(G.slice_layout(N, C, dtype, wide), tdt, a)
                mb = None if m is None else G.Buf(G.slice_layout(N, C, dtype, wide), tdt, m)
                lda = G.slice_layout(N, C, dtype, wide).ld
                for acc in (0, 1):
                    lay = G.slice_layout(N * HW, C, dtype, wide)
                    dxb = G.Buf(lay, tdt, prev) if acc else G.Buf(lay, tdt)
                    G.call("ydl_global_pool_bwd", d, ab.p if ab else None, lda, mb.p if mb else None, lda, ib.p, dxb.p, lay.ld, acc,
                           N, HW, C, G.stream())
                    G.sync()
                    exact(f"global_pool_bwd {dtype} HW={HW} C={C} {what} wide={wide} acc={acc}", dxb,
                          R.global_pool_bwd_ref(a, m, am, HW, prev if acc else None))


NAN_HW = 1000


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", [[601], [300, 777]], ids=["one", "two"])
def test_global_max_of_a_plane_with_nan(dtype, where):
    """what F.adaptive_max_pool2d returns on the CPU (tests/test_spatial_ref_cpu.py pins it): the maximum is NaN and the index that of the
    LAST NaN; the NaNs sit at pixels owned by threads 89, 44 and 9.  The gradient of the max branch goes to that index."""
    d, tdt, es, V = G.dt(dtype)
    C = CS[dtype][0]
    x = tie_planes(5, 2, NAN_HW, C)
    x[1, where, 2] = np.nan
    avg, mx, am = R.global_pool_ref(x)
    assert np.isnan(mx[1, 2]) and am[1, 2] == where[-1]
    ab, mb, ib = global_pool_call(dtype, x, False)
    exact("global max with NaN", mb, mx)
    exact("arg-max with NaN", ib, am, -7)
    dmx = np.ones((2, C))
    mbuf = G.Buf(G.slice_layout(2, C, dtype, False), tdt, dmx)
    dxb = G.Buf(G.slice_layout(2 * NAN_HW, C, dtype, False), tdt)
    G.call("ydl_global_pool_bwd", d, None, C, mbuf.p, mbuf.lay.ld, ib.p, dxb.p, dxb.lay.ld, 0, 2, NAN_HW, C, G.stream())
    G.sync()
    exact("gradient of the max branch", dxb, R.global_pool_bwd_ref(None, dmx, am, NAN_HW))
    assert dxb.lay.answer(dxb.host()).reshape(2, NAN_HW, C)[1, :, 2].argmax() == where[-1]


# ---------------------------------------------------------------------------------------------------------------------------
# the second trip of the grid-stride loops
# ---------------------------------------------------------------------------------------------------------------------------
BIG_H, BIG_W, BIG_C = 513, 512, 16            # 262 656 pixels x 4 float32 chunks: just over the 4096 x 256 threads of the capped grid


def _big(seed, lo, hi, shape=(1, BIG_H, BIG_W, BIG_C)):
    return rng(seed).randint(lo, hi + 1, size=shape).astype(F32)


def test_grid_stride_second_trip_max_pool():
    d, tdt, es, V = G.dt("f32")
    k, s, p = 3, 1, 1
    x = _big(1, -3, 3)
    y, code = R.maxpool_ref(x, k, s, p)
    xb = G.Buf(R.Layout(BIG_H * BIG_W, BIG_C, BIG_C), tdt, x)
    yb = G.Buf(xb.lay, tdt)
    ib = G.Buf(xb.lay, torch.uint8, sent=255)
    G.call("ydl_maxpool_fwd", d, xb.p, BIG_C, yb.p, BIG_C, ib.p, 1, BIG_H, BIG_W, BIG_H, BIG_W, BIG_C, k, s, p, G.stream())
    G.sync()
    exact("values", yb, y)
    exact("codes", ib, code, 255)
    dy = _big(2, -2, 2)
    prev = _big(3, -4, 4)
    dyb, dxb = G.Buf(xb.lay, tdt, dy), G.Buf(xb.lay, tdt, prev)
    G.call("ydl_maxpool_bwd", d, dyb.p, BIG_C, ib.p, dxb.p, BIG_C, 1, 1, BIG_H, BIG_W, BIG_H, BIG_W, BIG_C, k, s, p, G.stream())
    G.sync()
    exact("backward", dxb, R.maxpool_bwd_ref(dy, code, BIG_H, BIG_W, k, s, p, prev))


def test_grid_stride_second_trip_copy_scale_and_global_pool_backward():
    d, tdt, es, V = G.dt("f32")
    lay = R.Layout(BIG_H * BIG_W, BIG_C, BIG_C)
    src, prev = _big(4, -2, 2), _big(5, -4, 4)
    sb, db = G.Buf(lay, tdt, src), G.Buf(lay, tdt, prev)
    G.call("ydl_copy2d", d, sb.p, BIG_C, db.p, BIG_C, BIG_H * BIG_W, BIG_C, 1, G.stream())
    G.sync()
    exact("copy2d", db, src + prev)
    # the scalar path: 11 channels of the same rows, 2 889 216 elements
    db = G.Buf(R.Layout(BIG_H * BIG_W, BIG_C, 11), tdt, prev[..., :11])
    G.call("ydl_copy2d", d, sb.p, BIG_C, db.p, BIG_C, BIG_H * BIG_W, 11, 1, G.stream())
    G.sync()
    exact("copy2d, scalar path", db, (src + prev)[..., :11])
    gate = rng(6).randint(-2, 3, size=(1, BIG_C)).astype(F32)
    gb = torch.from_numpy(gate).cuda()
    ob = G.Buf(lay, tdt)
    G.call("ydl_scale_channels", d, sb.p, BIG_C, ctypes.c_void_p(gb.data_ptr()), ob.p, BIG_C, 1, BIG_H * BIG_W, BIG_C, G.stream())
    G.sync()
    exact("scale_channels", ob, src * gate[None])
    HW = BIG_H * BIG_W
    am = rng(7).randint(0, HW, size=(1, BIG_C)).astype(np.int32)
    am[0, 0], am[0, 1] = HW - 1, 262144               # the last pixel, and the first one of the second trip
    dmx = rng(8).randint(-2, 3, size=(1, BIG_C)).astype(F32)
    ib = G.Buf(R.Layout(1, BIG_C, BIG_C), torch.int32, am, sent=-7)
    mb = G.Buf(R.Layout(1, BIG_C, BIG_C), tdt, dmx)
    dxb = G.Buf(lay, tdt, prev)
    G.call("ydl_global_pool_bwd", d, None, BIG_C, mb.p, BIG_C, ib.p, dxb.p, BIG_C, 1, 1, HW, BIG_C, G.stream())
    G.sync()
    exact("global_pool_bwd", dxb, R.global_pool_bwd_ref(None, dmx, am, HW, prev.reshape(1, HW, BIG_C), dtype=F32))


def test_grid_stride_second_trip_nearest_resize():
    """the element-indexed forward at 513 x 512 output pixels, the backward at 513 x 512 input pixels, and the row-walking forward at
    4100 rows of 8 pixels (its cap is 4096 CTAs)"""
    L = G.lib()
    d, tdt, es, V = G.dt("f32")
    Hi, Wi = 257, 256
    x = _big(9, -3, 3, (1, Hi, Wi, BIG_C))
    c = R.case_bilinear(x, 0, BIG_H, BIG_W, "f32")
    xb = G.Buf(R.Layout(Hi * Wi, BIG_C, BIG_C), tdt, x)
    yb = G.Buf(R.Layout(BIG_H * BIG_W, BIG_C, BIG_C), tdt)
    L.debug_set(11, 0)
    try:
        G.call("ydl_resize_fwd", d, 0, xb.p, BIG_C, yb.p, BIG_C, 1, Hi, Wi, BIG_H, BIG_W, BIG_C, 0.0, 0.0, G.stream())
        G.sync()
    finally:
        L.debug_set(11, 1)
    exact("element-indexed forward", yb, c["ref"])
    # backward: 513 x 512 input pixels gather from a 257 x 256 output (down-sampling)
    dy = _big(10, -2, 2, (1, Hi, Wi, BIG_C))
    th, tw = R.axis_taps(0, BIG_H, Hi), R.axis_taps(0, BIG_W, Wi)
    ref = R.resize_bwd_matrix(dy, th, tw, BIG_H, BIG_W)[0]
    dyb = G.Buf(R.Layout(Hi * Wi, BIG_C, BIG_C), tdt, dy)
    dxb = G.Buf(R.Layout(BIG_H * BIG_W, BIG_C, BIG_C), tdt)
    G.call("ydl_resize_bwd", d, 0, dyb.p, BIG_C, dxb.p, BIG_C, 0, 1, BIG_H, BIG_W, Hi, Wi, BIG_C, 0.0, 0.0, G.stream())
    G.sync()
    exact("backward", dxb, ref)
    x = _big(11, -3, 3, (1, 2050, 4, 4))
    c = R.case_bilinear(x, 0, 4100, 8, "f32")
    xb = G.Buf(R.Layout(2050 * 4, 4, 4), tdt, x)
    yb = G.Buf(R.Layout(4100 * 8, 4, 4), tdt)
    G.call("ydl_resize_fwd", d, 0, xb.p, 4, yb.p, 4, 1, 2050, 4, 4100, 8, 4, 0.0, 0.0, G.stream())
    G.sync()
    exact("row-walking forward", yb, c["ref"])


def test_grid_stride_second_trip_stream_grid():
    """stream_grid of csrc/dcn_blocks.hip caps the grid at 4096 CTAs of 256 threads: 1 048 577 work items are one more than its threads"""
    n = 4096 * 256 + 1
    for dtype in DTYPES:
        d, tdt, es, V = G.dt(dtype)
        v = R.store(rng(1).randn(2, n).astype(F32), dtype)
        vb = G.Buf(R.Layout(2, n, n), tdt, v)
        ob = G.Buf(R.Layout(1, n, n), torch.float32)
        G.call("ydl_cast_to_f32", d, vb.p, ob.p, n, 0, G.stream())
        G.sync()
        exact("cast_to_f32", ob, v[0])
        ob = G.Buf(R.Layout(1, n, n), torch.float32)
        G.call("ydl_reduce_chunks", d, vb.p, ob.p, n, 2, G.stream())
        G.sync()
        exact("reduce_chunks", ob, (v[0] + v[1]).astype(F32))
        sb = G.Buf(R.Layout(1, n, n), torch.float32, v[:1])
        ob = G.Buf(R.Layout(n, 1, 1), tdt)
        G.call("ydl_cast_f32", d, sb.p, 1, ob.p, 1, n, 1, 0, G.stream())
        G.sync()
        exact("cast_f32", ob, v[0])
        ob = G.Buf(R.Layout(n, 2, 1), tdt)
        G.call("ydl_zero2d", d, ob.p, 2, n, 1, G.stream())
        G.sync()
        exact("zero2d", ob, np.zeros(n))


# ---------------------------------------------------------------------------------------------------------------------------
# host refusals: non-zero return, ydl_last_error names the function, nothing launched
# ---------------------------------------------------------------------------------------------------------------------------
def _bufs(dtype, rows=6 * 6 * 2, ld=None):
    d, tdt, es, V = G.dt(dtype)
    lay = R.Layout(rows, ld or 2 * V, 2 * V)
    return G.Buf(lay, tdt), G.Buf(lay, tdt)


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_of_short_strides_null_pointers_sizes_and_modes(dtype):
    d, tdt, es, V = G.dt(dtype)
    C, st = 2 * V, G.stream()
    a, b = _bufs(dtype)
    idx = G.Buf(R.Layout(72, C, C), torch.uint8, sent=255)
    am = G.Buf(R.Layout(2, C, C), torch.int32, sent=-7)
    f = G.Buf(R.Layout(2, C, C), torch.float32)
    N, H, W = 2, 6, 6
    short = C - V
    # ld < Cp
    G.refused("ydl_maxpool_fwd", (d, a.p, short, b.p, C, idx.p, N, H, W, H, W, C, 3, 1, 1, st), [b, idx])
    G.refused("ydl_maxpool_bwd", (d, a.p, C, idx.p, b.p, short, 0, N, H, W, H, W, C, 3, 1, 1, st), [b])
    G.refused("ydl_resize_fwd", (d, 1, a.p, C, b.p, short, N, 3, 3, H, W, C, 0.0, 0.0, st), [b])
    G.refused("ydl_resize_bwd", (d, 1, a.p, short, b.p, C, 0, N, 3, 3, H, W, C, 0.0, 0.0, st), [b])
    G.refused("ydl_resize_acc_sums", (d, 1, a.p, short, b.p, C, N, 3, 3, H, W, C, 0.0, 0.0, None, 0, st), [b])
    G.refused("ydl_copy2d", (d, a.p, C - 1, b.p, C, 72, C, 0, st), [b])
    G.refused("ydl_scale_channels", (d, a.p, C, f.p, b.p, short, N, 36, C, st), [b])
    G.refused("ydl_global_pool_fwd", (d, a.p, C, b.p, short, b.p, C, am.p, N, 36, C, st), [b, am])
    G.refused("ydl_global_pool_bwd", (d, a.p, C, None, C, am.p, b.p, short, 0, N, 36, C, st), [b])
    G.refused("ydl_channel_dot", (d, a.p, short, b.p, C, f.p, N, 36, C, st), [f])
    G.refused("ydl_nchw_to_nhwc", (d, f.p, b.p, C - 8, 1, C, 2, 2, st), [b])
    G.refused("ydl_nhwc_to_nchw", (d, a.p, short, f.p, 1, C, 1, 2, 0, st), [f])
    G.refused("ydl_group_softmax_fwd", (d, a.p, C - 1, b.p, C, 72, 1, C, st), [b])
    G.refused("ydl_group_softmax_bwd", (d, a.p, C, a.p, C, b.p, C - 1, 0, 72, 1, C, st), [b])
    G.refused("ydl_cast_f32", (d, f.p, C, b.p, C - 1, 2, C, 0, st), [b])
    G.refused("ydl_zero2d", (d, b.p, C - 1, 72, C, st), [b])
    # null pointers
    G.refused("ydl_maxpool_fwd", (d, None, C, b.p, C, idx.p, N, H, W, H, W, C, 3, 1, 1, st), [b, idx])
    G.refused("ydl_maxpool_bwd", (d, a.p, C, None, b.p, C, 0, N, H, W, H, W, C, 3, 1, 1, st), [b])
    G.refused("ydl_resize_fwd", (d, 1, None, C, b.p, C, N, 3, 3, H, W, C, 0.0, 0.0, st), [b])
    G.refused("ydl_resize_bwd", (d, 1, None, C, b.p, C, 0, N, 3, 3, H, W, C, 0.0, 0.0, st), [b])
    G.refused("ydl_copy2d", (d, None, C, b.p, C, 72, C, 0, st), [b])
    G.refused("ydl_scale_channels", (d, a.p, C, None, b.p, C, N, 36, C, st), [b])
    G.refused("ydl_global_pool_fwd", (d, a.p, C, b.p, C, b.p, C, None, N, 36, C, st), [b])
    G.refused("ydl_global_pool_bwd", (d, None, C, None, C, am.p, b.p, C, 0, N, 36, C, st), [b])
    G.refused("ydl_gate_fwd", (d, a.p, C, None, C, f.p, 2, C, st), [f])
    G.refused("ydl_gate_bwd", (d, f.p, None, a.p, C, 0, b.p, C, 0, 2, C, st), [a, b])
    G.refused("ydl_channel_dot", (d, a.p, C, b.p, C, None, N, 36, C, st), [])
    G.refused("ydl_nchw_to_nhwc", (d, None, b.p, C, 1, C, 2, 2, st), [b])
    G.refused("ydl_nhwc_to_nchw", (d, None, C, f.p, 1, C, 1, 2, 0, st), [f])
    G.refused("ydl_nchw_to_s2d", (d, None, b.p, C, 1, 1, 2, 2, 2, st), [b])
    G.refused("ydl_cast_to_f32", (d, None, f.p, 2 * C, 0, st), [f])
    G.refused("ydl_reduce_chunks", (d, a.p, None, C, 2, st), [])
    G.refused("ydl_bn_eval_coeffs", (C, f.p, f.p, f.p, None, 1e-3, f.p, f.p, st), [f])
    G.refused("ydl_fill_zero", (None, 16, st), [])
    # an output size that does not match (k, s, p); a mode outside 0..2; H % s != 0
    G.refused("ydl_maxpool_fwd", (d, a.p, C, b.p, C, idx.p, N, H, W, H, W, C, 3, 2, 1, st), [b, idx], "output size")
    G.refused("ydl_maxpool_fwd", (d, a.p, C, b.p, C, idx.p, N, H, W, H - 1, W, C, 3, 1, 1, st), [b, idx], "output size")
    for mode in (-1, 3):
        G.refused("ydl_resize_fwd", (d, mode, a.p, C, b.p, C, N, 3, 3, H, W, C, 0.0, 0.0, st), [b])
        G.refused("ydl_resize_bwd", (d, mode, a.p, C, b.p, C, 0, N, 3, 3, H, W, C, 0.0, 0.0, st), [b])
        G.refused("ydl_resize_acc_sums", (d, mode, a.p, C, b.p, C, N, 3, 3, H, W, C, 0.0, 0.0, None, 0, st), [b])
    G.refused("ydl_nchw_to_s2d", (d, f.p, b.p, 16, 1, 1, 3, 4, 2, st), [b])
    G.refused("ydl_nchw_to_s2d", (d, f.p, b.p, 16, 1, 1, 4, 3, 2, st), [b])


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_of_misaligned_vector_operands(dtype):
    """the entry points that read or write 16-byte channel vectors refuse a pointer that is not 16-byte aligned and a pixel stride that
    is no whole number of chunks (the three-pool launches, ydl_resize_acc_sums and ydl_bn_act_fwd always did)"""
    d, tdt, es, V = G.dt(dtype)
    C, st = 2 * V, G.stream()
    a, b = _bufs(dtype, ld=2 * V + V)
    odd = 2 * V + 1                                          # a stride that covers C but is no chunk multiple
    a1, b1 = ctypes.c_void_p(a.p.value + es), ctypes.c_void_p(b.p.value + es)      # one element past the boundary
    idx = G.Buf(R.Layout(72, C, C), torch.uint8, sent=255)
    am = G.Buf(R.Layout(2, C, C), torch.int32, sent=-7)
    f = G.Buf(R.Layout(2 * C, 4, 4), torch.float32)
    N, H, W, ld = 2, 6, 6, 3 * V
    for x_, ldx, y_, ldy in [(a1, ld, b.p, ld), (a.p, ld, b1, ld), (a.p, odd, b.p, ld), (a.p, ld, b.p, odd)]:
        G.refused("ydl_maxpool_fwd", (d, x_, ldx, y_, ldy, idx.p, N, 4, 4, 4, 4, C, 3, 1, 1, st), [b, idx], "alignment")
        G.refused("ydl_maxpool_bwd", (d, x_, ldx, idx.p, y_, ldy, 0, N, 4, 4, 4, 4, C, 3, 1, 1, st), [b], "alignment")
        G.refused("ydl_resize_fwd", (d, 1, x_, ldx, y_, ldy, N, 2, 2, 4, 4, C, 0.0, 0.0, st), [b], "alignment")
        G.refused("ydl_resize_bwd", (d, 1, x_, ldx, y_, ldy, 0, N, 4, 4, 2, 2, C, 0.0, 0.0, st), [b], "alignment")
        G.refused("ydl_scale_channels", (d, x_, ldx, f.p, y_, ldy, N, 16, C, st), [b], "alignment")
    for x_, ldx in [(a1, ld), (a.p, odd)]:
        G.refused("ydl_global_pool_fwd", (d, x_, ldx, b.p, ld, b.p, ld, am.p, N, 16, C, st), [b, am], "alignment")
        G.refused("ydl_global_pool_bwd", (d, a.p, ld, None, ld, am.p, ctypes.c_void_p(b.p.value + (x_.value - a.p.value)), ldx, 0, N, 16, C, st), [b], "alignment")
        G.refused("ydl_channel_dot", (d, x_, ldx, b.p, ld, f.p, N, 16, C, st), [f], "alignment")
        G.refused("ydl_channel_dot", (d, b.p, ld, x_, ldx, f.p, N, 16, C, st), [f], "alignment")
        G.refused("ydl_nhwc_to_nchw", (d, x_, ldx, f.p, 1, 4, 1, 2, 0, st), [f], "alignment")
    G.refused("ydl_nchw_to_nhwc", (d, f.p, b1, 8, 1, 4, 1, 2, st), [b], "alignment")
