"""GPU: ydl_space_to_depth / ydl_depth_to_space at the C ABI, to the bit.  Copies are exact, so the reference is torch indexing on the CPU
(tests/sd_ref.py, pinned to Focus / Contract / Expand by tests/test_sd_ref_cpu.py) and every comparison is on the raw bit patterns.

Shapes are the smallest at which a path can go wrong: N = 2, a 4 x 6 coarse map (the fine side is 4s x 6s, so a coarse row holds up to
6 * 9 * 24 elements: several blocks), C in {3, 8, 12, 24} (the element kernel; one 16-byte vector in bf16; blocks that start at 24-byte
offsets; several vectors), s in {2, 3}, both orders, bf16 and f32.  Per case three layouts:
  dense       whole buffers, row stride = the channels rounded up to 8
  out_slice   the output is a channel slice at offset 8 of a wider buffer
  in_slice    the input is a slice at offset 3 of a wider buffer (not a multiple of 8: only the element kernel can serve it)
Every buffer is filled with a sentinel bit pattern first; after the launch the padding and the neighbouring channels still hold it.
``accumulate`` = 1 equals the once-rounded f32 sum; depth_to_space(space_to_depth(x)) is x; bad arguments return non-zero with a
message and launch nothing."""
import ctypes

import pytest
import torch

from tests.sd_ref import depth_to_space_ref, space_to_depth_ref

pytestmark = pytest.mark.gpu

N, HC, WC = 2, 4, 6
CS = (3, 8, 12, 24)
LAYOUTS = ("dense", "out_slice", "in_slice")
SENTINEL = {torch.bfloat16: 0x7FC1, torch.float32: 0x7FC12345}


def _L():
    from yolo_dual_amd import _lib as L
    return L


def _dt(dtype):
    L = _L()
    return (L.YDL_BF16, torch.bfloat16) if dtype == "bf16" else (L.YDL_F32, torch.float32)


def _raw(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _up8(c):
    return (c + 7) // 8 * 8


def sentinel_buffer(n, h, w, ld, tdt):
    buf = torch.empty((n, h, w, ld), dtype=tdt, device="cuda")
    _raw(buf).fill_(SENTINEL[tdt])          # a NaN pattern no random draw produces
    return buf


def place(buf, off, nchw):
    """write an (N, C, H, W) tensor into channels [off, off + C) of an NHWC buffer"""
    buf[..., off:off + nchw.shape[1]] = nchw.permute(0, 2, 3, 1).to(buf.device)
    return buf


def at(buf, off):
    return ctypes.c_void_p(buf.data_ptr() + off * buf.element_size())


def untouched(buf, off, c):
    """every channel outside [off, off + c) still holds the sentinel"""
    r = _raw(buf)
    return bool((r[..., :off] == SENTINEL[buf.dtype]).all()) and bool((r[..., off + c:] == SENTINEL[buf.dtype]).all())


def geometry(down, C, s):
    """shapes (N, C, H, W) of x and y and the entry point"""
    fine, coarse = (N, C, HC * s, WC * s), (N, C * s * s, HC, WC)
    return ("ydl_space_to_depth", fine, coarse) if down else ("ydl_depth_to_space", coarse, fine)


def layout(kind, cx, cy):
    """(ldx, x offset, ldy, y offset)"""
    if kind == "dense":
        return _up8(cx), 0, _up8(cy), 0
    if kind == "out_slice":
        return _up8(cx), 0, _up8(cy) + 24, 8
    return _up8(cx) + 8, 3, _up8(cy), 0


def launch(entry, dt, xb, ldx, xo, yb, ldy, yo, xshape, C, s, order, acc):
    _L().call(entry, dt, at(xb, xo), ldx, at(yb, yo), ldy, xshape[0], xshape[2], xshape[3], C, s, order, acc, _st())
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("down", [True, False], ids=["space_to_depth", "depth_to_space"])
def test_copy_is_exact_in_every_layout_and_touches_nothing_else(down, s, order, dtype):
    dt, tdt = _dt(dtype)
    ref = space_to_depth_ref if down else depth_to_space_ref
    g = torch.Generator().manual_seed(100 * s + 10 * order + down)
    for C in CS:
        entry, xs, ys = geometry(down, C, s)
        x = torch.randn(*xs, generator=g).to(tdt)
        want = ref(x, s, order)
        assert tuple(want.shape) == ys
        for kind in LAYOUTS:
            ldx, xo, ldy, yo = layout(kind, xs[1], ys[1])
            xb = place(sentinel_buffer(xs[0], xs[2], xs[3], ldx, tdt), xo, x)
            yb = sentinel_buffer(ys[0], ys[2], ys[3], ldy, tdt)
            x_before = _raw(xb).clone()
            launch(entry, dt, xb, ldx, xo, yb, ldy, yo, xs, C, s, order, 0)
            got = yb[..., yo:yo + ys[1]].permute(0, 3, 1, 2).cpu()
            assert torch.equal(_raw(got.contiguous()), _raw(want.contiguous())), (C, kind)
            assert untouched(yb, yo, ys[1]), (C, kind)
            assert torch.equal(_raw(xb), x_before), (C, kind)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("down", [True, False], ids=["space_to_depth", "depth_to_space"])
def test_accumulate_adds_in_f32_with_one_rounding(down, dtype):
    dt, tdt = _dt(dtype)
    ref = space_to_depth_ref if down else depth_to_space_ref
    g = torch.Generator().manual_seed(7 + down)
    for C, s, order, kind in ((3, 2, 1, "dense"), (8, 2, 0, "out_slice"), (12, 3, 0, "dense"), (24, 2, 1, "in_slice"), (24, 3, 1, "dense")):
        entry, xs, ys = geometry(down, C, s)
        x, y0 = torch.randn(*xs, generator=g).to(tdt), torch.randn(*ys, generator=g).to(tdt)
        want = (ref(x, s, order).float() + y0.float()).to(tdt)
        ldx, xo, ldy, yo = layout(kind, xs[1], ys[1])
        xb = place(sentinel_buffer(xs[0], xs[2], xs[3], ldx, tdt), xo, x)
        yb = place(sentinel_buffer(ys[0], ys[2], ys[3], ldy, tdt), yo, y0)
        launch(entry, dt, xb, ldx, xo, yb, ldy, yo, xs, C, s, order, 1)
        got = yb[..., yo:yo + ys[1]].permute(0, 3, 1, 2).cpu()
        assert torch.equal(_raw(got.contiguous()), _raw(want.contiguous())), (C, s, order, kind)
        assert untouched(yb, yo, ys[1]), (C, s, order, kind)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("order", [0, 1])
def test_depth_to_space_inverts_space_to_depth(order, dtype):
    dt, tdt = _dt(dtype)
    g = torch.Generator().manual_seed(21 + order)
    for C, s in ((3, 2), (12, 3), (24, 2)):
        _e, xs, ys = geometry(True, C, s)
        x = torch.randn(*xs, generator=g).to(tdt)
        ldx, ldy = _up8(xs[1]), _up8(ys[1])
        xb = place(sentinel_buffer(xs[0], xs[2], xs[3], ldx, tdt), 0, x)
        yb = sentinel_buffer(ys[0], ys[2], ys[3], ldy, tdt)
        zb = sentinel_buffer(xs[0], xs[2], xs[3], ldx, tdt)
        launch("ydl_space_to_depth", dt, xb, ldx, 0, yb, ldy, 0, xs, C, s, order, 0)
        launch("ydl_depth_to_space", dt, yb, ldy, 0, zb, ldx, 0, ys, C, s, order, 0)
        assert torch.equal(_raw(zb), _raw(xb)), (C, s)            # the sentinel padding included


def test_bad_arguments_are_refused_with_a_message():
    L = _L()
    lib = L.lib()
    dt, tdt = _dt("bf16")
    xb, yb = sentinel_buffer(2, 4, 6, 8, tdt), sentinel_buffer(2, 2, 3, 32, tdt)
    before = _raw(yb).clone()

    def s2d(H=4, W=6, C=8, s=2, order=0, ldx=8, ldy=32, dtype=dt):
        return lib.ydl_space_to_depth(dtype, at(xb, 0), ldx, at(yb, 0), ldy, 2, H, W, C, s, order, 0, _st())

    def d2s(C=2, s=2, order=0, ldx=8, ldy=32):
        return lib.ydl_depth_to_space(dt, at(xb, 0), ldx, at(yb, 0), ldy, 2, 1, 1, C, s, order, 0, _st())
    for what, rc in (("H % s", s2d(H=3)), ("W % s", s2d(W=5)), ("ldx < C", s2d(ldx=7)), ("ldy < s*s*C", s2d(ldy=31)), ("s < 1", s2d(s=0)),
                     ("order", s2d(order=2)), ("order", s2d(order=-1)), ("dtype", s2d(dtype=7)),
                     ("ldx < s*s*C", d2s(ldx=7)), ("ldy < C", d2s(ldy=1)), ("s < 1", d2s(s=0)), ("order", d2s(order=2))):
        msg = (lib.ydl_last_error() or b"").decode()
        assert rc != 0 and ("ydl_space_to_depth" in msg or "ydl_depth_to_space" in msg), (what, rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(_raw(yb), before)
    assert s2d() == 0
    torch.cuda.synchronize()
