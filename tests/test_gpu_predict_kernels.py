"""GPU: the prediction kernels (csrc/predict.hip) at their C ABI, exact against tests/predict_ref.py / torch on the same stored values.
Outputs go into sentinel-filled buffers with strides wider than a row: every byte outside the promised ones keeps the sentinel."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import predict_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENT = 0xEE
vp = ctypes.c_void_p


def _lib():
    from yolo_dual_amd import _lib as L
    return L


def _call(name, *args):
    L = _lib()
    L.call(name, *args, vp(0))
    torch.cuda.synchronize()


def _ptr(t):
    return vp(0 if t is None else t.data_ptr())


def _scores(N, C, H, W, seed, special=False):
    """small integers so that ties occur in most pixels (exact in bf16 too)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).float()
    if special:
        inf, nan = float("inf"), float("nan")
        x[0, :, 0, 0] = -inf                                  # all -inf: label 0
        if C >= 4:
            x[0, :4, 0, 1] = torch.tensor([1.0, nan, 3.0, nan])     # the first NaN wins
            x[0, 2, 0, 2] = inf
            x[0, 1, 0, 3], x[0, 3, 0, 3] = inf, inf           # two +inf: the first
            x[0, 0, 1, 0], x[0, 2, 1, 0] = inf, nan           # NaN beats +inf
        x[0, C - 1, 1, 1] = nan                               # NaN in the last channel
    return x


def _argmax_case(dtype, N, C, H, W, ld, rep, nchw, seed, special=False, pad=3):
    """``ld``: pixel stride of the NHWC rows; ``nchw``: an NCHW-contiguous tensor instead.  Returns (got, want, whole buffer, mask)"""
    L = _lib()
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    x = _scores(N, C, H, W, seed, special).to(tdt)
    if nchw:
        dev = x.cuda().contiguous()
        view = dev
    else:
        buf = torch.full((N, H, W, ld), 9.0, dtype=tdt).cuda()         # the padding channels hold a LARGER value: never read as scores
        buf[..., :C] = x.permute(0, 2, 3, 1).cuda()
        view = buf.permute(0, 3, 1, 2)[:, :C]
    LH, LW = H * rep[0], W * rep[1]
    ldh, ldn = LW + pad, (LH + 1) * (LW + pad)
    out = torch.full((N * ldn + 8,), SENT, dtype=torch.uint8, device="cuda")
    sn, sc, sh, sw = view.stride()
    _call("ydl_argmax_labels", L.YDL_F32 if dtype == "f32" else L.YDL_BF16, _ptr(view), sn, sc, sh, sw, N, C, H, W, rep[0], rep[1],
          _ptr(out), ldn, ldh)
    img = out[:N * ldn].reshape(N, LH + 1, ldh).cpu()
    mask = torch.zeros_like(img, dtype=torch.bool)
    mask[:, :LH, :LW] = True
    return img[:, :LH, :LW], R.argmax_labels(x, rep), torch.cat([img[~mask], out[N * ldn:].cpu()]), x


SHAPES = [(2, 5, 7), (1, 33, 65)]
LAYOUTS = [(12, 16), (5, 8), (1, 8), (32, 32)]            # (C, ld) of the NHWC rows


@pytest.mark.parametrize("rep", [(1, 1), (2, 2), (1, 3)])
@pytest.mark.parametrize("C,ld", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_argmax_nhwc(dtype, shape, C, ld, rep):
    N, H, W = shape
    got, want, outside, x = _argmax_case(dtype, N, C, H, W, ld, rep, False, 11 + C)
    assert torch.equal(got, want)
    assert bool((outside == SENT).all())
    if C > 1:
        top2 = x.float().topk(2, dim=1).values
        assert float((top2[:, 0] == top2[:, 1]).float().mean()) > 0.25          # ties are the common case, not the exception


@pytest.mark.parametrize("rep", [(1, 1), (2, 2), (1, 3)])
@pytest.mark.parametrize("shape", SHAPES)
def test_argmax_nchw_f32(shape, rep):
    N, H, W = shape
    got, want, outside, _ = _argmax_case("f32", N, 12, H, W, 0, rep, True, 5)
    assert torch.equal(got, want) and bool((outside == SENT).all())


@pytest.mark.parametrize("pad", [2, 4])
@pytest.mark.parametrize("rep", [(2, 2), (3, 4)])
def test_argmax_wide_stores(rep, pad):
    """row strides that are multiples of rep_w take the 2- / 4-byte stores, the others the byte stores: same labels, same guard"""
    got, want, outside, _ = _argmax_case("bf16", 2, 12, 5, 7, 16, rep, False, 3, pad=pad)
    assert torch.equal(got, want) and bool((outside == SENT).all())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nchw", [False, True])
def test_argmax_nan_and_infinities(dtype, nchw):
    got, want, outside, _ = _argmax_case(dtype, 2, 12, 5, 7, 16, (2, 2), nchw, 21, special=True)
    assert want[0, 0, 0] == 0 and want[0, 0, 2] == 1 and want[0, 0, 4] == 2 and want[0, 0, 6] == 1 and want[0, 2, 0] == 2
    assert torch.equal(got, want) and bool((outside == SENT).all())


def test_argmax_unaligned_rows_read_element_by_element():
    """sc == 1 but a pixel stride that is no multiple of 16 bytes (a channel slice at an odd offset): the scalar path, same labels"""
    L = _lib()
    x = _scores(2, 5, 5, 7, 31)
    buf = torch.full((2, 5, 7, 11), 9.0).cuda()
    buf[..., 3:8] = x.permute(0, 2, 3, 1).cuda()
    view = buf.permute(0, 3, 1, 2)[:, 3:8]
    out = torch.full((2 * 5 * 7,), SENT, dtype=torch.uint8, device="cuda")
    _call("ydl_argmax_labels", L.YDL_F32, _ptr(view), *view.stride(), 2, 5, 5, 7, 1, 1, _ptr(out), 35, 7)
    assert torch.equal(out.reshape(2, 5, 7).cpu(), R.argmax_labels(x))


def test_bad_arguments_are_refused_without_a_launch():
    L = _lib()
    lib = L.lib()
    x = torch.zeros(1, 4, 4, 40, device="cuda")
    out = torch.full((64,), SENT, dtype=torch.uint8, device="cuda")
    rc = lib.ydl_argmax_labels(L.YDL_F32, _ptr(x), 640, 1, 160, 40, 1, 33, 4, 4, 1, 1, _ptr(out), 16, 4, vp(0))
    assert rc != 0 and b"C <= 32" in lib.ydl_last_error()
    assert lib.ydl_argmax_labels(L.YDL_F32, _ptr(x), 640, 1, 160, 40, 1, 0, 4, 4, 1, 1, _ptr(out), 16, 4, vp(0)) != 0
    assert lib.ydl_argmax_labels(L.YDL_F16, _ptr(x), 640, 1, 160, 40, 1, 4, 4, 4, 1, 1, _ptr(out), 16, 4, vp(0)) != 0
    assert lib.ydl_argmax_labels(L.YDL_F32, _ptr(x), 640, 1, 160, 40, 1, 4, 4, 4, 2, 2, _ptr(out), 64, 7, vp(0)) != 0      # row stride < row
    assert lib.ydl_labels_resize(_ptr(out), 64, 8, 1, 0, 4, 4, 5, _ptr(out), 64, 8, 4, 4, vp(0)) != 0                     # box leaves the row
    assert lib.ydl_labels_resize(_ptr(out), 64, 8, 1, 0, 0, 0, 4, _ptr(out), 64, 8, 4, 4, vp(0)) != 0
    m = torch.zeros(33 * 33, dtype=torch.int64, device="cuda")
    assert lib.ydl_confusion_labels(_ptr(out), 16, 4, _ptr(out), 0, 16, 4, 1, 4, 4, 33, -1, _ptr(m), vp(0)) != 0
    assert lib.ydl_label_bincount(_ptr(out), 0, 16, 0, _ptr(m), vp(0)) != 0
    assert lib.ydl_labels_render(3, _ptr(out), None, None, _ptr(out), 4, _ptr(out), 1, 2, 2, 0, vp(0)) != 0
    assert lib.ydl_labels_render(1, _ptr(out), None, None, _ptr(out), 4, _ptr(out), 1, 2, 2, 0, vp(0)) != 0               # no target
    assert lib.ydl_labels_render(2, _ptr(out), None, None, _ptr(out), 4, _ptr(out), 1, 2, 2, 0, vp(0)) != 0               # no image
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and int(m.sum()) == 0


@pytest.mark.parametrize("C,ld", [(12, 16), (5, 8), (32, 32), (17, 24)])
# scales above 0.6 take the direct kernel, the others the tiled one (a 16 x 16 output tile blends from softmaxes kept in LDS):
# one tile, several tiles with ragged edges, a scale just under the threshold, a single source pixel
@pytest.mark.parametrize("sizes", [((9, 7), (5, 11)), ((33, 17), (4, 65)), ((7, 9), (11, 14)),
                                   ((6, 6), (15, 15)), ((13, 9), (40, 33)), ((10, 19), (17, 33)), ((1, 1), (3, 2))])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_softmax_resize_labels_equals_the_two_launches_it_replaces(dtype, sizes, C, ld):
    """ydl_softmax_resize_labels against ydl_softmax_fwd + ydl_resize_fwd (bilinear) at the C ABI and torch.argmax of their f32 result:
    the same arithmetic, so the same labels, near-ties included (scores on a coarse grid make many)"""
    L = _lib()
    (Hi, Wi), (Ho, Wo) = sizes
    N = 2
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    dt = L.YDL_F32 if dtype == "f32" else L.YDL_BF16
    g = torch.Generator().manual_seed(Hi * 100 + C)
    x = torch.full((N, Hi, Wi, ld), 9.0, dtype=tdt)
    x[..., :C] = (torch.randint(-8, 9, (N, Hi, Wi, C), generator=g).float() * 0.25).to(tdt)
    x = x.cuda()
    ldp = (C + 3) // 4 * 4
    p = torch.zeros((N, Hi, Wi, ldp), dtype=torch.float32, device="cuda")
    _call("ydl_softmax_fwd", dt, _ptr(x), ld, _ptr(p), Hi * Wi * ldp, 1, Wi * ldp, ldp, N, Hi, Wi, C, 1, 1)
    y = torch.zeros((N, Ho, Wo, ldp), dtype=torch.float32, device="cuda")
    _call("ydl_resize_fwd", L.YDL_F32, L.RESIZE_BILINEAR, _ptr(p), ldp, _ptr(y), ldp, N, Hi, Wi, Ho, Wo, C, 0.0, 0.0)
    want = y[..., :C].cpu().argmax(-1).to(torch.uint8)
    ldh, ldn = Wo + 3, (Ho + 1) * (Wo + 3)
    out = torch.full((N * ldn + 8,), SENT, dtype=torch.uint8, device="cuda")
    _call("ydl_softmax_resize_labels", dt, _ptr(x), ld, N, C, Hi, Wi, Ho, Wo, _ptr(out), ldn, ldh)
    img = out[:N * ldn].reshape(N, Ho + 1, ldh).cpu()
    assert torch.equal(img[:, :Ho, :Wo], want)
    mask = torch.zeros_like(img, dtype=torch.bool)
    mask[:, :Ho, :Wo] = True
    assert bool((img[~mask] == SENT).all()) and bool((out[N * ldn:] == SENT).all())
    lib = L.lib()
    assert lib.ydl_softmax_resize_labels(dt, _ptr(x), ld, N, 33, Hi, Wi, Ho, Wo, _ptr(out), ldn, ldh, vp(0)) != 0
    assert lib.ydl_softmax_resize_labels(dt, _ptr(x), ld, N, C, Hi, Wi, Ho, Wo, _ptr(out), ldn, Wo - 1, vp(0)) != 0


# ------------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("box,size", R.RESIZE_CASES)
def test_labels_resize(box, size):
    rs = np.random.RandomState(3)
    canvas = rs.randint(0, 200, size=(2, 16, 16)).astype(np.uint8)
    src = torch.full((2, 17, 19), SENT, dtype=torch.uint8)
    src[:, :16, :16] = torch.from_numpy(canvas)
    src = src.cuda()
    Ho, Wo = size
    ldh, ldn = Wo + 5, (Ho + 1) * (Wo + 5)
    out = torch.full((2 * ldn + 8,), SENT, dtype=torch.uint8, device="cuda")
    _call("ydl_labels_resize", _ptr(src), 17 * 19, 19, 2, *box, _ptr(out), ldn, ldh, Ho, Wo)
    img = out[:2 * ldn].reshape(2, Ho + 1, ldh).cpu()
    assert np.array_equal(img[:, :Ho, :Wo].numpy(), R.labels_resize(canvas, box, Ho, Wo))
    mask = torch.zeros_like(img, dtype=torch.bool)
    mask[:, :Ho, :Wo] = True
    assert bool((img[~mask] == SENT).all()) and bool((out[2 * ldn:] == SENT).all())


# ------------------------------------------------------------------------------------------------------ counting
def _label_pair(N, H, W, C, seed):
    rs = np.random.RandomState(seed)
    pred = rs.randint(0, C + 2, size=(N, H, W)).astype(np.uint8)               # predictions >= C among them
    target = rs.randint(0, C, size=(N, H, W)).astype(np.int64)
    target[0, 0, :3] = 255
    target[0, 1, :3] = C
    return pred, target


@pytest.mark.parametrize("ignore", [-1, 11, 3])
@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 7), (3, 33, 65)])               # 6435 pixels: more than one block's 256 threads, grid stride
def test_confusion_labels(shape, i64, ignore):
    C = 12
    pred, target = _label_pair(*shape, C, 40)
    if i64:
        target[0, 2, :3] = -1
        target[0, 3, 0] = -(1 << 40)
        target[0, 3, 1] = (1 << 32) + 2            # not class 2
    N, H, W = shape
    tt = torch.from_numpy(target if i64 else target.astype(np.uint8))
    # strided operands: rows of W + 3, images one row longer
    pbuf = torch.full((N, H + 1, W + 3), 1, dtype=torch.uint8)
    pbuf[:, :H, :W] = torch.from_numpy(pred)
    tbuf = torch.full((N, H + 1, W + 3), 1, dtype=tt.dtype)
    tbuf[:, :H, :W] = tt
    pbuf, tbuf = pbuf.cuda(), tbuf.cuda()
    start = torch.arange(C * C, dtype=torch.int64).reshape(C, C) * 1000          # accumulate into a non-zero matrix
    m = start.clone().cuda()
    _call("ydl_confusion_labels", _ptr(pbuf), (H + 1) * (W + 3), W + 3, _ptr(tbuf), int(i64), (H + 1) * (W + 3), W + 3, N, H, W, C,
          ignore, _ptr(m))
    want = R.confusion(pred, tt.numpy(), C, ignore)
    assert np.array_equal((m.cpu() - start).numpy(), want)
    assert want.sum() < N * H * W            # something was dropped


@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("n,nbins", [(35, 12), (6435, 12), (6435, 256), (1000, 1)])
def test_label_bincount(n, nbins, i64):
    rs = np.random.RandomState(n + nbins)
    v = rs.randint(0, min(nbins + 3, 256), size=n).astype(np.int64 if i64 else np.uint8)
    if i64:
        v[:4] = [-1, -(1 << 40), 1 << 33, 300]
    t = torch.from_numpy(v).cuda()
    start = torch.arange(nbins + 1, dtype=torch.int64) * 7
    counts = torch.cat([start, torch.full((3,), -5, dtype=torch.int64)]).cuda()
    _call("ydl_label_bincount", _ptr(t), int(i64), n, nbins, _ptr(counts))
    got = counts.cpu()
    assert np.array_equal((got[:nbins + 1] - start).numpy(), R.bincount(v, nbins))
    assert np.array_equal(R.bincount(v, nbins)[:nbins], np.bincount(v[(v >= 0) & (v < nbins)].astype(np.int64), minlength=nbins))
    assert got[nbins + 1:].tolist() == [-5, -5, -5]


# ------------------------------------------------------------------------------------------------------ pictures
def _render(mode, pred, target, img, pal, bgr):
    N, H, W = pred.shape
    out = torch.full((N * H * W * 3 + 16,), SENT, dtype=torch.uint8, device="cuda")
    p, pl = torch.from_numpy(pred).cuda(), torch.from_numpy(pal).cuda()
    t = torch.from_numpy(target).cuda() if target is not None else None
    im = torch.from_numpy(img).cuda() if img is not None else None
    _call("ydl_labels_render", mode, _ptr(p), _ptr(t), _ptr(im), _ptr(pl), len(pal), _ptr(out), N, H, W, int(bgr))
    assert bool((out[N * H * W * 3:] == SENT).all())
    return out[:N * H * W * 3].reshape(N, H, W, 3).cpu().numpy()


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_render_modes(mode, bgr):
    rs = np.random.RandomState(50 + mode)
    N, H, W, K = 2, 33, 65, 12
    pal = rs.randint(0, 256, size=(K, 3)).astype(np.uint8)
    gt = rs.randint(0, K + 3, size=(N, H, W)).astype(np.uint8)                 # labels >= npal among them
    pred = np.where(rs.rand(N, H, W) < 0.5, gt, rs.randint(0, K + 3, size=(N, H, W))).astype(np.uint8)
    # pixel values k/255 +- a little, and exact halves after the blend: both rounding directions and ties occur
    img = ((rs.randint(0, 256, size=(N, 3, H, W)) + rs.choice([0.0, 0.4, 0.999], size=(N, 3, H, W))) / 255.0).astype(np.float32)
    img[0, :, 0, :4] = [[0.0, 1.0, 1.5, -0.25]] * 3                            # the ends of the range and beyond them
    got = _render(mode, pred, gt if mode == 1 else None, img if mode == 2 else None, pal, bgr)
    if mode == 0:
        want = R.colorize(pred, pal)
    elif mode == 1:
        want = R.difference(gt, pred, pal)
    else:
        want = np.stack([R.overlay(img[n], pred[n], pal, bgr) for n in range(N)])
        halves = (np.float32(0.5) * (img[:, 0] * np.float32(255)).clip(0, 255).astype(np.uint8) + 0.5 * R.colorize(pred, pal)[..., 2 if bgr else 0])
        assert (halves % 1 == 0.5).mean() > 0.2
    assert np.array_equal(got, want)


def test_render_equals_the_reference_recordings():
    g = np.load(os.path.join(GOLDEN, "predict_render.npz"))
    pal = g["palette"]
    for c in (0, 1):
        gt, pred = g[f"c{c}/gt"][None], g[f"c{c}/pred"][None]
        assert np.array_equal(_render(0, pred, None, None, pal, False)[0], g[f"c{c}/colour"])
        assert np.array_equal(_render(1, pred, gt, None, pal, False)[0], g[f"c{c}/difference"])
