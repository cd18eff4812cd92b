"""float64 restatement of the bicubic resize of csrc/spatial.hip (ydl_bicubic_fwd / ydl_bicubic_bwd), its bounds and its
cases, in the scheme of tests/spatial_ref.py (Layout, sentinels, check_rounded: imported, not restated).  numpy on the CPU only; nothing
of yolo_dual_amd is imported.  Tensors are NHWC.  tests/test_up_ref_cpu.py holds every expression here to F.interpolate(mode='bicubic')
and its autograd in float64; tests/test_gpu_bicubic.py compares the kernels with them.

The arithmetic is ATen's upsample_bicubic2d with A = -0.75:
  scale   as for bilinear: 1 / scale_factor when one was given, else in / out; align_corners: (in - 1) / (out - 1), 0 when out == 1
  src     scale * (dst + 0.5) - 0.5, NOT clamped at 0 (bilinear clamps); align_corners: scale * dst
  i, t    floor(src), src - i
  taps    i - 1 .. i + 2, each clamped to [0, in - 1]
  c0      ((A (t + 1) - 5 A) (t + 1) + 8 A) (t + 1) - 4 A        c1   ((A + 2) t - (A + 3)) t t + 1
  c2      c1 evaluated at 1 - t                                   c3   c0's cubic evaluated at (1 - t) + 1
Index and coefficient arithmetic is available op by op in float32 (numpy rounds every float32 operation separately), which is what the
kernel does with explicit round-to-nearest operations; ``dtype=F64`` gives what F.interpolate(float64) uses."""
import numpy as np

from tests import spatial_ref as R

U, BF16, F32, F64 = R.U, R.BF16, R.F32, R.F64
A_ATEN = -0.75
FWD_DEPTH = 10          # roundings on the path of one term of the 4 x 4 sum: see bicubic_fwd_bound
BWD_CONST = 8           # roundings of one term of the backward sum before the additions over the outputs: see bicubic_bwd_bound


def cub_scale(align, n_in, n_out, given=0.0, dtype=F32):
    if align:
        return dtype(n_in - 1) / dtype(n_out - 1) if n_out > 1 else dtype(0)
    if given > 0:
        return dtype(given)
    return dtype(n_in) / dtype(n_out)


def cubic1(x, A, dtype):
    """((A + 2) x - (A + 3)) x x + 1, one rounding per operation"""
    x = np.asarray(x, dtype=dtype)
    return ((((dtype(A + 2) * x).astype(dtype) - dtype(A + 3)).astype(dtype) * x).astype(dtype) * x).astype(dtype) + dtype(1)


def cubic2(x, A, dtype):
    """((A x - 5 A) x + 8 A) x - 4 A, one rounding per operation"""
    x = np.asarray(x, dtype=dtype)
    v = ((dtype(A) * x).astype(dtype) - dtype(5 * A)).astype(dtype)
    v = ((v * x).astype(dtype) + dtype(8 * A)).astype(dtype)
    return ((v * x).astype(dtype) - dtype(4 * A)).astype(dtype)


def cub_src(n_out, scale, align, dtype=F32, clamp0=False):
    """-> (floor(src) as int64, t = src - floor(src)) for every destination index of one axis.  clamp0: clamp src at 0 the way the
    bilinear path does (a WRONG answer for bicubic, for tests)"""
    dst = np.arange(n_out, dtype=dtype)
    scale = dtype(scale)
    if align:
        src = (scale * dst).astype(dtype)
    else:
        src = ((scale * (dst + dtype(0.5))).astype(dtype) - dtype(0.5)).astype(dtype)
        if clamp0:
            src = np.where(src < 0, dtype(0), src).astype(dtype)
    fl = np.floor(src).astype(dtype)
    return fl.astype(np.int64), (src - fl).astype(dtype)


def cub_taps(align, n_in, n_out, given=0.0, dtype=F32, A=A_ATEN, clamp0=False, wrap=False):
    """-> (idx int64 [n_out, 4], coefficients dtype [n_out, 4]) of one axis.  A, clamp0, wrap (border taps wrap around instead of
    clamping) select wrong answers for tests"""
    i, t = cub_src(n_out, cub_scale(align, n_in, n_out, given, dtype), align, dtype, clamp0)
    u = (dtype(1) - t).astype(dtype)
    c = np.stack([cubic2((t + dtype(1)).astype(dtype), A, dtype), cubic1(t, A, dtype), cubic1(u, A, dtype),
                  cubic2((u + dtype(1)).astype(dtype), A, dtype)], axis=1).astype(dtype)
    idx = i[:, None] + np.arange(-1, 3)[None, :]
    idx = np.mod(idx, n_in) if wrap else np.clip(idx, 0, n_in - 1)
    return idx, c


def bicubic_fwd_ref(x, th, tw, dtype=F64):
    """y[n, ho, wo] = sum_a ch[a] (sum_b cw[b] x[ih_a, iw_b]): the kernel's separable form, rows and columns in tap order, evaluated in
    ``dtype`` with the coefficients of th / tw; also sum |ch[a] cw[b] x| of each element's own sixteen taps"""
    x = np.asarray(x, dtype=dtype)
    ih, ch = th
    iw, cw = tw
    ch, cw = np.asarray(ch, dtype=dtype), np.asarray(cw, dtype=dtype)
    N, Hi, Wi, C = x.shape
    y = np.zeros((N, len(ih), len(iw), C), dtype=dtype)
    mag = np.zeros(y.shape, dtype=F64)
    xa = np.abs(x).astype(F64)
    for a in range(4):
        rows, ra = x[:, ih[:, a]], xa[:, ih[:, a]]                      # (N, Ho, Wi, C)
        rs = np.zeros(y.shape, dtype=dtype)
        rm = np.zeros(y.shape, dtype=F64)
        for b in range(4):
            rs = (rs + (cw[None, None, :, b, None] * rows[:, :, iw[:, b]]).astype(dtype)).astype(dtype)
            rm += np.abs(cw[None, None, :, b, None].astype(F64)) * ra[:, :, iw[:, b]]
        y = (y + (ch[None, :, a, None, None] * rs).astype(dtype)).astype(dtype)
        mag += np.abs(ch[None, :, a, None, None].astype(F64)) * rm
    return y, mag


def _piles(idx, c, dtype):
    """the weight every input index carries in one output: {index: (sum of its coefficients in tap order, sum of their magnitudes)};
    clamped border taps pile onto 0 and in - 1"""
    out = {}
    for j in range(4):
        w, m = out.get(int(idx[j]), (dtype(0), 0.0))
        out[int(idx[j])] = (dtype(w + dtype(c[j])), m + abs(float(c[j])))
    return out


def bicubic_bwd_ref(dy, th, tw, Hi, Wi, prev=None, dtype=F64):
    """the explicit transpose of bicubic_fwd_ref: loop over outputs, scatter-add (wh ww) dy with wh, ww the piled weights.  -> (dx,
    sum (sum |ch|)(sum |cw|) |dy| per input element, number of outputs that contribute with a non-zero weight).  In float32 the
    kernel's order: previous contents first, outputs rows outer, columns inner, ascending"""
    dy = np.asarray(dy, dtype=dtype)
    N, Ho, Wo, C = dy.shape
    ih, ch = th
    iw, cw = tw
    dx = np.zeros((N, Hi, Wi, C), dtype=dtype) if prev is None else np.array(prev, dtype=dtype)
    mag = np.zeros((N, Hi, Wi, C), dtype=F64)
    cnt = np.zeros((Hi, Wi), dtype=np.int64)
    cols = [_piles(iw[wo], cw[wo], dtype) for wo in range(Wo)]
    for ho in range(Ho):
        rows = _piles(ih[ho], ch[ho], dtype)
        for wo in range(Wo):
            for i, (wh, mh) in rows.items():
                if wh == 0:
                    continue
                for j, (ww, mw) in cols[wo].items():
                    if ww == 0:
                        continue
                    wgt = dtype(wh * ww)
                    dx[:, i, j] = (dx[:, i, j] + (wgt * dy[:, ho, wo]).astype(dtype)).astype(dtype)
                    mag[:, i, j] += mh * mw * np.abs(dy[:, ho, wo]).astype(F64)
                    cnt[i, j] += 1
    return dx, mag, cnt


def bicubic_fwd_bound(mag, ref, bf16):
    """one term ch[a] cw[b] x of the 4 x 4 sum passes the product with cw, at most four additions of the row sum, the product with ch
    and at most four additions of the column sum: FWD_DEPTH = 10 roundings (a fused multiply-add has fewer), each at most U of the
    partial sum it rounds, which the element's own sum |ch cw x| bounds (sum |c| <= 1.375 per axis, so it is at most 1.9 max |x|);
    1e-6 covers the second-order terms.  One bf16 store."""
    return FWD_DEPTH * U * (1 + 1e-6) * mag + (BF16 * np.abs(ref) if bf16 else 0.0)


def bicubic_bwd_bound(mag, cnt, ref, prev, bf16):
    """like spatial_ref.resize_bwd_bound: a term (wh ww) dy carries the at most three additions of each piled weight (relative to the
    sum of the coefficients' magnitudes, which is what ``mag`` holds), the product wh * ww and the product with dy: BWD_CONST = 8;
    then one addition per contributing output.  The previous contents enter every partial sum: (outputs) U |prev|.  One bf16 store."""
    cnt = np.asarray(cnt, dtype=F64)[None, :, :, None]
    b = (cnt + BWD_CONST) * U * (1 + 1e-6) * mag
    if prev is not None:
        b = b + cnt * U * np.abs(np.asarray(prev, dtype=F64))
    return b + (BF16 * np.abs(ref) if bf16 else 0.0)


def case_bicubic(x, align, Ho, Wo, dtype, ld=None, gh=0.0, gw=0.0, lead=R.LEAD):
    """inputs as the kernel reads them (already rounded to the storage type), float64 reference on the kernel's float32 taps, bound,
    float32 floor, Layout"""
    x = R.store(x, dtype)
    N, Hi, Wi, C = x.shape
    Cp = R.rup(C, R.vec(dtype))
    th, tw = cub_taps(align, Hi, Ho, gh), cub_taps(align, Wi, Wo, gw)
    ref, mag = bicubic_fwd_ref(x.astype(F64), th, tw)
    f32, _ = bicubic_fwd_ref(x, th, tw, F32)
    return dict(layout=R.Layout(N * Ho * Wo, ld or Cp, C, Cp, "free", lead), x=x, th=th, tw=tw, ref=ref, mag=mag,
                bound=bicubic_fwd_bound(mag, ref, dtype == "bf16"), floor=R.store(f32, dtype))


def case_bicubic_bwd(dy, align, Hi, Wi, dtype, prev=None, ld=None, gh=0.0, gw=0.0, lead=R.LEAD):
    dy = R.store(dy, dtype)
    prev = None if prev is None else R.store(prev, dtype)
    N, Ho, Wo, C = dy.shape
    Cp = R.rup(C, R.vec(dtype))
    th, tw = cub_taps(align, Hi, Ho, gh), cub_taps(align, Wi, Wo, gw)
    ref, mag, cnt = bicubic_bwd_ref(dy.astype(F64), th, tw, Hi, Wi, None if prev is None else prev.astype(F64))
    f32 = bicubic_bwd_ref(dy, th, tw, Hi, Wi, prev, dtype=F32)[0]
    return dict(layout=R.Layout(N * Hi * Wi, ld or Cp, C, Cp, "free", lead), dy=dy, prev=prev, th=th, tw=tw, ref=ref, mag=mag, cnt=cnt,
                bound=bicubic_bwd_bound(mag, cnt, ref, prev, dtype == "bf16"), floor=R.store(f32, dtype))


check_bicubic = check_bicubic_bwd = R.check_rounded
