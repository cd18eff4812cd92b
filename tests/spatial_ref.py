"""float64 restatements of the pooling, resize, gate, layout and transport kernels (csrc/spatial.hip, the group soft-max / casts /
chunk reduction of csrc/dcn_blocks.hip, bn_eval_coeffs of csrc/bn.hip), their bounds and their comparison helpers.  numpy / torch on
the CPU only; nothing of yolo_dual_amd is imported.  Tensors are NHWC.  tests/test_spatial_ref_cpu.py holds every expression here to
torch's float64 operators and autograd; tests/test_gpu_spatial_f64.py compares the kernels with them.

A comparison helper is a function check_<family>(got, case) -> (error, floor, bound).  ``got`` is the WHOLE buffer the answer lives in
(a plain array: leading sentinels, rows of ``ld`` elements, slack), ``case`` carries the Layout, the float64 reference, the per-element
bound and the same reference evaluated in float32 (the floor).  The answer passes iff error <= bound; the floor must pass too.
  exact families     error = number of elements that differ from the reference to the bit, sentinels and pad channels included;
                     floor = bound = 0
  rounded families   the bound is per element; error = the largest |got - ref| / bound_i, scaled to the smallest non-zero bound_i,
                     which is what is returned as ``bound`` (so for a uniform bound error is the plain largest error); an element
                     whose bound is 0 must be met exactly; a sentinel or pad channel violation makes error infinite
Bounds are sums of named terms in units of U = 2^-24 (float32 unit roundoff) plus, for a bf16 store, BF16 = 2^-8 relative (the
convention of tests/census.py)."""
import math

import numpy as np
import torch

U = 2.0 ** -24
BF16 = 2.0 ** -8
SENT = -24576.0         # -1.5 * 2^14: exact in f32 and bf16, far outside every output's range
LEAD = 16               # sentinel elements in front of every view (a multiple of 8: 16-byte alignment is kept in both types)
SLACK = 64
EXPF = 4 * U            # __expf: see softmax_rel_bound
F32, F64 = np.float32, np.float64


def rup(c, v):
    return (c + v - 1) // v * v


def bf16_round(a):
    """round-to-nearest-even to bf16, returned as float32 (torch's .bfloat16())"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).bfloat16().float().numpy()


def store(a, dtype):
    """the value a kernel stores for the float32 number ``a``"""
    return bf16_round(a) if dtype == "bf16" else np.asarray(a, dtype=F32)


# ---------------------------------------------------------------------------------------------------------------------------
# buffers with sentinels
# ---------------------------------------------------------------------------------------------------------------------------
class Layout:
    """``rows`` rows of ``ld`` elements starting ``lead`` elements into a buffer; the answer is columns [0, C); columns [C, Cw) are pad
    channels the kernel writes (pad = "zero": they must be 0; "free": whatever the kernel made of its input's pad channels);
    everything else must keep the sentinel"""

    def __init__(self, rows, ld, C, Cw=None, pad="free", lead=LEAD, slack=SLACK):
        self.rows, self.ld, self.C, self.Cw, self.pad, self.lead, self.slack = rows, ld, C, (C if Cw is None else Cw), pad, lead, slack
        assert self.C <= self.Cw <= ld
        self.size = lead + rows * ld + slack

    def canvas(self, dtype=F32, fill=SENT):
        return np.full(self.size, fill, dtype=dtype)

    def rows_of(self, buf):
        return buf[self.lead:self.lead + self.rows * self.ld].reshape(self.rows, self.ld)

    def embed(self, values, dtype=F32, pad_value=0.0, fill=SENT):
        buf = self.canvas(dtype, fill)
        r = self.rows_of(buf)
        r[:, :self.C] = np.asarray(values).reshape(self.rows, self.C)
        r[:, self.C:self.Cw] = pad_value
        return buf

    def violations(self, buf, sent=SENT):
        """number of elements outside the answer that are not what they must be"""
        buf = np.asarray(buf)
        assert buf.size == self.size
        r = self.rows_of(buf)
        bad = int((buf[:self.lead] != sent).sum()) + int((buf[self.lead + self.rows * self.ld:] != sent).sum())
        bad += int((r[:, self.Cw:] != sent).sum())
        if self.pad == "zero":
            bad += int((r[:, self.C:self.Cw] != 0).sum())
        return bad

    def answer(self, buf):
        return self.rows_of(np.asarray(buf))[:, :self.C]


def _bits_differ(a, b):
    """number of elements where a and b differ; NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        a, b = a.astype(F64), b.astype(F64)
        return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())
    return int((a != b).sum())


def check_exact(got, case):
    """exact families (max pool, nearest resize, copy2d, layout, zero fills, casts, chunk reduction, global max / arg-max and the
    global pool backward on dyadic data): case = dict(layout, ref [, sent])"""
    lay = case["layout"]
    sent = case.get("sent", SENT)
    bad = lay.violations(got, sent) + _bits_differ(lay.answer(got), np.asarray(case["ref"]).reshape(lay.rows, lay.C))
    return float(bad), 0.0, 0.0


check_maxpool = check_nearest = check_copy2d = check_layout = check_zero = check_cast = check_reduce = check_global_max = check_exact


def _worst(err, bound):
    """-> (largest err_i / bound_i scaled to the smallest non-zero bound, that bound)"""
    err, bound = np.asarray(err, dtype=F64), np.broadcast_to(np.asarray(bound, dtype=F64), np.shape(err))
    pos = bound > 0
    bmin = float(bound[pos].min()) if pos.any() else 0.0
    ratio = 0.0
    if pos.any():
        ratio = float((err[pos] / bound[pos]).max())
    if (~pos).any() and float(err[~pos].max()) > 0:
        ratio = math.inf
    if np.isnan(err).any():
        ratio = math.inf
    return (ratio * bmin if bmin > 0 else ratio), bmin


def check_rounded(got, case):
    """rounded families: case = dict(layout, ref (float64), bound (per element or scalar), floor (the reference in float32, already
    stored as the kernel stores it))"""
    lay = case["layout"]
    ref = np.asarray(case["ref"], dtype=F64).reshape(lay.rows, lay.C)
    bound = np.broadcast_to(np.asarray(case["bound"], dtype=F64), ref.shape) if np.ndim(case["bound"]) == 0 else \
        np.asarray(case["bound"], dtype=F64).reshape(lay.rows, lay.C)
    floor, bmin = _worst(np.abs(np.asarray(case["floor"], dtype=F64).reshape(lay.rows, lay.C) - ref), bound)
    if lay.violations(got, case.get("sent", SENT)):
        return math.inf, floor, bmin
    error, _ = _worst(np.abs(lay.answer(got).astype(F64) - ref), bound)
    return error, floor, bmin


check_bilinear = check_resize_bwd = check_acc_sums = check_global_avg = check_channel_dot = check_scale_channels = check_rounded
check_gate = check_group_softmax = check_bn_eval = check_rounded


def accepted(res):
    error, floor, bound = res
    return error <= bound


# ---------------------------------------------------------------------------------------------------------------------------
# max pool
# ---------------------------------------------------------------------------------------------------------------------------
def pool_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def maxpool_ref(x, k, s, p, last_tie=False):
    """x (N, H, W, C) -> (values, codes ky * k + kx of the FIRST maximum in scan order) with ATen's update rule: the first tap inside
    the image initialises, then ``v > best or isnan(v)``.  last_tie: break ties towards the last maximum (a wrong answer for tests)"""
    x = np.asarray(x)
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H, k, s, p), pool_out(W, k, s, p)
    best = np.full((N, Ho, Wo, C), -np.inf, dtype=x.dtype)
    code = np.zeros((N, Ho, Wo, C), dtype=np.uint8)
    first = np.ones((N, Ho, Wo, 1), dtype=bool)
    for ky in range(k):
        ih = np.arange(Ho) * s - p + ky
        vh = (ih >= 0) & (ih < H)
        for kx in range(k):
            iw = np.arange(Wo) * s - p + kx
            vw = (iw >= 0) & (iw < W)
            valid = (vh[:, None] & vw[None, :])[None, :, :, None]
            v = x[:, np.clip(ih, 0, H - 1)][:, :, np.clip(iw, 0, W - 1)]
            with np.errstate(invalid="ignore"):
                upd = valid & (first | (v >= best if last_tie else v > best) | np.isnan(v))
            best = np.where(upd, v, best)
            code = np.where(upd, np.uint8(ky * k + kx), code)
            first = first & ~valid
    return best, code


def maxpool_bwd_ref(dy, code, H, W, k, s, p, prev=None):
    """scatter of dy (N, Ho, Wo, C) by code into (N, H, W, C), float64; prev: previous contents (the accumulate form)"""
    dy = np.asarray(dy, dtype=F64)
    N, Ho, Wo, C = dy.shape
    dx = np.zeros((N, H, W, C), dtype=F64) if prev is None else np.array(prev, dtype=F64)
    for ky in range(k):
        ih = np.arange(Ho) * s - p + ky
        ho = np.nonzero((ih >= 0) & (ih < H))[0]
        for kx in range(k):
            iw = np.arange(Wo) * s - p + kx
            wo = np.nonzero((iw >= 0) & (iw < W))[0]
            if ho.size == 0 or wo.size == 0:
                continue
            sel = np.ix_(np.arange(N), ho, wo)
            contrib = np.where(code[sel] == ky * k + kx, dy[sel], 0.0)
            dx[np.ix_(np.arange(N), ih[ho], iw[wo])] += contrib          # distinct targets within one (ky, kx)
    return dx


# ---------------------------------------------------------------------------------------------------------------------------
# resize: source indices and weights, op by op in float32 (numpy rounds every float32 operation separately)
# ---------------------------------------------------------------------------------------------------------------------------
def axis_scale(mode, n_in, n_out, given=0.0):
    if mode == 2:
        return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    if given > 0:
        return F32(given)
    return F32(n_in) / F32(n_out)


def lin_src(n_out, scale, n_in, align):
    """-> (i0, i1, w0, w1) for every destination index of one axis (lin_src of csrc/spatial.hip, ATen's float path)"""
    dst = np.arange(n_out, dtype=F32)
    scale = F32(scale)
    if align:
        src = scale * dst
    else:
        src = scale * (dst + F32(0.5)) - F32(0.5)
        src = np.where(src < 0, F32(0), src).astype(F32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    w1 = (src - i0.astype(F32)).astype(F32)
    w0 = (F32(1) - w1).astype(F32)
    return i0, i1, w0, w1


def near_src(n_out, scale, n_in):
    v = np.floor(np.arange(n_out, dtype=F32) * F32(scale)).astype(np.int64)
    return np.minimum(v, n_in - 1)


def axis_taps(mode, n_in, n_out, given=0.0):
    """the two taps of every destination index: nearest is (i, i, 1, 0)"""
    sc = axis_scale(mode, n_in, n_out, given)
    if mode == 0:
        i = near_src(n_out, sc, n_in)
        return i, i.copy(), np.ones(n_out, dtype=F32), np.zeros(n_out, dtype=F32)
    return lin_src(n_out, sc, n_in, mode == 2)


def exact_taps(mode, n_in, n_out, given=0.0):
    """the bilinear taps with source coordinate and weights in float64 (what F.interpolate(float64) uses)"""
    dst = np.arange(n_out, dtype=F64)
    if mode == 2:
        sc = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        src = sc * dst
    else:
        sc = float(given) if given > 0 else n_in / n_out
        src = np.maximum(sc * (dst + 0.5) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    w1 = src - i0
    return i0, i1, 1.0 - w1, w1


def resize_fwd_ref(x, th, tw, dtype=F64):
    """y[n, ho, wo] = wh0 (ww0 x[h0, w0] + ww1 x[h0, w1]) + wh1 (ww0 x[h1, w0] + ww1 x[h1, w1]), the kernel's two-level combination,
    evaluated in ``dtype`` with the float32 weights of th / tw (axis_taps); also sum w |v| of each element's own four taps"""
    x = np.asarray(x, dtype=dtype)
    h0, h1, a0, a1 = th
    w0, w1, b0, b1 = tw
    a0, a1 = np.asarray(a0, dtype=dtype)[None, :, None, None], np.asarray(a1, dtype=dtype)[None, :, None, None]
    b0, b1 = np.asarray(b0, dtype=dtype)[None, None, :, None], np.asarray(b1, dtype=dtype)[None, None, :, None]
    r0, r1 = x[:, h0], x[:, h1]
    y = a0 * (b0 * r0[:, :, w0] + b1 * r0[:, :, w1]) + a1 * (b0 * r1[:, :, w0] + b1 * r1[:, :, w1])
    r0, r1 = np.abs(r0).astype(F64), np.abs(r1).astype(F64)
    mag = a0.astype(F64) * (b0.astype(F64) * r0[:, :, w0] + b1.astype(F64) * r0[:, :, w1]) + \
        a1.astype(F64) * (b0.astype(F64) * r1[:, :, w0] + b1.astype(F64) * r1[:, :, w1])
    return y, mag


def resize_bwd_ref(dy, th, tw, Hi, Wi, prev=None, dtype=F64):
    """the explicit transpose of resize_fwd_ref: loop over outputs, scatter-add w * dy.  -> (dx, sum |w dy| per input element, number
    of outputs that contribute to it with a non-zero weight).  dtype float32: products and additions in float32, in the order of the
    kernel (rows outer, columns inner, ascending; previous contents first)"""
    dy = np.asarray(dy, dtype=dtype)
    N, Ho, Wo, C = dy.shape
    h0, h1, a0, a1 = th
    w0, w1, b0, b1 = tw
    dx = np.zeros((N, Hi, Wi, C), dtype=dtype) if prev is None else np.array(prev, dtype=dtype)
    mag = np.zeros((N, Hi, Wi, C), dtype=F64)
    cnt = np.zeros((Hi, Wi), dtype=np.int64)
    for ho in range(Ho):
        # weight of input row ih for this output row, as the kernel re-derives it: (i0 == ih ? w0 : 0) + (i1 == ih ? w1 : 0)
        rows = {}
        for i, w in ((h0[ho], a0[ho]), (h1[ho], a1[ho])):
            rows[int(i)] = dtype(rows.get(int(i), dtype(0)) + dtype(w))
        for wo in range(Wo):
            cols = {}
            for i, w in ((w0[wo], b0[wo]), (w1[wo], b1[wo])):
                cols[int(i)] = dtype(cols.get(int(i), dtype(0)) + dtype(w))
            for ih, wh in rows.items():
                if wh == 0:
                    continue
                for iw, ww in cols.items():
                    if ww == 0:
                        continue
                    wgt = dtype(wh * ww)
                    dx[:, ih, iw] += wgt * dy[:, ho, wo]
                    mag[:, ih, iw] += float(wgt) * np.abs(dy[:, ho, wo]).astype(F64)
                    cnt[ih, iw] += 1
    return dx, mag, cnt


def bilinear_fwd_bound(mag, ref, bf16):
    """the two-level combination: two products and one addition per row pair, one product and one addition across: at most 6 U of the
    element's own sum w |v|"""
    return 6 * U * mag + (BF16 * np.abs(ref) if bf16 else 0.0)


def resize_bwd_bound(mag, cnt, ref, prev, bf16):
    """(contributing outputs + 3) U of sum |w dy| (wh * ww, the product with dy, one addition per output), the previous contents enter
    every partial sum: (outputs) U |prev|; one bf16 store"""
    cnt = np.asarray(cnt, dtype=F64)[None, :, :, None]
    b = (cnt + 3) * U * mag
    if prev is not None:
        b = b + cnt * U * np.abs(np.asarray(prev, dtype=F64))
    return b + (BF16 * np.abs(ref) if bf16 else 0.0)


def interpolate_gap_bound(x, mode, Hi, Wi, Ho, Wo, gh=0.0, gw=0.0):
    """|restated bilinear (float32 weights) - exact bilinear (float64 weights)| per output element.  The float32 source coordinate
    scale * (dst + 0.5) - 0.5 carries three roundings (the scale, the product, the subtraction; dst + 0.5 is exact), each of
    at most U times the magnitude (in-1 at most, +0.5), and w1 = src - i0 is exact (Sterbenz), w0 = 1 - w1 one more rounding of a
    number <= 1: |dw| <= (3 (in + 0.5) + 1) U per axis.  A weight error dw moves the result by dw * |difference of the two taps| <=
    dw * 2 max|x|, one axis at a time"""
    m = float(np.abs(np.asarray(x, dtype=F64)).max())
    dwh = (3 * (Hi + 0.5) + 1) * U
    dww = (3 * (Wi + 0.5) + 1) * U
    return 2 * m * (dwh + dww)


# ---------------------------------------------------------------------------------------------------------------------------
# global average / max
# ---------------------------------------------------------------------------------------------------------------------------
def global_pool_ref(x, dtype=F64, last_tie=False, div=None):
    """x (N, HW, C) -> (avg, max, arg-max = FIRST maximum in pixel order; a NaN wins and the LAST NaN stays, as ATen's
    ``v > best or isnan(v)`` scan leaves it)"""
    x = np.asarray(x)
    N, HW, C = x.shape
    avg = (x.astype(dtype).sum(1) / dtype(HW if div is None else div)).astype(dtype)
    nan = np.isnan(x)
    if last_tie:
        am = HW - 1 - np.flip(np.where(nan, -np.inf, x), 1).argmax(1)
    else:
        am = np.where(nan, -np.inf, x).argmax(1)
    last_nan = HW - 1 - np.flip(nan, 1).argmax(1)
    am = np.where(nan.any(1), last_nan, am)
    mx = np.take_along_axis(x, am[:, None, :], 1)[:, 0]
    return avg, mx, am.astype(np.int32)


def global_pool_bwd_ref(davg, dmx, amax, HW, prev=None, dtype=F64):
    """dx[n, p, c] = prev + davg[n, c] / HW + (p == amax[n, c]) dmx[n, c];  davg or dmx may be None.  In float32 the kernel's order:
    prev, then davg * (1 / HW), then dmx"""
    amax = np.asarray(amax)
    N, C = amax.shape
    dx = np.zeros((N, HW, C), dtype=dtype) if prev is None else np.array(prev, dtype=dtype)
    if davg is not None:
        inv = dtype(1) / dtype(HW)
        dx = (dx + (np.asarray(davg, dtype=dtype) * inv)[:, None, :]).astype(dtype)
    if dmx is not None:
        hit = np.arange(HW)[None, :, None] == amax[:, None, :]
        dx = np.where(hit, dx + np.asarray(dmx, dtype=dtype)[:, None, :], dx).astype(dtype)
    return dx


def global_avg_bound(x, bf16):
    """depth: ceil(HW / 256) - 1 additions in a thread, 256 in the merge, the division; times sum |x| / HW"""
    x = np.asarray(x, dtype=F64)
    HW = x.shape[1]
    depth = (math.ceil(HW / 256) - 1) + 256 + 1
    b = depth * U * np.abs(x).sum(1) / HW
    return b + (BF16 * np.abs(x.sum(1) / HW) if bf16 else 0.0)


def thread_partials(t, nthreads=256):
    """t (N, HW, C) float32 -> (N, nthreads, C): thread i adds elements i, i + nthreads, ... in that order, in float32"""
    t = np.asarray(t, dtype=F32)
    N, HW, C = t.shape
    T = -(-HW // nthreads)
    pad = np.zeros((N, T * nthreads, C), dtype=F32)             # adding zeros is exact
    pad[:, :HW] = t
    return np.cumsum(pad.reshape(N, T, nthreads, C), axis=1, dtype=F32)[:, -1]


def seq_sum(parts):
    return np.cumsum(np.asarray(parts, dtype=F32), axis=1, dtype=F32)[:, -1]


def tree_sum(parts):
    """halving tree over axis 1 in float32 (log2 levels; the length is padded with zeros to a power of two)"""
    parts = np.asarray(parts, dtype=F32)
    n = 1
    while n < parts.shape[1]:
        n *= 2
    pad = np.zeros((parts.shape[0], n) + parts.shape[2:], dtype=F32)
    pad[:, :parts.shape[1]] = parts
    while n > 1:
        n //= 2
        pad = (pad[:, :n] + pad[:, n:2 * n]).astype(F32)
    return pad[:, 0]


def global_avg_f32(x):
    """the float32 floor in the kernel's own shape: 256 strided partial sums, merged one after the other, one division"""
    return (seq_sum(thread_partials(x)) / F32(np.shape(x)[1])).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# small expressions
# ---------------------------------------------------------------------------------------------------------------------------
def sigmoid_ref(z, dtype=F64):
    z = np.asarray(z, dtype=dtype)
    with np.errstate(over="ignore"):
        return (dtype(1) / (dtype(1) + np.exp(-z))).astype(dtype)


def gate_fwd_ref(a, b, dtype=F64):
    return sigmoid_ref(np.asarray(a, dtype=dtype) + np.asarray(b, dtype=dtype), dtype)


def gate_fwd_bound(a, b):
    """sigmoid_f(z) = rcp(1 + exp2(-log2(e) z)), z = a + b.  Relative error of the result: the rounding of z and of the scaling enter
    the exponent, |z| (2 U) + U (the rounded constant) relative on e = exp(-z), then 1 ulp (2 U) of v_exp_f32, all weighted by
    e / (1 + e) <= 1; the addition U; v_rcp_f32 1 ulp (2 U).  (1 - g) z <= 1 bounds the exponent's share: g' / g = 1 - g.)
    Where exp2 underflows or the sum overflows the result saturates to 1 or 0 exactly like the reference rounded to float32, up to
    the smallest normal number: an absolute 2^-126 is added."""
    z = np.abs(np.asarray(a, dtype=F64) + np.asarray(b, dtype=F64))
    g = sigmoid_ref(np.asarray(a, dtype=F64) + np.asarray(b, dtype=F64))
    rel = (1 - g) * (3 * z * U + 2 * U) + U + 2 * U + U
    return rel * g + 2.0 ** -126


def gate_bwd_ref(gate, dgate, dtype=F64):
    g, d = np.asarray(gate, dtype=dtype), np.asarray(dgate, dtype=dtype)
    return (d * g * (dtype(1) - g)).astype(dtype)


def gate_bwd_bound(gate, dgate, prev, bf16):
    """d = dgate * g * (1 - g): the subtraction (U relative to 1, i.e. U |dgate| g absolute), two products; one addition of the
    previous contents; one bf16 store"""
    g, d = np.asarray(gate, dtype=F64), np.asarray(dgate, dtype=F64)
    ref = d * g * (1 - g)
    b = np.abs(d) * g * U + 2 * U * np.abs(ref)
    if prev is not None:
        ref = ref + np.asarray(prev, dtype=F64)
        b = b + U * np.abs(ref)
    return b + (BF16 * np.abs(ref) if bf16 else 0.0) + 2.0 ** -140


def channel_dot_ref(a, b, dtype=F64):
    """(N, HW, C) x 2 -> (N, C)"""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    if dtype == F64:
        return (a * b).sum(1)
    return tree_sum(thread_partials((a * b).astype(F32)))        # 256 strided partial sums, then 8 halving levels (kernel: 6 + 3)


def channel_dot_bound(a, b):
    """one product, ceil(HW / 256) - 1 additions in a thread, 6 wave steps, 3 across the waves: times sum |a b|"""
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    HW = a.shape[1]
    depth = 1 + (math.ceil(HW / 256) - 1) + 6 + 3
    return depth * U * np.abs(a * b).sum(1)


def scale_channels_ref(x, gate, dtype=F64):
    """x (N, HW, C) * gate (N, C)"""
    return (np.asarray(x, dtype=dtype) * np.asarray(gate, dtype=dtype)[:, None, :]).astype(dtype)


def group_softmax_ref(x, G, P, dtype=F64):
    """x (npix, G * P): soft-max over the P points of each group"""
    x = np.asarray(x, dtype=dtype).reshape(-1, G, P)
    e = np.exp(x - x.max(2, keepdims=True))
    return (e / e.sum(2, keepdims=True)).astype(dtype).reshape(-1, G * P)


def group_softmax_bwd_ref(y, dy, G, P, prev=None, dtype=F64):
    y, dy = np.asarray(y, dtype=dtype).reshape(-1, G, P), np.asarray(dy, dtype=dtype).reshape(-1, G, P)
    dx = (y * (dy - (y * dy).sum(2, keepdims=True))).astype(dtype).reshape(-1, G * P)
    return dx if prev is None else (dx + np.asarray(prev, dtype=dtype)).astype(dtype)


def softmax_rel_bound(P, D):
    """relative error of one probability e_k / s over P points;  D = largest |v - max| of the data.  As softmax_rel_bound of
    tests/test_gpu_prediction_tail.py with C replaced by P.  EXPF: the kernel's __expf is v_exp_f32 of the argument times log2(e):
    the rounded product moves the exponent by |d| U (counted with D below, twice: the product and the rounded constant) and the
    instruction itself is 1 ulp (2 U); 4 U = 2 ulp is taken, the figure the prediction-tail module takes for expf"""
    num = 3 * D * U + EXPF
    den = num + (P - 1) * U
    return num + den + 2 * U


def group_softmax_bwd_bound(y, dy, G, P, prev, bf16):
    """like softmax_bwd_abs_bound: S = sum |y dy| of the group bounds the dot (P products and additions), g - dot, the product; the
    previous contents one addition; one bf16 store"""
    y64, d64 = np.asarray(y, dtype=F64).reshape(-1, G, P), np.asarray(dy, dtype=F64).reshape(-1, G, P)
    S = np.abs(y64 * d64).sum(2, keepdims=True)
    ref = y64 * (d64 - (y64 * d64).sum(2, keepdims=True))
    b = y64 * ((P + 1) * U * S) + 2 * U * y64 * (np.abs(d64) + S)
    b, ref = b.reshape(-1, G * P), ref.reshape(-1, G * P)
    if prev is not None:
        ref = ref + np.asarray(prev, dtype=F64)
        b = b + U * np.abs(ref)
    return b + (BF16 * np.abs(ref) if bf16 else 0.0)


def bn_eval_ref(gamma, beta, rm, rv, eps, dtype=F64):
    g, b, m, v = (np.asarray(t, dtype=dtype) for t in (gamma, beta, rm, rv))
    scale = (g / np.sqrt(v + dtype(eps))).astype(dtype)
    return scale, (b - m * scale).astype(dtype)


def bn_eval_bound(gamma, beta, rm, rv, eps):
    """scale: the addition (half of it survives the root), sqrtf and the division: 3 U relative.  shift: the product carries scale's
    error plus its own rounding, then the subtraction"""
    scale, shift = bn_eval_ref(gamma, beta, rm, rv, eps)
    bs = 3 * U * np.abs(scale)
    return bs, 4 * U * np.abs(np.asarray(rm, dtype=F64) * scale) + U * np.abs(shift)


def acc_sums_depth(N, Ho, Wo, Cp, V, replicas=8):
    """roundings on the path of one summand of ydl_resize_acc_sums' statistics: a thread owns one channel chunk and walks
    ceil(rows / CTAs) rows x ceil(Wo / R) pixels (R = 256 / chunks threads share a chunk), the R partials are added in LDS order, and
    the CTAs add theirs with atomics onto ``replicas`` rows (ceil(CTAs / replicas) each); the fused multiply-add of the squares counts
    one more.  The rows are summed in float64 by the caller."""
    cpb = min(Cp // V, 256)
    R = 256 // cpb
    ctas = min(N * Ho, 4096)
    return math.ceil(N * Ho / ctas) * math.ceil(Wo / R) + R + math.ceil(ctas / replicas) + 1


def acc_sums_ref(want, dtype=F64):
    """want (N, Ho, Wo, C): the unrounded results -> (2, C): sum and sum of squares per channel"""
    w = np.asarray(want, dtype=dtype)
    if dtype == F64:
        return np.stack([w.sum((0, 1, 2)), (w * w).sum((0, 1, 2))])
    w = w.reshape(1, -1, w.shape[-1])
    # float32 floor: 256 strided partial sums, then a halving tree (no deeper than the kernel's path for the shapes of the tests)
    return np.stack([tree_sum(thread_partials(w))[0], tree_sum(thread_partials((w * w).astype(F32)))[0]])


def acc_sums_bound(want, want_err, depth):
    """per (statistic, channel): depth U times sum |v| (sum v^2), plus the error of the summands themselves (want_err: the per-element
    bound of the values before they are rounded to the storage type; for the squares 2 |v| times it)"""
    w = np.abs(np.asarray(want, dtype=F64))
    e = np.broadcast_to(np.asarray(want_err, dtype=F64), w.shape)
    return np.stack([depth * U * w.sum((0, 1, 2)) + e.sum((0, 1, 2)), depth * U * (w * w).sum((0, 1, 2)) + (2 * w * e).sum((0, 1, 2))])


# ---------------------------------------------------------------------------------------------------------------------------
# the resize as two matrices (a second form of the same operator: y = Mh x Mw^T, dx = Mh^T dy Mw), for large shapes and as a cross-check
# ---------------------------------------------------------------------------------------------------------------------------
def axis_matrix(taps, n_in):
    i0, i1, w0, w1 = taps
    M = np.zeros((len(i0), n_in), dtype=F64)
    np.add.at(M, (np.arange(len(i0)), i0), np.asarray(w0, dtype=F64))
    np.add.at(M, (np.arange(len(i0)), i1), np.asarray(w1, dtype=F64))
    return M


def resize_fwd_matrix(x, th, tw):
    x = np.asarray(x, dtype=F64)
    return np.einsum("ah,nhwc,bw->nabc", axis_matrix(th, x.shape[1]), x, axis_matrix(tw, x.shape[2]), optimize=True)


def resize_bwd_matrix(dy, th, tw, Hi, Wi, prev=None):
    """-> (dx, sum |w dy|, contributing outputs) like resize_bwd_ref (weights wh * ww formed in float64 from the float32 axis
    weights: the float32 rounding of that product is one of the terms of resize_bwd_bound)"""
    dy = np.asarray(dy, dtype=F64)
    Mh, Mw = axis_matrix(th, Hi), axis_matrix(tw, Wi)
    dx = np.einsum("ah,nabc,bw->nhwc", Mh, dy, Mw, optimize=True)
    mag = np.einsum("ah,nabc,bw->nhwc", Mh, np.abs(dy), Mw, optimize=True)
    cnt = np.outer((Mh != 0).sum(0), (Mw != 0).sum(0))
    return (dx if prev is None else dx + np.asarray(prev, dtype=F64)), mag, cnt


# ---------------------------------------------------------------------------------------------------------------------------
# cases: inputs as the kernel reads them (already rounded to the storage type), float64 reference, bound, float32 floor, Layout
# ---------------------------------------------------------------------------------------------------------------------------
def vec(dtype):
    return 4 if dtype == "f32" else 8


def case_bilinear(x, mode, Ho, Wo, dtype, ld=None, gh=0.0, gw=0.0, lead=LEAD):
    x = store(x, dtype)
    N, Hi, Wi, C = x.shape
    Cp = rup(C, vec(dtype))
    th, tw = axis_taps(mode, Hi, Ho, gh), axis_taps(mode, Wi, Wo, gw)
    ref, mag = resize_fwd_ref(x.astype(F64), th, tw)
    f32, _ = resize_fwd_ref(x, th, tw, F32)
    return dict(layout=Layout(N * Ho * Wo, ld or Cp, C, Cp, "free", lead), x=x, th=th, tw=tw, ref=ref, mag=mag,
                bound=bilinear_fwd_bound(mag, ref, dtype == "bf16") if mode else 0.0, floor=store(f32, dtype))


RESIZE_BWD_CEILING = {"f32": 2e-6, "bf16": 1e-2}        # of the largest element: what tests/test_gpu_spatial.py asserts already


def case_resize_bwd(dy, mode, Hi, Wi, dtype, prev=None, ld=None, gh=0.0, gw=0.0, lead=LEAD, matrix=False):
    dy = store(dy, dtype)
    prev = None if prev is None else store(prev, dtype)
    N, Ho, Wo, C = dy.shape
    Cp = rup(C, vec(dtype))
    th, tw = axis_taps(mode, Hi, Ho, gh), axis_taps(mode, Wi, Wo, gw)
    if matrix:
        ref, mag, cnt = resize_bwd_matrix(dy, th, tw, Hi, Wi, prev)
        f32 = np.einsum("ah,nabc,bw->nhwc", axis_matrix(th, Hi).astype(F32), dy, axis_matrix(tw, Wi).astype(F32), optimize=True)
        f32 = f32 if prev is None else (prev + f32).astype(F32)
    else:
        ref, mag, cnt = resize_bwd_ref(dy.astype(F64), th, tw, Hi, Wi, None if prev is None else prev.astype(F64))
        f32 = resize_bwd_ref(dy, th, tw, Hi, Wi, prev, dtype=F32)[0]
    if mode == 0:
        bound = (U * np.abs(ref) * np.asarray(cnt)[None, :, :, None]) + (BF16 * np.abs(ref) if dtype == "bf16" else 0.0)
    else:
        bound = resize_bwd_bound(mag, cnt, ref, prev, dtype == "bf16")
    bound = np.minimum(bound, RESIZE_BWD_CEILING[dtype] * np.abs(ref).max())
    return dict(layout=Layout(N * Hi * Wi, ld or Cp, C, Cp, "free", lead), dy=dy, prev=prev, th=th, tw=tw, ref=ref, mag=mag, cnt=cnt,
                bound=bound, floor=store(f32, dtype))


def case_global_avg(x, dtype, ld=None, lead=LEAD):
    """x (N, HW, C)"""
    x = store(x, dtype)
    N, HW, C = x.shape
    Cp = rup(C, vec(dtype))
    avg = global_pool_ref(x.astype(F64))[0]
    return dict(layout=Layout(N, ld or Cp, C, Cp, "free", lead), x=x, ref=avg, bound=global_avg_bound(x, dtype == "bf16"),
                floor=store(global_avg_f32(x), dtype))


def case_channel_dot(a, b, dtype):
    a, b = store(a, dtype), store(b, dtype)
    N, HW, C = a.shape
    return dict(layout=Layout(N, C, C), a=a, b=b, ref=channel_dot_ref(a, b), bound=channel_dot_bound(a, b), floor=channel_dot_ref(a, b, F32))


def case_scale_channels(x, gate, dtype, ld=None, lead=LEAD):
    x, gate = store(x, dtype), np.asarray(gate, dtype=F32)
    N, HW, C = x.shape
    Cp = rup(C, vec(dtype))
    ref = scale_channels_ref(x, gate)
    return dict(layout=Layout(N * HW, ld or Cp, C, Cp, "zero", lead), x=x, gate=gate, ref=ref,
                bound=U * np.abs(ref) + (BF16 * np.abs(ref) if dtype == "bf16" else 0.0), floor=store(scale_channels_ref(x, gate, F32), dtype))


def case_gate_fwd(a, b, dtype):
    a, b = store(a, dtype), store(b, dtype)
    N, C = a.shape
    return dict(layout=Layout(N, C, C), a=a, b=b, ref=gate_fwd_ref(a, b), bound=gate_fwd_bound(a, b), floor=gate_fwd_ref(a, b, F32))


def case_gate_bwd(gate, dgate, dtype, prev=None, ld=None, lead=LEAD):
    gate, dgate = np.asarray(gate, dtype=F32), np.asarray(dgate, dtype=F32)
    prev = None if prev is None else store(prev, dtype)
    N, C = gate.shape
    ref = gate_bwd_ref(gate, dgate) + (0.0 if prev is None else prev.astype(F64))
    f32 = gate_bwd_ref(gate, dgate, F32)
    f32 = f32 if prev is None else (prev + f32).astype(F32)
    return dict(layout=Layout(N, ld or C, C, lead=lead), gate=gate, dgate=dgate, prev=prev, ref=ref,
                bound=gate_bwd_bound(gate, dgate, prev, dtype == "bf16"), floor=store(f32, dtype))


def case_group_softmax(x, G, P, dtype, ld=None, lead=LEAD):
    x = store(x, dtype)
    ref = group_softmax_ref(x, G, P)
    D = float((x.reshape(-1, G, P).max(2, keepdims=True) - x.reshape(-1, G, P)).astype(F64).max())
    rel = softmax_rel_bound(P, D)
    return dict(layout=Layout(x.shape[0], ld or G * P, G * P, lead=lead), x=x, ref=ref, rel=rel,
                bound=rel * ref + (BF16 * ref if dtype == "bf16" else 0.0), floor=store(group_softmax_ref(x, G, P, F32), dtype))


def case_group_softmax_bwd(y, dy, G, P, dtype, prev=None, ld=None, lead=LEAD):
    y, dy = store(y, dtype), store(dy, dtype)
    prev = None if prev is None else store(prev, dtype)
    ref = group_softmax_bwd_ref(y, dy, G, P, prev)
    return dict(layout=Layout(y.shape[0], ld or G * P, G * P, lead=lead), y=y, dy=dy, prev=prev, ref=ref,
                bound=group_softmax_bwd_bound(y, dy, G, P, prev, dtype == "bf16"),
                floor=store(group_softmax_bwd_ref(y, dy, G, P, prev, F32), dtype))


def case_bn_eval(gamma, beta, rm, rv, eps):
    g, b, m, v = (np.asarray(t, dtype=F32) for t in (gamma, beta, rm, rv))
    C = g.size
    scale, shift = bn_eval_ref(g, b, m, v, eps)
    bs, bh = bn_eval_bound(g, b, m, v, eps)
    fs, fh = bn_eval_ref(g, b, m, v, eps, F32)
    return dict(layout=Layout(2, C, C), gamma=g, beta=b, rm=m, rv=v, ref=np.stack([scale, shift]), bound=np.stack([bs, bh]),
                floor=np.stack([fs, fh]))


def case_global_pool_bwd(davg, dmx, amax, HW, dtype, prev=None, ld=None, lead=LEAD):
    """dx = prev + davg * (1 / HW) + [p == arg-max] dmx in that order: 1 / HW and the product (2 U |davg / HW|), two additions (U of
    each partial sum, bounded by the sum of the magnitudes), one bf16 store"""
    davg = None if davg is None else store(davg, dtype)
    dmx = None if dmx is None else store(dmx, dtype)
    prev = None if prev is None else store(prev, dtype)
    N, C = np.shape(amax)
    Cp = rup(C, vec(dtype))
    ref = global_pool_bwd_ref(davg, dmx, amax, HW, prev)
    a = np.zeros((N, 1, C)) if davg is None else np.abs(davg.astype(F64))[:, None, :] / HW
    hit = np.arange(HW)[None, :, None] == np.asarray(amax)[:, None, :]
    m = np.zeros((N, HW, C)) if dmx is None else np.where(hit, np.abs(dmx.astype(F64))[:, None, :], 0.0)
    pv = np.zeros((N, HW, C)) if prev is None else np.abs(prev.astype(F64))
    bound = 2 * U * a + 2 * U * (pv + a + m) + (BF16 * np.abs(ref) if dtype == "bf16" else 0.0)
    return dict(layout=Layout(N * HW, ld or Cp, C, Cp, "free", lead), davg=davg, dmx=dmx, prev=prev, ref=ref, bound=bound,
                floor=store(global_pool_bwd_ref(davg, dmx, amax, HW, prev, dtype=F32), dtype))


def case_acc_sums(dtype, mode, N, Hi, Wi, Ho, Wo, C, x, y0):
    """-> (values case, statistics case) of y0 + resize(x); the statistics are those of the float32 results before the store"""
    V = vec(dtype)
    Cp = rup(C, V)
    c = case_bilinear(x, mode, Ho, Wo, dtype)
    y0 = store(y0, dtype)
    want = y0.astype(F64) + c["ref"]
    err = (6 * U * c["mag"] if mode else 0.0) + U * np.abs(want)
    f32 = (y0 + resize_fwd_ref(c["x"], c["th"], c["tw"], F32)[0]).astype(F32)
    vals = dict(layout=Layout(N * Ho * Wo, Cp, C, Cp), x=c["x"], y0=y0, ref=want, bound=err + (BF16 * np.abs(want) if dtype == "bf16" else 0.0),
                floor=store(f32, dtype))
    ref = acc_sums_ref(want)
    bound = np.minimum(acc_sums_bound(want, err, acc_sums_depth(N, Ho, Wo, Cp, V)), 2e-5 * np.abs(ref).max())
    stats = dict(layout=Layout(2, C, C), ref=ref, bound=bound, floor=acc_sums_ref(f32, F32))
    return vals, stats
