"""The prediction tail (csrc/loss.hip) through the C ABI against the float64 reference of tests/loss_ref.py: channel softmax forward
and backward (generic and rep4 kernels, <16> and <32> instantiations, padded rows, replication), the dense and the replicated
CE + Dice/Jaccard loss with their gradients and the merged I/P/T sums, and the argmax confusion matrix.  Every output lives in a
larger buffer pre-filled with a sentinel; everything outside the documented output must still hold it afterwards.

Bounds.  Each asserted quantity has a helper below that adds up named worst-case terms in units of U = 2^-24 (float32 unit roundoff):
EXPF / LOGF (device expf / logf, taken as 2 ulp = 4 U), the rounding of v - max scaled by the largest |v - max| of the case's own data,
C - 1 additions, one division and one product, the depth of each sum (terms per thread + 6 wave steps + 3 across waves + the float
store of the double merge), and for a bf16 store one rounding of the bf16 format, 2^-8 relative (the unit roundoff of 8 significant
bits, as tests/census.py has it; half of that, 2^-9, is not attainable by a correctly rounded store).  No bound is looser than what the
suite already asserts for the same quantity: 1e-4 relative on the loss items, 1e-4 / 1e-5 of the largest element on the dense /
replicated gradient.  Every test also evaluates the same reference expressions in float32 on the CPU and asserts that this floor
itself passes the bound.  Being sums of worst-case terms, the bounds come out at 3x to 50x the floor rather than at a fixed 4x (the
gradient bound, which takes the largest class weight for every pixel, at more; there the suite's 1e-4 / 1e-5 cap usually binds).  Every
test prints gpu error, floor and bound (pytest -s).

Measured on one MI355X, worst case per family: GPU error (float32 floor) / smallest asserted bound
  softmax forward, relative per element     f32 3.6e-7 (3.6e-7), bf16 input 3.0e-7 (3.1e-7) / 6.0e-7; at most 0.11 of the bound
  softmax backward, max-norm                f32 1.3e-6 (1.3e-6), at most 0.07 of the bound; bf16 7.5e-3 (7.5e-3), 0.87 of the bound,
                                            all of it the store rounding: with 2^-9 for it the float32 floor itself would not pass
  merged I / P, relative per (image, class) dense 3.2e-7 / 1.4e-7 (3.2e-7 / 1.8e-7), replicated 3.2e-7 / 1.5e-7 (2.8e-7 / 2.6e-7) / 1.3e-6
  T                                         exact
  CE / overlap / total, absolute            dense 7.3e-7 / 3.1e-8 / 9.2e-7 (2.0e-6 / 3.9e-8 / 2.1e-6) / 6.7e-6 / 1.2e-7 / 8.6e-6;
                                            replicated 6.2e-7 / 3.0e-8 / 6.9e-7 (1.6e-6 / 3.1e-8 / 1.6e-6)
  loss gradients, max-norm                  at most 0.05 of the bound, within 1.15x of the float32 floor in every case
  confusion matrix, sentinels, pad channels exact
154 tests, 4.1 s for the module on the GPU (the slowest test 0.5 s, which includes loading the library).

Labels outside [0, C) with label smoothing: the kernels keep such pixels in the smoothing sum, torch's ignore_index drops them, and the
reference project never feeds such labels; only ls = 0 is compared with float64 here (test_gpu_blocks keeps dense == replicated)."""
import functools
import math

import pytest
import torch

from tests import loss_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EXPF = 4 * U            # device expf: 2 ulp
LOGF = 4 * U            # device logf: 2 ulp of |log|
BF16 = 2.0 ** -8        # one round-to-nearest bf16 store
SENT = -24576.0         # -1.5 * 2^14: exact in f32 and bf16, far outside every output's range
LEAD = 16               # sentinel elements in front of every output view (a multiple of 4: 16-byte alignment is kept)
SLACK = 64
LOSS_THREADS = 128 * 256


def _L():
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.tape import _p, _stream
    return L, _p, _stream


def r8(c):
    return (c + 7) // 8 * 8


# ---------------------------------------------------------------------------------------------------------------------------
# bounds from named terms
# ---------------------------------------------------------------------------------------------------------------------------
def softmax_rel_bound(C, D):
    """relative error of one probability e_c / s;  D = largest |v - max| of the data"""
    num = D * U + EXPF                  # the rounded difference is exponentiated: its rounding counts |v - max| times; then expf
    den = num + (C - 1) * U             # s is a positive sum of such terms: the worst of them, plus C - 1 additions
    return num + den + 2 * U            # 1 / s and the product


def sum_depth(terms_per_thread):
    """roundings on the path of one summand through a per-thread sum, the 64-lane wave total, the 4 waves and the float store"""
    return (terms_per_thread - 1) + 6 + 3 + 1


def softmax_bwd_abs_bound(C, nrep, S, ref_max, bf16):
    """max-norm error of dx = p (g - sum p g);  S = largest sum of |dp| over one pixel's replicas, so |g| <= S, |dot| <= S"""
    g = (nrep - 1) * U * S              # nrep - 1 additions over the replicas
    dot = g + (C + 1) * U * S           # C products and additions of p g (p sums to 1)
    sub = 2 * S * U                     # g - dot
    mul = 2 * S * U                     # p * (...)
    return g + dot + sub + mul + (BF16 * ref_max if bf16 else 0.0)


def loss_bounds(ref, C, stats, npix_img, nrep, ls, cw, w_label_sum, n_pix_total, kind, eps, dloss):
    """-> dict of bounds for one loss case.  ref: float64 LossRef;  stats: _spread() of the predictions;  npix_img: stored pixels per
    image (they are spread over 128 x 256 threads);  nrep: replicas per stored pixel;  w_label_sum = sum_i w_t(i).
    A probability's error is p_c (|d_c| + sum_j p_j |d_j|) U + p_c (2 EXPF + (C + 1) U) with d = v - max: the numerator's argument
    rounding, the p-weighted one of the denominator, two expf, C - 1 additions, the division and the product.  p_c |d_c| <= 1 / e
    because p_c <= exp(d_c);  E1 = the largest sum_j p_j |d_j| of any pixel and E2 = the largest p-weighted mean of |d_c| within one
    (image, class) sum are taken from the case's own data."""
    D, M, E1, E2 = stats
    e_p = (1 / math.e + E1) * U + 2 * EXPF + (C + 1) * U                              # absolute error of one probability
    depth = sum_depth(math.ceil(npix_img / LOSS_THREADS)) + (2 if nrep > 1 else 0)      # count * term and rr * term products
    b_sum = (E2 + E1) * U + 2 * EXPF + (C + 1) * U + U + depth * U                    # I and P, per element, relative (w * p, depth)
    logc = math.log(C) if C > 1 else 0.0
    e_nlp = (D * U + EXPF + (C - 1) * U) + LOGF * logc + U * (M + logc) + U * (D + logc)   # |error| of one -log p_c
    wsum = float(cw.sum()) if cw is not None else float(C)
    ce = (1 - ls) * e_nlp + (ls / C) * e_nlp * n_pix_total * wsum / w_label_sum + (2 * depth + 3) * U * abs(ref.ce)
    I, P, T = ref.I, ref.P, ref.T
    if kind == "dice":
        den = P + T + eps
        aI, aP = 2.0 / den, (2.0 * I + eps) / den ** 2
    else:
        num, den = I + eps, P + T - I + eps
        aI, aP = 1.0 / den + num / den ** 2, num / den ** 2
    ov = float((aI * I + aP * P).mean()) * b_sum + U * abs(ref.overlap)               # first-order propagation of the I, P errors
    total = ce + 0.5 * ov + U * abs(ref.total)
    # gradient, max-norm: every term is (coefficient) x (a factor <= 1 made of probabilities); K_ce and K_ov are the largest coefficient
    # sums of any pixel.  aI reaches a pixel only through its own label, so classes without pixels do not count for it.
    wmax = float(cw.max()) if cw is not None else 1.0
    k_nll, k_sm = (1 - ls) / w_label_sum, ls / (C * w_label_sum)
    nc = I.numel()
    k_ce = nrep * abs(dloss) * (k_nll * wmax + k_sm * 2 * wsum)
    k_ov = nrep * abs(dloss) * 0.5 * 2 * wmax * float((torch.where(T > 0, aI, torch.zeros_like(aI)) + aP).max()) / nc
    grad = k_ce * (e_p + depth * U + 5 * U) + k_ov * (2 * e_p + 2 * b_sum + C * U + 6 * U)
    return dict(ce=ce, overlap=ov, total=total, sums=b_sum, grad=grad)


def _report(what, gpu, floor, bound):
    print(f"  {what}: gpu {gpu:.2e}  floor {floor:.2e}  bound {bound:.2e}")


def _check(what, gpu, floor, bound, ceiling=None):
    """the GPU error and the float32 floor of the same expression must both lie under the bound; the bound under the suite's ceiling"""
    if ceiling is not None:
        bound = min(bound, ceiling)
    _report(what, gpu, floor, bound)
    assert floor <= bound, (what, "the float32 evaluation of the reference misses its own bound", floor, bound)
    assert gpu <= bound, (what, gpu, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------------
def _strides(shape, layout):
    N, C, H, W = shape
    if layout == "nchw":
        return (C * H * W, H * W, W, 1)
    if layout == "cl":
        return (H * W * C, 1, W * C, C)
    if layout == "slice":                       # an NCHW window of a (N, C+3, H+2, W+5) tensor
        return ((C + 3) * (H + 2) * (W + 5), (H + 2) * (W + 5), W + 5, 1)
    raise ValueError(layout)


def _canvas(shape, strides, dtype=torch.float32, lead=LEAD, fill=SENT):
    need = lead + sum((s - 1) * st for s, st in zip(shape, strides)) + 1
    buf = torch.full((need + SLACK,), fill, dtype=dtype, device="cuda")
    return buf, buf.as_strided(shape, strides, lead)


def _outside_untouched(buf, shape, strides, lead=LEAD):
    mask = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    mask.as_strided(shape, strides, lead).fill_(True)
    return bool((buf[~mask] == SENT).all())


def _place(t, layout, lead=LEAD):
    """copy of the CPU tensor ``t`` (N, C, H, W) on the GPU with the strides of ``layout``, surrounded by sentinels"""
    st = _strides(t.shape, layout)
    buf, view = _canvas(tuple(t.shape), st, t.dtype, lead)
    view.copy_(t)
    return view


def _logits(shape, seed, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=gen) * 16 - 8).to(dtype)


def _spread(x64):
    """(D, M, E1, E2): largest |v - max| over the channel axis, largest |v|, largest sum_j p_j |d_j| of a pixel, largest p-weighted mean of
    |d_c| over one image and class (d = v - max)"""
    d = (x64.max(1, keepdim=True).values - x64)
    p = torch.softmax(x64, 1)
    e2 = (p * d).sum((2, 3)) / p.sum((2, 3))
    return float(d.max()), float(x64.abs().max()), float((p * d).sum(1).max()), float(e2.max())


# ---------------------------------------------------------------------------------------------------------------------------
# softmax forward
# ---------------------------------------------------------------------------------------------------------------------------
def _softmax_fwd_case(C, rep, dtype, ldx, layout, lead=LEAD, N=2, H=5, W=7, seed=1):
    L, _p, _stream = _L()
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    x = _logits((N, C, H, W), seed + C, tdt)                               # bf16 cases: the rounded values are the input
    rows = torch.full((N * H * W + 3, ldx), 99.0, dtype=tdt)               # pad channels hold a value that would win every max
    rows[:N * H * W, :C] = x.permute(0, 2, 3, 1).reshape(-1, C)
    xd = rows.cuda()
    shape = (N, C, H * rep[0], W * rep[1])
    st = _strides(shape, layout)
    buf, out = _canvas(shape, st, torch.float32, lead)
    L.call("ydl_softmax_fwd", L.YDL_F32 if dtype == "f32" else L.YDL_BF16, _p(xd), ldx, _p(out), *st, N, H, W, C, rep[0], rep[1],
           _stream())
    torch.cuda.synchronize()
    x64 = x.double()
    ref = R.softmax_ref(x64, rep)
    floor = float(((R.softmax_ref(x.float(), rep).double() - ref).abs() / ref).max())
    gpu = float(((out.cpu().double() - ref).abs() / ref).max())
    tag = f"softmax_fwd C={C} rep={rep} {dtype} ldx={ldx} {layout} lead={lead}"
    _check(tag, gpu, floor, softmax_rel_bound(C, _spread(x64)[0]))
    assert _outside_untouched(buf, shape, st, lead), tag
    return gpu, floor


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 2, 12, 16, 17, 24, 32])
def test_softmax_forward(C, dtype):
    for ldx in (r8(C), C + 3):
        for layout in ("nchw", "cl"):
            _softmax_fwd_case(C, (1, 1), dtype, ldx, layout)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("C,rep,layout,lead", [
    (12, (2, 3), "nchw", LEAD), (17, (2, 3), "cl", LEAD), (12, (3, 4), "cl", LEAD), (17, (3, 4), "nchw", LEAD),
    (12, (4, 4), "nchw", LEAD), (16, (4, 4), "nchw", LEAD), (12, (1, 4), "nchw", LEAD), (16, (1, 4), "nchw", LEAD),   # rep4 kernel
    (17, (4, 4), "nchw", LEAD),             # C > 16: generic kernel
    (12, (4, 4), "cl", LEAD),               # W stride != 1: generic kernel
    (12, (1, 4), "nchw", LEAD + 1),         # the view starts one float past a 16-byte boundary: generic kernel
    (12, (4, 4), "slice", LEAD),            # row stride W*4 + 5 is no multiple of 4 floats: generic kernel
    (16, (4, 4), "slice", LEAD + 3)])
def test_softmax_forward_replicated(C, rep, layout, lead, dtype):
    # ydl_debug_last_kernel does not report this family, so the kernel choice is not asserted; each path is judged by its output
    _softmax_fwd_case(C, rep, dtype, r8(C), layout, lead)


@pytest.mark.parametrize("C,rep", [(2, (1, 1)), (1, (1, 4))], ids=["generic", "rep4"])
def test_softmax_forward_grid_stride_tail(C, rep):
    """1032 x 1032 stored pixels: more than the 4096 x 256 threads of the capped grid"""
    _softmax_fwd_case(C, rep, "f32", r8(C), "nchw", N=1, H=1032, W=1032)


# ---------------------------------------------------------------------------------------------------------------------------
# softmax backward
# ---------------------------------------------------------------------------------------------------------------------------
def _softmax_bwd_case(C, rep, dtype, lddx, layout, N=2, H=5, W=7, seed=2):
    L, _p, _stream = _L()
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    gen = torch.Generator().manual_seed(seed + C)
    p_low = R.softmax_ref(_logits((N, C, H, W), seed + 7 * C).double()).float()        # the stored probabilities, float32
    p_full = R.replicate(p_low, rep)
    dp = torch.randn(p_full.shape, generator=gen)
    pd, dpd = _place(p_full, layout), _place(dp, layout)
    st = pd.stride()
    assert dpd.stride() == st
    npix = N * H * W
    dx = torch.full((npix * lddx + SLACK,), SENT, dtype=tdt, device="cuda")
    L.call("ydl_softmax_bwd", L.YDL_F32 if dtype == "f32" else L.YDL_BF16, _p(pd), _p(dpd), *st, _p(dx), lddx, N, H, W, C,
           rep[0], rep[1], _stream())
    torch.cuda.synchronize()
    got = dx.cpu()
    assert bool((got[npix * lddx:] == SENT).all())
    got = got[:npix * lddx].view(npix, lddx)
    Cp = r8(C) if r8(C) <= lddx else C
    tag = f"softmax_bwd C={C} rep={rep} {dtype} lddx={lddx} {layout}"
    assert bool((got[:, C:Cp] == 0).all()), tag + ": pad channels [C, Cp) must be exactly 0"
    assert bool((got[:, Cp:] == SENT).all()), tag + ": channels [Cp, lddx) must keep the sentinel"
    ref = R.softmax_bwd_ref(p_low.double(), dp.double(), rep)
    f32 = R.softmax_bwd_ref(p_low, dp, rep)
    to_rows = lambda t: t.permute(0, 2, 3, 1).reshape(npix, C).double()
    S = float(R.replica_sum(dp.abs().double(), rep).max())
    bound = softmax_bwd_abs_bound(C, rep[0] * rep[1], S, float(ref.abs().max()), dtype == "bf16")
    floor = float((to_rows(f32.to(tdt).float()) - to_rows(ref)).abs().max())
    gpu = float((got[:, :C].double() - to_rows(ref)).abs().max())
    _check(tag, gpu, floor, bound)


REPS = [(12, (1, 1)), (12, (2, 3)), (17, (2, 3)), (12, (3, 4)), (17, (3, 4)), (12, (4, 4)), (16, (4, 4)), (17, (4, 4)), (12, (1, 4)),
        (16, (1, 4))]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 2, 12, 16, 17, 24, 32])
def test_softmax_backward(C, dtype):
    for lddx in sorted({C, r8(C), r8(C) + 8}):
        _softmax_bwd_case(C, (1, 1), dtype, lddx, "nchw")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("C,rep", REPS[1:])
def test_softmax_backward_replicated(C, rep, dtype):
    for lddx in sorted({C, r8(C), r8(C) + 8}):
        _softmax_bwd_case(C, rep, dtype, lddx, "nchw")


@pytest.mark.parametrize("layout", ["cl", "slice"])
def test_softmax_backward_strided_gradient(layout):
    _softmax_bwd_case(12, (2, 3), "f32", 16, layout)
    _softmax_bwd_case(17, (1, 1), "bf16", 32, layout)


def test_softmax_backward_grid_stride_tail():
    _softmax_bwd_case(2, (1, 1), "f32", 8, "nchw", N=1, H=1032, W=1032)


# ---------------------------------------------------------------------------------------------------------------------------
# segmentation loss
# ---------------------------------------------------------------------------------------------------------------------------
def _weights(C, seed):
    gen = torch.Generator().manual_seed(100 + seed)
    return torch.rand(C, generator=gen) * 24.5 + 0.5


def _labels(N, C, Ht, Wt, seed, special=None, bad=False):
    gen = torch.Generator().manual_seed(200 + seed)
    t = torch.randint(0, C, (N, Ht, Wt), generator=gen)
    if special == "half":                       # image 0 never shows the upper half of the classes
        t[0] = torch.randint(0, max(C // 2, 1), (Ht, Wt), generator=gen)
    if special == "one":                        # image 1 is one class throughout
        t[min(1, N - 1)] = C - 1
    if bad:                                     # labels outside [0, C): no class
        t[0, :max(Ht // 3, 1), :max(Wt // 2, 1)] = 255
        t[N - 1, Ht - 1, ::2] = -1
    return t


@functools.lru_cache(maxsize=4)
def _dense_reference(N, C, H, W, Ht, Wt, kind, ls, weighted, special, bad, seed):
    pred = _logits((N, C, H, W), seed)
    target = _labels(N, C, Ht, Wt, seed, special, bad)
    cw = _weights(C, seed) if weighted else None
    ref = R.seg_loss_ref(pred, target, cw, kind, ls, 1e-6, (H, W))
    f32 = R.seg_loss_ref(pred, target, cw, kind, ls, 1e-6, (H, W), dtype=torch.float32)
    return pred, target, cw, ref, f32


def _compare_loss(tag, ref, f32, bounds, losses, ws, N, C, grad, dloss, grad_ceiling):
    nc = N * C
    for k, name in enumerate(("total", "ce", "overlap")):
        r = getattr(ref, name)
        _check(f"{tag} {name}", abs(float(losses[k]) - r), abs(getattr(f32, name) - r), bounds[name], 1e-4 * abs(r))
    for k, name in enumerate("IP"):
        r = getattr(ref, name).flatten()
        got, fl = ws[k * nc:(k + 1) * nc].double(), getattr(f32, name).flatten().double()
        scale = r.clamp_min(1e-300)
        assert bool((got[r == 0] == 0).all()), (tag, name, "a class without pixels must sum to exactly 0")
        _check(f"{tag} {name}", float(((got - r).abs() / scale).max()), float(((fl - r).abs() / scale).max()), bounds["sums"])
    assert torch.equal(ws[2 * nc:3 * nc].double(), ref.T.flatten()), (tag, "T is a count: exact")
    g = ref.dpred * dloss
    gmax = float(g.abs().max())
    _check(f"{tag} grad", float((grad.double() - g).abs().max()), float((f32.dpred.double() * dloss - g).abs().max()),
           bounds["grad"], grad_ceiling * gmax)


def _dense_case(N, C, H, W, kind, ls, weighted, layout="nchw", special=None, bad=False, dloss=0.7, Ht=None, Wt=None, seed=0):
    L, _p, _stream = _L()
    Ht, Wt = Ht or H, Wt or W
    pred, target, cw, ref, f32 = _dense_reference(N, C, H, W, Ht, Wt, kind, ls, weighted, special, bad, seed)
    pd = _place(pred, layout)
    st = pd.stride()
    td = target.cuda()
    cwd = None if cw is None else cw.cuda()
    nws = L.lib().ydl_seg_loss_ws_floats(N, C)
    ws = torch.full((nws + SLACK,), SENT, device="cuda")
    losses = torch.full((3 + SLACK,), SENT, device="cuda")
    gbuf, gd = _canvas(tuple(pred.shape), st)
    k = L.LOSS_DICE if kind == "dice" else L.LOSS_JACCARD
    dl = None if dloss is None else torch.tensor([dloss], device="cuda")
    L.call("ydl_seg_loss_fwd", _p(pd), *st, _p(td), Ht, Wt, _p(cwd), k, ls, 1e-6, N, C, H, W, _p(ws), _p(losses), _stream())
    L.call("ydl_seg_loss_bwd", _p(pd), *st, _p(td), Ht, Wt, _p(cwd), k, ls, 1e-6, N, C, H, W, _p(ws), _p(dl), _p(gd), _stream())
    torch.cuda.synchronize()
    tag = f"dense N={N} C={C} {H}x{W} labels {Ht}x{Wt} {kind} ls={ls} cw={weighted} {layout} {special} bad={bad} dloss={dloss}"
    print(tag)
    assert bool((ws[nws:] == SENT).all()) and bool((losses[3:] == SENT).all()), tag
    assert _outside_untouched(gbuf, tuple(pred.shape), st), tag
    t_at = R.resize_labels(target, (H, W))
    wl = (cw if cw is not None else torch.ones(C))[t_at.clamp(0, C - 1)].double()
    wl = float(wl[(t_at >= 0) & (t_at < C)].sum())
    stats = _spread(pred.double())
    g0 = 1.0 if dloss is None else dloss
    b = loss_bounds(ref, C, stats, H * W, 1, ls, cw, wl, N * H * W, kind, 1e-6, g0)
    _compare_loss(tag, ref, f32, b, losses[:3].cpu(), ws[:3 * N * C].cpu(), N, C, gd.cpu(), g0, 1e-4)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["dice", "jaccard"])
def test_dense_loss(kind, ls, weighted):
    _dense_case(3, 12, 9, 14, kind, ls, weighted)


@pytest.mark.parametrize("C,kind,ls,weighted", [(2, "jaccard", 0.1, True), (16, "dice", 0.1, False), (17, "jaccard", 0.0, True),
                                                (17, "dice", 0.1, True), (32, "dice", 0.0, True), (32, "jaccard", 0.1, False)])
def test_dense_loss_channel_counts(C, kind, ls, weighted):
    _dense_case(3, C, 9, 14, kind, ls, weighted)


@pytest.mark.parametrize("H,W,C,kind", [(1, 1, 12, "dice"), (1, 300, 17, "jaccard"), (200, 200, 12, "jaccard"), (200, 200, 32, "dice")])
def test_dense_loss_sizes(H, W, C, kind):
    """200 x 200 is more than the 128 x 256 threads of one image: the grid-stride loops take a second turn"""
    _dense_case(3, C, H, W, kind, 0.1, True)


@pytest.mark.parametrize("layout", ["cl", "slice"])
@pytest.mark.parametrize("C", [12, 17])
def test_dense_loss_strided_predictions(C, layout):
    _dense_case(3, C, 9, 14, "dice" if C == 12 else "jaccard", 0.1, True, layout)


@pytest.mark.parametrize("special", ["half", "one"])
@pytest.mark.parametrize("C,kind", [(12, "dice"), (12, "jaccard"), (32, "jaccard")])
def test_dense_loss_absent_classes(C, kind, special):
    """T = 0 for the absent classes: only eps keeps R finite"""
    _dense_case(3, C, 9, 14, kind, 0.0, True, special=special)


@pytest.mark.parametrize("dloss", [None, 0.7, 1.0])
def test_dense_loss_upstream_gradient(dloss):
    _dense_case(3, 12, 9, 14, "jaccard", 0.1, True, dloss=dloss)


@pytest.mark.parametrize("Ht,Wt,H,W,N", [(13, 11, 9, 14, 3), (18, 28, 9, 14, 3), (5, 5, 9, 14, 3), (640, 640, 48, 40, 2)])
def test_dense_loss_label_resize(Ht, Wt, H, W, N):
    _dense_case(N, 12, H, W, "dice", 0.1, True, Ht=Ht, Wt=Wt)
    _dense_case(N, 17, H, W, "jaccard", 0.0, False, Ht=Ht, Wt=Wt)


@pytest.mark.parametrize("C,kind", [(12, "dice"), (17, "jaccard")])
def test_dense_loss_out_of_range_labels(C, kind):
    """ls = 0: a label outside [0, C) has no CE term (ignore_index) and an all-zero one-hot row"""
    _dense_case(3, C, 9, 14, kind, 0.0, True, bad=True)


# ---------------------------------------------------------------------------------------------------------------------------
# replicated loss
# ---------------------------------------------------------------------------------------------------------------------------
def _rep_case(N, C, h, w, rep, kind, ls, weighted, layout="nchw", bad=False, dloss=0.7, seed=0):
    L, _p, _stream = _L()
    rh, rw = rep
    low = _logits((N, C, h, w), seed + 31)
    target = _labels(N, C, h * rh, w * rw, seed + 31, None, bad)
    cw = _weights(C, seed) if weighted else None
    ref = R.seg_loss_rep_ref(low, target, rep, cw, kind, ls, 1e-6)
    f32 = R.seg_loss_rep_ref(low, target, rep, cw, kind, ls, 1e-6, dtype=torch.float32)
    ld = _place(low, layout)
    st = ld.stride()
    td = target.cuda()
    cwd = None if cw is None else cw.cuda()
    nws = L.lib().ydl_seg_loss_ws_floats(N, C)
    ws = torch.full((nws + SLACK,), SENT, device="cuda")
    losses = torch.full((3 + SLACK,), SENT, device="cuda")
    gbuf, gd = _canvas(tuple(low.shape), st)
    k = L.LOSS_DICE if kind == "dice" else L.LOSS_JACCARD
    dl = None if dloss is None else torch.tensor([dloss], device="cuda")
    L.call("ydl_seg_loss_rep_fwd", _p(ld), *st, _p(td), _p(cwd), k, ls, 1e-6, N, C, h, w, rh, rw, _p(ws), _p(losses), _stream())
    L.call("ydl_seg_loss_rep_bwd", _p(ld), *st, _p(td), _p(cwd), k, ls, 1e-6, N, C, h, w, rh, rw, _p(ws), _p(dl), _p(gd), _stream())
    torch.cuda.synchronize()
    tag = f"replicated N={N} C={C} {h}x{w} rep={rep} {kind} ls={ls} cw={weighted} {layout} bad={bad} dloss={dloss}"
    print(tag)
    assert bool((ws[nws:] == SENT).all()) and bool((losses[3:] == SENT).all()), tag
    assert _outside_untouched(gbuf, tuple(low.shape), st), tag
    wl = (cw if cw is not None else torch.ones(C))[target.clamp(0, C - 1)].double()
    wl = float(wl[(target >= 0) & (target < C)].sum())
    stats = _spread(low.double())
    g0 = 1.0 if dloss is None else dloss
    b = loss_bounds(ref, C, stats, h * w, rh * rw, ls, cw, wl, N * h * w * rh * rw, kind, 1e-6, g0)
    _compare_loss(tag, ref, f32, b, losses[:3].cpu(), ws[:3 * N * C].cpu(), N, C, gd.cpu(), g0, 1e-5)


_COMBOS = [("dice", 0.0, True), ("jaccard", 0.05, False), ("jaccard", 0.0, True), ("dice", 0.05, True), ("dice", 0.0, False),
           ("jaccard", 0.05, True), ("dice", 0.05, False), ("jaccard", 0.0, False)]


@pytest.mark.parametrize("C", [12, 17, 32])
@pytest.mark.parametrize("rep", [(1, 1), (2, 3), (4, 2), (4, 4), (3, 4), (1, 4)])
def test_replicated_loss(rep, C):
    """against the float64 loss of the materialised replication; the (kind, ls, weights) combinations rotate over the grid so that
    every rep and every C meets both kinds, both ls and both weightings"""
    i = [(1, 1), (2, 3), (4, 2), (4, 4), (3, 4), (1, 4)].index(rep) + [12, 17, 32].index(C) * 3
    for j in (i, i + 5):
        kind, ls, weighted = _COMBOS[j % 8]
        _rep_case(3, C, 9, 14, rep, kind, ls, weighted)


@pytest.mark.parametrize("C,rep,kind,ls,weighted", [(12, (4, 4), "dice", 0.0, True), (17, (2, 3), "jaccard", 0.05, False),
                                                    (32, (1, 4), "jaccard", 0.05, True), (12, (4, 2), "dice", 0.05, False)])
def test_replicated_loss_large(C, rep, kind, ls, weighted):
    """190 x 180 stored pixels: more than the 128 x 256 threads of one image"""
    _rep_case(1, C, 190, 180, rep, kind, ls, weighted)


@pytest.mark.parametrize("layout,dloss", [("cl", None), ("slice", 0.7)])
def test_replicated_loss_strides_and_upstream_gradient(layout, dloss):
    _rep_case(3, 12, 9, 14, (4, 4), "jaccard", 0.05, True, layout, dloss=dloss)
    _rep_case(3, 17, 9, 14, (2, 3), "dice", 0.0, True, layout, dloss=dloss)


@pytest.mark.parametrize("C,rep,kind", [(12, (4, 4), "dice"), (17, (2, 3), "jaccard"), (32, (1, 4), "dice")])
def test_replicated_loss_out_of_range_labels(C, rep, kind):
    _rep_case(3, C, 9, 14, rep, kind, 0.0, True, bad=True)


# ---------------------------------------------------------------------------------------------------------------------------
# confusion matrix: exact
# ---------------------------------------------------------------------------------------------------------------------------
ISENT = -77777


def _confusion_inputs(N, C, H, W, seed):
    gen = torch.Generator().manual_seed(300 + seed)
    pred = torch.rand(N, C, H, W, generator=gen) * 16 - 8
    if C > 1:                                            # exact ties: one channel's float32 value copied into another
        n = N * H * W
        pix = pred.permute(0, 2, 3, 1).reshape(n, C)
        a = torch.randint(0, C, (n,), generator=gen)
        b = torch.randint(0, C, (n,), generator=gen)
        top = pix.max(1).values
        tie = torch.rand(n, generator=gen) < 0.5
        rows = torch.arange(n)[tie]
        pix[rows, a[tie]] = top[tie]                     # the maximum now sits at two places for about half of the pixels
        pix[rows, b[tie]] = top[tie]
        pred = pix.view(N, H, W, C).permute(0, 3, 1, 2).contiguous()
    target = torch.randint(-2, C + 3, (N, H, W), generator=gen)
    target[0, 0, : min(W, 4)] = 255
    return pred, target


def _confusion_case(C, ignore, layout="nchw", N=2, H=9, W=14, calls=1, seed=0):
    L, _p, _stream = _L()
    mat = torch.full((C * C + 16,), ISENT, dtype=torch.int64, device="cuda")
    mat[:C * C] = 0
    want = torch.zeros(C, C, dtype=torch.int64)
    kept = 0
    for i in range(calls):
        pred, target = _confusion_inputs(N, C, H, W, seed + i)
        pd, td = _place(pred, layout), target.cuda()
        L.call("ydl_confusion_matrix", _p(pd), *pd.stride(), _p(td), N, C, H, W, ignore, _p(mat), _stream())
        want += R.confusion_ref(pred, target, C, ignore)
        kept += int(((target >= 0) & (target < C) & (target != ignore)).sum())
    torch.cuda.synchronize()
    got = mat.cpu()
    tag = (C, ignore, layout, N, H, W, calls)
    assert bool((got[C * C:] == ISENT).all()), tag
    assert torch.equal(got[:C * C].view(C, C), want), tag
    assert int(got[:C * C].sum()) == kept, tag
    return want


@pytest.mark.parametrize("C", [1, 2, 12, 32])
def test_confusion_matrix(C):
    for ignore in (-1, 0, C - 1, 255):
        _confusion_case(C, ignore)
    want = _confusion_case(C, -1, seed=5)
    if C > 1:
        assert int(want.sum() - want.diag().sum()) > 0


@pytest.mark.parametrize("C", [2, 12, 32])
def test_confusion_matrix_first_maximum_wins(C):
    """every channel holds the same value: each kept pixel must land in column 0"""
    L, _p, _stream = _L()
    N, H, W = 1, 5, 7
    pred = torch.full((N, C, H, W), 0.25, device="cuda")
    target = (torch.arange(N * H * W) % C).view(N, H, W).cuda()
    mat = torch.zeros(C * C, dtype=torch.int64, device="cuda")
    L.call("ydl_confusion_matrix", _p(pred), *pred.stride(), _p(target), N, C, H, W, -1, _p(mat), _stream())
    torch.cuda.synchronize()
    assert torch.equal(mat.cpu().view(C, C), R.confusion_ref(pred.cpu(), target.cpu(), C, -1))
    assert int(mat.view(C, C)[:, 0].sum()) == N * H * W


@pytest.mark.parametrize("layout", ["cl", "slice"])
def test_confusion_matrix_strided_predictions(layout):
    _confusion_case(12, 11, layout)
    _confusion_case(32, 0, layout)


def test_confusion_matrix_accumulates_over_calls():
    _confusion_case(12, 11, calls=2)


def test_confusion_matrix_grid_stride_tail():
    """2 x 400 x 400 pixels: more than the 1024 x 256 threads of the capped grid"""
    _confusion_case(12, 11, N=2, H=400, W=400)


# ---------------------------------------------------------------------------------------------------------------------------
# python layer
# ---------------------------------------------------------------------------------------------------------------------------
def test_segmentation_loss_module_input_types():
    """a bf16 prediction, an int32 target and a non-contiguous target view give the bits of their float32 / int64 / contiguous
    equivalents"""
    import yolo_dual_amd as ydl
    N, C, H, W = 2, 12, 9, 14
    pred16 = _logits((N, C, H, W), 41, torch.bfloat16).cuda()
    wide = _labels(N, C, H, 2 * W, 41).cuda()
    cw = _weights(C, 41)
    strided = wide.int()[:, :, ::2]
    assert not strided.is_contiguous() and strided.dtype == torch.int32
    res = []
    for pred, target in ((pred16, strided), (pred16.float(), wide[:, :, ::2].contiguous())):
        assert target.shape == (N, H, W)
        x = pred.clone().requires_grad_(True)
        crit = ydl.SegmentationLoss(C, 0.1, cw, "jaccard")
        total, items = crit(x, target)
        total.backward()
        res.append((total.detach().cpu(), torch.tensor(items), x.grad.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][2].dtype == torch.bfloat16                 # autograd hands a bf16 leaf the float32 gradient rounded once
    assert torch.equal(res[0][2], res[1][2].to(torch.bfloat16))
    ref = R.seg_loss_ref(pred16.cpu(), wide[:, :, ::2].cpu(), cw, "jaccard", 0.1, 1e-6)
    assert abs(float(res[0][0]) - ref.total) <= 1e-4 * abs(ref.total)


def test_confusion_matrix_class_input_types():
    import yolo_dual_amd as ydl
    N, C, H, W = 2, 12, 9, 14
    pred, target = _confusion_inputs(N, C, H, 2 * W, 43)
    pred16 = pred[:, :, :, :W].to(torch.bfloat16).cuda()
    wide = target.cuda()
    a, b = ydl.ConfusionMatrix(C, ignore_index=11), ydl.ConfusionMatrix(C, ignore_index=11)
    strided = wide.int()[:, :, ::2]
    assert not strided.is_contiguous() and strided.dtype == torch.int32
    a.process_batch(pred16, strided)
    b.process_batch(pred16.float().contiguous(), wide[:, :, ::2].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(a.matrix, b.matrix)
    assert torch.equal(a.matrix.cpu(), R.confusion_ref(pred16.float().cpu(), wide[:, :, ::2].cpu(), C, 11))
