"""The fused replicated tail (csrc/loss.hip: ydl_seg_tail_fwd / ydl_seg_tail_bwd) through the C ABI: against the float64 reference of
tests/loss_ref.py and against the unfused launches (ydl_softmax_fwd at the stored resolution, ydl_seg_loss_rep_fwd,
ydl_seg_loss_rep_bwd, ydl_softmax_bwd) on the same operands.

What is asserted per case
  losses        fused == unfused at rtol 2e-6 (tests/test_gpu_blocks.py::test_loss_replicated_matches_full uses it between paths: the
                per-CTA sums are associated differently, nothing else changes); T exact, I and P at the same rtol scaled to the
                largest entry
  label counts  exact, one byte per class, against a CPU count (rh * rw <= 255); the bytes around the buffer keep their canary
  dx            (a) max-norm error against float64 under dx_bound() below; (b) relative-L2 and max-abs error against float64 at most
                1.1 x those of the unfused pair; pad channels [C, Cp) exactly 0, channels [Cp, lddx) and the elements behind the last
                row keep the sentinel
dx_bound adds up what tests/test_gpu_prediction_tail.py asserts for the two unfused launches, plus the terms that only exist once
they are chained (there each launch is judged on exact inputs).  With g = dlow, S = the largest sum_c |g_c| of a pixel:
  2 b_g         dx = p (g - sum p g): an error of g enters once directly and once through the p-weighted mean; b_g = the bound
                loss_bounds() gives for dlow, capped at 1e-5 of its largest element as test_replicated_loss caps it
  2 b_in        the loss reads probabilities that are themselves rounded: relative error rel_p = softmax_rel_bound(), so (p <= 1) the
                inner soft-max of the loss moves by at most 2 rel_p where loss_bounds() allows e_p for its own arithmetic: the
                uncapped gradient bound scaled by 2 rel_p / e_p
  3 rel_p S     the error of p in p (g - sum p g): the factor, and every term of the mean
  softmax_bwd_abs_bound(C, 1, S, max |dx|, bf16)     the arithmetic and the store of the soft-max backward

Measured on one MI355X: in every case the fused pair's max-abs and relative-L2 errors against float64 equal the unfused pair's to the
printed digits (the per-pixel statements are the same; at these sizes the partial sums happen to associate alike too), f32 at most
0.0023 of dx_bound, bf16 at most 0.86 of it (the store rounding, as for the unfused soft-max backward).  34 tests, 4.1 s for the module."""
import math

import pytest
import torch

from tests import loss_ref as R
from tests import test_gpu_prediction_tail as PT

pytestmark = pytest.mark.gpu

U, SENT, SLACK = PT.U, PT.SENT, PT.SLACK
CANARY = 0xA5


def dx_bound(C, rep, kind, ls, cw, target, x64, p64, ref, dlow64, dx64, g0, bf16):
    N, _, h, w = p64.shape
    nrep = rep[0] * rep[1]
    wl = (cw if cw is not None else torch.ones(C))[target.clamp(0, C - 1)].double()
    wl = float(wl[(target >= 0) & (target < C)].sum())
    stats = PT._spread(p64)
    b = PT.loss_bounds(ref, C, stats, h * w, nrep, ls, cw, wl, N * h * w * nrep, kind, 1e-6, g0)
    b_g = min(b["grad"], 1e-5 * float(dlow64.abs().max()))
    rel_p = PT.softmax_rel_bound(C, PT._spread(x64)[0])
    e_p = (1 / math.e + stats[2]) * U + 2 * PT.EXPF + (C + 1) * U
    b_in = b["grad"] * 2 * rel_p / e_p
    S = float(dlow64.abs().sum(1).max())
    return 2 * (b_g + b_in) + 3 * rel_p * S + PT.softmax_bwd_abs_bound(C, 1, S, float(dx64.abs().max()), bf16)


def _rows(t, ld, tdt, pad):
    """(N, C, h, w) CPU tensor -> NHWC rows of stride ld on the GPU; the pad channels hold ``pad``"""
    N, C, h, w = t.shape
    rows = torch.full((N * h * w, ld), pad, dtype=tdt)
    rows[:, :C] = t.permute(0, 2, 3, 1).reshape(-1, C).to(tdt)
    return rows.cuda()


def _case(N, C, h, w, rep, dtype, ldx, kind, ls, weighted, bad, lddx=None, dloss=0.7, seed=0, floor=True):
    L, _p, _stream = PT._L()
    rh, rw = rep
    lddx = lddx or ldx
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    dt = L.YDL_F32 if dtype == "f32" else L.YDL_BF16
    x = PT._logits((N, C, h, w), seed + 41, tdt)                       # bf16 cases: the rounded values are the input
    target = PT._labels(N, C, h * rh, w * rw, seed + 41, None, bad)
    cw = PT._weights(C, seed) if weighted else None
    k = L.LOSS_DICE if kind == "dice" else L.LOSS_JACCARD
    tag = f"tail N={N} C={C} {h}x{w} rep={rep} {dtype} ldx={ldx} lddx={lddx} {kind} ls={ls} cw={weighted} bad={bad} dloss={dloss}"
    print(tag)
    npix = N * h * w
    xd = _rows(x, ldx, tdt, 99.0)                                      # a pad value that would win every max
    td = target.cuda()
    cwd = None if cw is None else cw.cuda()
    dl = None if dloss is None else torch.tensor([dloss], device="cuda")
    g0 = 1.0 if dloss is None else dloss
    nws = L.lib().ydl_seg_loss_ws_floats(N, C)
    st = _stream()

    def buffers():
        return (torch.full((nws + SLACK,), SENT, device="cuda"), torch.full((3 + SLACK,), SENT, device="cuda"),
                torch.full((npix * lddx + SLACK,), SENT, dtype=tdt, device="cuda"))

    # fused pair
    ws_f, loss_f, dx_f = buffers()
    nb = L.lib().ydl_seg_tail_count_bytes(N, C, h, w, rh, rw)
    assert nb == (npix * (16 if C <= 16 else 32) if rh * rw <= 255 else 0)
    cbuf = torch.full((16 + nb + SLACK,), CANARY, dtype=torch.uint8, device="cuda")
    counts = cbuf[16:16 + nb]
    L.call("ydl_seg_tail_fwd", dt, _p(xd), ldx, _p(td), _p(cwd), k, ls, 1e-6, N, C, h, w, rh, rw, _p(ws_f), _p(loss_f),
           _p(counts) if nb else None, st)
    L.call("ydl_seg_tail_bwd", dt, _p(xd), ldx, _p(counts) if nb else None, _p(td), _p(cwd), ls, N, C, h, w, rh, rw, _p(ws_f), _p(dl),
           _p(dx_f), lddx, st)
    # unfused launches on the same operands
    ws_u, loss_u, dx_u = buffers()
    plow = torch.empty((N, C, h, w), device="cuda")
    dlow = torch.empty_like(plow)
    ps = plow.stride()
    L.call("ydl_softmax_fwd", dt, _p(xd), ldx, _p(plow), *ps, N, h, w, C, 1, 1, st)
    L.call("ydl_seg_loss_rep_fwd", _p(plow), *ps, _p(td), _p(cwd), k, ls, 1e-6, N, C, h, w, rh, rw, _p(ws_u), _p(loss_u), st)
    L.call("ydl_seg_loss_rep_bwd", _p(plow), *ps, _p(td), _p(cwd), k, ls, 1e-6, N, C, h, w, rh, rw, _p(ws_u), _p(dl), _p(dlow), st)
    L.call("ydl_softmax_bwd", dt, _p(plow), _p(dlow), *ps, _p(dx_u), lddx, N, h, w, C, 1, 1, st)
    torch.cuda.synchronize()

    # ---- canaries
    assert bool((ws_f[nws:] == SENT).all()) and bool((loss_f[3:] == SENT).all()), tag
    assert bool((cbuf[:16] == CANARY).all()) and bool((cbuf[16 + nb:] == CANARY).all()), tag + ": bytes around the counts"
    Cp = PT.r8(C) if PT.r8(C) <= lddx else C
    got_f, got_u = dx_f.cpu(), dx_u.cpu()
    assert bool((got_f[npix * lddx:] == SENT).all()), tag
    got_f, got_u = got_f[:npix * lddx].view(npix, lddx), got_u[:npix * lddx].view(npix, lddx)
    assert bool((got_f[:, C:Cp] == 0).all()), tag + ": pad channels [C, Cp) must be exactly 0"
    assert bool((got_f[:, Cp:] == SENT).all()), tag + ": channels [Cp, lddx) must keep the sentinel"

    # ---- label counts: exact
    if nb:
        MC = 16 if C <= 16 else 32
        t6 = target.view(N, h, rh, w, rw).permute(0, 1, 3, 2, 4).reshape(npix, rh * rw)
        want = torch.stack([(t6 == c).sum(1) for c in range(MC)], 1).to(torch.uint8)
        assert torch.equal(counts.cpu().view(npix, MC), want), tag + ": label counts"

    # ---- losses and merged sums: fused against unfused
    lf, lu = loss_f[:3].cpu(), loss_u[:3].cpu()
    print(f"  losses fused {lf.tolist()} unfused {lu.tolist()}")
    assert torch.allclose(lf, lu, rtol=2e-6, atol=0), (tag, lf, lu)
    nc = N * C
    sf, su = ws_f[:3 * nc].cpu(), ws_u[:3 * nc].cpu()
    assert torch.equal(sf[2 * nc:], su[2 * nc:]), (tag, "T is a count: exact")
    for j, name in enumerate("IP"):
        a, b = sf[j * nc:(j + 1) * nc], su[j * nc:(j + 1) * nc]
        assert float((a - b).abs().max()) <= 2e-6 * float(b.abs().max()), (tag, name)

    # ---- float64 reference of the chain
    x64 = x.double()
    p64 = torch.softmax(x64, 1)
    ref = R.seg_loss_rep_ref(p64, target, rep, cw, kind, ls, 1e-6)
    for j, name in enumerate(("total", "ce", "overlap")):
        r = getattr(ref, name)
        assert abs(float(lf[j]) - r) <= 1e-4 * abs(r), (tag, name, float(lf[j]), r)       # the suite's ceiling on the loss items
    dlow64 = ref.dpred * g0
    dx64 = R.softmax_bwd_ref(p64, dlow64)
    to_rows = lambda t: t.permute(0, 2, 3, 1).reshape(npix, C).double()
    want = to_rows(dx64)
    ef, eu = got_f[:, :C].double() - want, got_u[:, :C].double() - want
    mf, mu = float(ef.abs().max()), float(eu.abs().max())
    l2f, l2u = float(ef.norm() / want.norm()), float(eu.norm() / want.norm())
    bound = dx_bound(C, rep, kind, ls, cw, target, x64, p64, ref, dlow64, dx64, g0, dtype == "bf16")
    print(f"  dx max-abs: fused {mf:.3e} unfused {mu:.3e} bound {bound:.3e}   rel-L2: fused {l2f:.3e} unfused {l2u:.3e}")
    if floor:           # the same reference expressions in float32 must pass the bound themselves
        p32 = torch.softmax(x.float(), 1)
        f32 = R.seg_loss_rep_ref(p32, target, rep, cw, kind, ls, 1e-6, dtype=torch.float32)
        fl = float((to_rows(R.softmax_bwd_ref(p32, f32.dpred * g0).to(tdt).float()) - want).abs().max())
        print(f"  dx float32 floor {fl:.3e}")
        assert fl <= bound, (tag, "the float32 evaluation of the reference misses its own bound", fl, bound)
    assert mf <= bound, (tag, mf, bound)
    assert mf <= 1.1 * mu, (tag, "max-abs error above 1.1 x the unfused pair's", mf, mu)
    assert l2f <= 1.1 * l2u, (tag, "relative-L2 error above 1.1 x the unfused pair's", l2f, l2u)


# (kind, ls, class weights, a block of labels = 255): rotated over the grid so that every C, rep and dtype meets both kinds, both
# smoothing values, weights present and absent; labels outside [0, C) only with ls = 0 (tests/test_gpu_prediction_tail.py: with
# smoothing the kernels keep such pixels in the smoothing sum and the float64 reference drops them)
_COMBOS = [("dice", 0.0, True, True), ("jaccard", 0.1, False, False), ("jaccard", 0.0, True, False), ("dice", 0.1, True, False),
           ("dice", 0.0, False, False), ("jaccard", 0.1, True, False), ("dice", 0.1, False, False), ("jaccard", 0.0, False, True)]
_REPS = [(4, 4), (2, 3), (4, 2), (1, 1)]
_LDS = {3: (8, 16), 12: (16, 24), 17: (24, 32)}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("C", [3, 12, 17])
@pytest.mark.parametrize("rep", _REPS)
def test_seg_tail(rep, C, dtype):
    i = _REPS.index(rep) + [3, 12, 17].index(C) * 3 + (1 if dtype == "bf16" else 0)
    for n, (h, w) in enumerate(((9, 14), (5, 7))):
        for j in (i + n, i + n + 5):
            kind, ls, weighted, bad = _COMBOS[j % 8]
            _case(3, C, h, w, rep, dtype, _LDS[C][(j + n) % 2], kind, ls, weighted, bad)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind,ls,weighted", [("dice", 0.0, True), ("jaccard", 0.0, False)])
def test_seg_tail_out_of_range_labels(kind, ls, weighted, dtype):
    """a block of labels set to 255 (and a row of -1): no class, in the counts and in every sum"""
    for C, rep in ((12, (4, 4)), (17, (2, 3)), (3, (4, 2)), (12, (1, 1))):
        _case(3, C, 9, 14, rep, dtype, PT.r8(C) + 8, kind, ls, weighted, True)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_seg_tail_unaligned_rows(dtype):
    """row strides that are no multiple of a 16-byte chunk, and a gradient without pad channels: the element-wise paths"""
    _case(3, 12, 9, 14, (4, 4), dtype, 15, "dice", 0.1, True, False)
    _case(3, 17, 5, 7, (2, 3), dtype, 19, "jaccard", 0.0, True, False, lddx=17)
    _case(3, 12, 5, 7, (4, 2), dtype, 16, "dice", 0.0, False, False, lddx=12)
    _case(3, 12, 9, 14, (4, 4), dtype, 16, "jaccard", 0.1, True, False, dloss=None)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_seg_tail_counts_beyond_a_byte(dtype):
    """rh * rw = 256 > 255: no counts buffer, the backward counts the labels itself"""
    _case(2, 12, 5, 7, (16, 16), dtype, 16, "dice", 0.1, True, False)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_seg_tail_more_pixels_than_threads(dtype):
    """600,000 stored pixels: 128 CTAs per image take several turns of the pixel loop, the last one partial"""
    _case(3, 12, 400, 500, (1, 1), dtype, 16, "dice", 0.1, True, False, floor=False)
