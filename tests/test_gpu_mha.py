"""GPU: dense multi-head self-attention through the C ABI (ydl_mha_fwd / ydl_mha_bwd) against the float64 closed form of
tests/mha_ref.py: out, lse, dQ, dK and dV.  Errors are relative to the reference tensor's max.

* f32: out <= 1e-5, dQ / dK / dV <= 1e-4 (the bounds of the sibling op, tests/test_gpu_local_attn.py; the f32 MFMA chains are exact fmaf).
* bf16: no number fixed in advance.  The same test runs a torch bf16 composition on the GPU (inputs rounded to bf16, matmul in bf16,
  softmax in f32, P rounded to bf16 before P.V, autograd backward) and measures it against the same float64 reference, which is fed
  the bf16-rounded inputs; per tensor, ours <= 2 x torch's.  The 2 covers the differing rounding points of two otherwise equivalent
  bf16 pipelines (where P and dS are rounded, accumulation order, delta taken from the rounded output).  Both errors are printed.
  Where the reference tensor is identically zero (one token: dS = P (dP - delta) cancels exactly, so dQ = dK = 0) there is no max to
  divide by, and torch's autograd cancels symbolically (error exactly 0).  There the error is taken relative to
  scale * max|dout| * max|v| * max|k or q|, the size of the terms that cancel, and must stay under the f32 gradient bound 1e-4: the
  cancelling terms are two f32 sums of the same exact bf16 products.
* shapes: the smallest at which the kernel can go wrong (one token; a tail tile with several heads in a row; d that is no multiple of
  the MFMA step; one row past a 64-row tile; several query and key tiles; the largest d; large scores across tiles).
* every operand row carries NaN outside its channels where the case has a wider leading dimension: a read of one poisons the result,
  a write to one is caught afterwards; lse and the workspace are guarded by NaN beyond their size.
* two backward runs are bitwise equal."""
import ctypes
import functools

import pytest
import torch

from tests import mha_ref as R

pytestmark = pytest.mark.gpu

# (id, N, S, heads, d, largest |score| wanted (0: as drawn), layout, accumulate)
#   layout "sep": q, k, v, out, dout, dq, dk, dv each in rows of their own; "pad": the same with 2 NaN elements after every row (rows that are not
#   16-byte aligned: the element-wise path);
#   "pad8": 8 NaN elements after every row (rows stay 16-byte aligned: the 8- and 16-byte vector loads and stores);
#   "qkv": q | k | v channel blocks of ONE buffer with ld = 3*C, and dq | dk | dv of another
CASES = [("one_token", 1, 1, 1, 8, 0, "sep", 0),
         ("tail_tile_heads_share_row", 2, 35, 4, 8, 0, "sep", 0),
         ("d24", 2, 20, 2, 24, 0, "sep", 0),
         ("one_past_tile", 1, 65, 1, 32, 0, "sep", 0),
         ("yaml_S400", 2, 400, 4, 64, 0, "sep", 0),
         ("d128", 1, 130, 2, 128, 0, "sep", 0),
         ("scores_30", 2, 35, 4, 8, 30.0, "sep", 0),
         ("qkv_blocks", 2, 35, 4, 8, 0, "qkv", 0),
         ("accumulate", 2, 20, 2, 24, 0, "sep", 1),
         ("nan_padding", 1, 65, 2, 16, 0, "pad", 0),
         ("nan_padding_vector_path", 1, 65, 2, 16, 0, "pad8", 0)]
IDS = [c[0] for c in CASES]


def _L():
    from yolo_dual_amd import _lib
    return _lib


def _P(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _err(got, want, scale=None):
    scale = float(want.abs().max()) if scale is None else scale
    return float((got.double().cpu() - want).abs().max()) / (scale if scale > 0 else 1.0)


@functools.lru_cache(maxsize=None)
def _problem(idx, dtype):
    """inputs exact in the compute dtype (float64 copies) and the float64 reference of one case"""
    _id, N, S, heads, d, smax, _layout, acc = CASES[idx]
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    gen = torch.Generator().manual_seed(100 + idx)
    C = heads * d
    draw = lambda: torch.randn(N, S, C, generator=gen, dtype=torch.float64).to(tdt).double()
    q, k, v, dout = draw(), draw(), draw(), draw()
    scale = d ** -0.5
    if smax:
        s = scale * torch.einsum("nihd,njhd->nhij", q.reshape(N, S, heads, d), k.reshape(N, S, heads, d))
        q = (q * (smax / float(s.abs().max()))).to(tdt).double()
    pre = [draw() for _ in range(3)] if acc else None
    out, lse = R.mha(q, k, v, heads, scale)
    dq, dk, dv = R.mha_grad(q, k, v, dout, heads, scale)
    return dict(q=q, k=k, v=v, dout=dout, pre=pre, scale=scale, tdt=tdt, ref=dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv))


def _run(idx, dtype):
    """-> dict of device results (float64, CPU) of one forward + backward through the ABI, after checking every guard"""
    _id, N, S, heads, d, _smax, layout, acc = CASES[idx]
    L = _L()
    pb = _problem(idx, dtype)
    tdt, C, rows = pb["tdt"], heads * d, N * S
    dt = L.YDL_BF16 if dtype == "bf16" else L.YDL_F32
    nan = float("nan")

    def rows_of(t64, ld):
        buf = torch.full((rows, ld), nan, dtype=tdt, device="cuda")
        buf[:, :C] = t64.reshape(rows, C).to(tdt).cuda()
        return buf
    if layout == "qkv":
        ld = 3 * C
        qkv = torch.cat([pb[n].reshape(rows, C) for n in ("q", "k", "v")], 1).to(tdt).cuda().contiguous()
        pq, pk, pv = _P(qkv), _P(qkv, C), _P(qkv, 2 * C)
        dqkv = torch.full((rows, ld), nan, dtype=tdt, device="cuda")
        pdq, pdk, pdv = _P(dqkv), _P(dqkv, C), _P(dqkv, 2 * C)
        grads = [dqkv[:, i * C:(i + 1) * C] for i in range(3)]
        ldo = C
    else:
        ld = ldo = C + {"pad": 2, "pad8": 8}.get(layout, 0)
        gq, gk, gv = rows_of(pb["q"], ld), rows_of(pb["k"], ld), rows_of(pb["v"], ld)
        pq, pk, pv = _P(gq), _P(gk), _P(gv)
        gbufs = [rows_of(pb["pre"][i], ld) if acc else torch.full((rows, ld), nan, dtype=tdt, device="cuda") for i in range(3)]
        pdq, pdk, pdv = (_P(b) for b in gbufs)
        grads = [b[:, :C] for b in gbufs]
    gout = torch.full((rows, ldo), nan, dtype=tdt, device="cuda")
    gdout = rows_of(pb["dout"], ldo)
    nstat = N * heads * S
    lse = torch.full((nstat + 64,), nan, dtype=torch.float32, device="cuda")
    wsn = L.lib().ydl_mha_bwd_ws_bytes(N, S, heads) // 4
    assert wsn == nstat
    ws = torch.full((wsn + 64,), nan, dtype=torch.float32, device="cuda")
    L.call("ydl_mha_fwd", dt, pq, ld, pk, ld, pv, ld, _P(gout), ldo, _P(lse), N, S, heads, d, pb["scale"], _stream())
    L.call("ydl_mha_bwd", dt, pq, ld, pk, ld, pv, ld, _P(gout), ldo, _P(lse), _P(gdout), ldo, pdq, pdk, pdv, ld, acc, _P(ws),
           N, S, heads, d, pb["scale"], _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(lse[nstat:]).all()) and bool(torch.isnan(ws[wsn:]).all()), "wrote past lse / the workspace"
    assert not bool(torch.isnan(ws[:wsn]).any())
    if ldo > C:
        assert bool(torch.isnan(gout[:, C:].float()).all()), "wrote into the padding of out"
    if layout.startswith("pad"):
        for b in gbufs:
            assert bool(torch.isnan(b[:, C:].float()).all()), "wrote into the padding of a gradient"
    res = {"out": gout[:, :C].double().cpu().reshape(N, S, C), "lse": lse[:nstat].double().cpu().reshape(N, heads, S)}
    for n, g in zip(("dq", "dk", "dv"), grads):
        res[n] = g.double().cpu().reshape(N, S, C)
    res["_raw"] = [g.clone() for g in grads]
    return res


def _want(pb, n):
    """expected value of a result: with accumulate the gradient is added to what the buffer held"""
    w = pb["ref"][n]
    if pb["pre"] is not None and n in ("dq", "dk", "dv"):
        w = w + pb["pre"][("dq", "dk", "dv").index(n)]
    return w


def _degenerate_scale(pb, n):
    """one token: dQ = dK = 0 exactly; the size of the terms that cancel"""
    other = pb["k"] if n == "dq" else pb["q"]
    return pb["scale"] * float(pb["dout"].abs().max()) * float(pb["v"].abs().max()) * float(other.abs().max())


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_mha_f32_matches_float64(idx):
    pb, res = _problem(idx, "f32"), _run(idx, "f32")
    for n, bound in (("out", 1e-5), ("lse", 1e-5), ("dq", 1e-4), ("dk", 1e-4), ("dv", 1e-4)):
        want = _want(pb, n)
        zero = float(pb["ref"][n].abs().max()) == 0.0
        e = _err(res[n], want, _degenerate_scale(pb, n) if zero else float(pb["ref"][n].abs().max()))
        print(f"f32 {IDS[idx]} {n}: {e:.3e}")
        assert e <= bound, f"{n}: {e:.3e} > {bound:.0e}"


def _torch_bf16(pb, heads):
    """the bf16 composition in torch on the GPU -> out, dq, dk, dv as float64 (N, S, C)"""
    N, S, C = pb["q"].shape
    d = C // heads
    h = lambda t: t.reshape(N, S, heads, d).permute(0, 2, 1, 3).to(torch.bfloat16).cuda().contiguous()
    q, k, v = (h(pb[n]).requires_grad_(True) for n in ("q", "k", "v"))
    s = (q @ k.transpose(-1, -2)).float() * pb["scale"]
    out = torch.softmax(s, -1).to(torch.bfloat16) @ v
    out.backward(h(pb["dout"]))
    r = lambda t: t.detach().double().cpu().permute(0, 2, 1, 3).reshape(N, S, C)
    return {"out": r(out), "dq": r(q.grad), "dk": r(k.grad), "dv": r(v.grad)}


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_mha_bf16_no_worse_than_twice_torch_bf16(idx):
    heads = CASES[idx][3]
    pb, res = _problem(idx, "bf16"), _run(idx, "bf16")
    tb = _torch_bf16(pb, heads)
    fails = []
    for n in ("out", "dq", "dk", "dv"):
        ref = pb["ref"][n]
        if float(ref.abs().max()) == 0.0:
            e = _err(res[n], _want(pb, n), _degenerate_scale(pb, n))
            print(f"bf16 {IDS[idx]} {n}: ours {e:.3e} of the cancelling terms (reference identically zero; torch {_err(tb[n], ref):.3e})")
            if e > 1e-4:
                fails.append(f"{n}: {e:.3e} > 1e-4 of the cancelling terms")
            continue
        scale = float(ref.abs().max())
        theirs_t = tb[n]
        if pb["pre"] is not None and n != "out":         # accumulate: torch's gradient added to the same bf16 buffer
            theirs_t = (theirs_t + pb["pre"][("dq", "dk", "dv").index(n)]).to(torch.bfloat16).double()
        ours, theirs = _err(res[n], _want(pb, n), scale), _err(theirs_t, _want(pb, n), scale)
        print(f"bf16 {IDS[idx]} {n}: ours {ours:.3e}  torch bf16 {theirs:.3e}")
        if ours > 2 * theirs:
            fails.append(f"{n}: ours {ours:.3e} > 2 x torch's {theirs:.3e}")
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mha_backward_is_bitwise_reproducible(dtype):
    idx = IDS.index("yaml_S400")
    a, b = _run(idx, dtype), _run(idx, dtype)
    for x, y in zip(a["_raw"], b["_raw"]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("d", [4, 12, 136])
def test_mha_refuses_other_head_dimensions(d):
    L = _L()
    t = torch.zeros(4, 2 * d, device="cuda")
    lse = torch.zeros(8, device="cuda")
    with pytest.raises(L.YdlError, match="multiple of 8 between 8 and 128"):
        L.call("ydl_mha_fwd", L.YDL_F32, _P(t), 2 * d, _P(t), 2 * d, _P(t), 2 * d, _P(t), 2 * d, _P(lse), 1, 4, 2, d, 1.0, _stream())
