"""GPU: the local self-attention op through the C ABI (ydl_local_attn_fwd / _bwd, ydl_attn_stem_table_fwd / _bwd) against the float64
closed form of tests/local_attn_ref.py: the output and every gradient (dQ, dK, dV^m, d rel_h, d rel_w, dE).

* f32: out < 1e-5, every gradient < 1e-4, relative to the reference tensor's max (the bound tests/test_gpu_deform.py applies to the
  sibling gather op).
* bf16: the reference is fed the bf16-rounded inputs.  Bound per tensor = 2 x the largest error measured over the cases below on an
  MI355X (BF16_MEASURED; the factor covers a change of seed, not a change of kernel).
* rows are allocated with NaN in every element outside [0, C) of a row (leading dimension > C, or the tail of the last 8-channel
  group): a read of one poisons the result, and a write to one is caught afterwards.
* two backward runs give bitwise-equal results; the workspace is sentinel-guarded beyond its queried size."""
import ctypes

import pytest
import torch

from tests import local_attn_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FA5A5A5
MIB_FLOATS = (1 << 20) // 4
F32_BOUND = {"out": 1e-5}          # every gradient: 1e-4
# largest error (relative to the reference tensor's max) over CASES in bf16 mode, measured on an MI355X
# (out 3.29e-3 at conv_k7, dQ 8.23e-3 at conv_k5, dK 5.47e-3 at conv_c64, dV 2.79e-3 at stem_m4, d rel_h 4.73e-3 and d rel_w 2.97e-3
# at conv_ld_acc / conv_k5; dE 3.74e-7 at stem_m4: it does not pass through the bf16-rounded `out`, only through f32 sums)
BF16_MEASURED = {"out": 3.29e-3, "dq": 8.23e-3, "dk": 5.47e-3, "dv": 2.79e-3, "drel_h": 4.73e-3, "drel_w": 2.97e-3, "de": 3.74e-7}

# (id, N, C, H, W, ks, m (0: AttentionConv form), extra leading dimension, accumulate)
CASES = [("conv_c24", 2, 24, 7, 5, 3, 0, 0, 0), ("conv_c64", 1, 64, 9, 11, 3, 0, 0, 0), ("conv_k5", 2, 16, 6, 6, 5, 0, 0, 0),
         ("conv_k7_window_larger_than_image", 1, 8, 3, 3, 7, 0, 0, 0), ("conv_c40_row", 1, 40, 1, 13, 3, 0, 0, 0),
         ("stem_m4", 2, 24, 7, 5, 3, 4, 0, 0), ("stem_m1", 1, 16, 4, 6, 3, 1, 0, 0),
         ("conv_ld_acc", 2, 24, 5, 6, 3, 0, 16, 1), ("stem_ld_acc", 1, 12, 5, 4, 3, 4, 4, 1)]


def _L():
    from yolo_dual_amd import _lib
    return _lib


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rows(t64, ld, tdt):
    """(N, C, H, W) float64 -> device rows [N*H*W][ld] of the compute dtype, NaN outside [0, C)"""
    N, C, H, W = t64.shape
    buf = torch.full((N * H * W, ld), float("nan"), dtype=tdt, device="cuda")
    buf[:, :C] = t64.permute(0, 2, 3, 1).reshape(-1, C).to(tdt).cuda()
    return buf


def _unrows(buf, N, C, H, W):
    return buf[:, :C].double().cpu().reshape(N, H, W, C).permute(0, 3, 1, 2)


def _pads_nan(buf, C):
    return buf.shape[1] == C or bool(torch.isnan(buf[:, C:].float()).all())


def _err(got, want):
    scale = float(want.abs().max())
    return float((got.double().cpu() - want).abs().max()) / (scale if scale > 0 else 1.0)


class Op:
    """one case on the device + its float64 reference"""

    def __init__(self, case, dtype):
        _id, N, C, H, W, ks, m, extra, acc = case
        L = _L()
        self.L, self.case = L, case
        self.dt, self.tdt = (L.YDL_BF16, torch.bfloat16) if dtype == "bf16" else (L.YDL_F32, torch.float32)
        self.mv = max(m, 1)
        self.ld = C + extra
        gen = torch.Generator().manual_seed(7 + len(_id) + C + ks)

        def draw(*shape, s=1.0):
            t = torch.randn(*shape, generator=gen, dtype=torch.float64) * s
            return t.to(self.tdt).double() if len(shape) == 4 else t.float().double()      # activations: exact in the compute dtype
        self.q, self.k = draw(N, C, H, W, s=0.8).requires_grad_(True), draw(N, C, H, W, s=0.8).requires_grad_(True)
        self.vs = [draw(N, C, H, W).requires_grad_(True) for _ in range(self.mv)]
        self.dout = draw(N, C, H, W)
        self.rel_h = self.rel_w = self.emb = None
        if m == 0:
            self.rel_h, self.rel_w = draw(C // 2, ks, s=0.8).requires_grad_(True), draw(C // 2, ks, s=0.8).requires_grad_(True)
        else:
            self.emb = torch.softmax(draw(m, ks * ks), 0).float().double().requires_grad_(True)
        self.pre = {n: draw(N, C, H, W) for n in ("dq", "dk")} if acc else {}
        if acc:
            self.pre["dv"] = [draw(N, C, H, W) for _ in range(self.mv)]
        out = R.local_attention(self.q, self.k, self.vs, ks, self.rel_h, self.rel_w, self.emb)
        out.backward(self.dout)
        self.ref = {"out": out.detach(), "dq": self.q.grad, "dk": self.k.grad, "dv": torch.stack([v.grad for v in self.vs])}
        if m == 0:
            self.ref.update(drel_h=self.rel_h.grad, drel_w=self.rel_w.grad)
        else:
            self.ref["de"] = self.emb.grad
        # device operands
        ld, tdt = self.ld, self.tdt
        self.gq, self.gk = _rows(self.q.detach(), ld, tdt), _rows(self.k.detach(), ld, tdt)
        self.gv = torch.stack([_rows(v.detach(), ld, tdt) for v in self.vs])
        self.gdout = _rows(self.dout, ld, tdt)
        f32 = lambda t: None if t is None else t.detach().float().cuda().contiguous()
        self.grel_h, self.grel_w, self.gemb = f32(self.rel_h), f32(self.rel_w), f32(self.emb)
        self.npix = N * H * W
        self.cp = (C + 7) // 8 * 8

    def forward(self):
        _id, N, C, H, W, ks, m, extra, acc = self.case
        self.gout = torch.full((self.npix, self.ld), float("nan"), dtype=self.tdt, device="cuda")
        self.lse = torch.empty(self.npix, self.cp, dtype=torch.float32, device="cuda")
        self.L.call("ydl_local_attn_fwd", self.dt, _P(self.gq), self.ld, _P(self.gk), self.ld, _P(self.gv), self.ld, self.npix * self.ld,
                    self.mv, _P(self.grel_h), _P(self.grel_w), _P(self.gemb), _P(self.gout), self.ld, _P(self.lse), N, H, W, C, ks, _stream())
        torch.cuda.synchronize()
        assert _pads_nan(self.gout, C), "forward wrote outside [0, C) of an output row"
        return _unrows(self.gout, N, C, H, W)

    def backward(self):
        _id, N, C, H, W, ks, m, extra, acc = self.case
        L, ld, tdt = self.L, self.ld, self.tdt
        if acc:
            dq, dk = _rows(self.pre["dq"], ld, tdt), _rows(self.pre["dk"], ld, tdt)
            dv = torch.stack([_rows(t, ld, tdt) for t in self.pre["dv"]])
        else:
            dq, dk = (torch.full((self.npix, ld), float("nan"), dtype=tdt, device="cuda") for _ in range(2))
            dv = torch.full((self.mv, self.npix, ld), float("nan"), dtype=tdt, device="cuda")
        q = L.lib().ydl_local_attn_bwd_ws_bytes(C, ks, self.mv) // 4
        assert q >= 1
        wsi = torch.full((max(2 * q, q + MIB_FLOATS),), SENT, dtype=torch.int32, device="cuda")
        drh = drw = de = None
        if m == 0:
            drh, drw = torch.zeros(C // 2, ks, device="cuda"), torch.zeros(C // 2, ks, device="cuda")
        else:
            de = torch.full((m, ks * ks), float("nan"), device="cuda")
        L.call("ydl_local_attn_bwd", self.dt, _P(self.gq), ld, _P(self.gk), ld, _P(self.gv), ld, self.npix * ld, self.mv,
               _P(self.grel_h), _P(self.grel_w), _P(self.gemb), _P(self.gout), ld, _P(self.lse), _P(self.gdout), ld,
               _P(dq), _P(dk), _P(dv), ld, self.npix * ld, acc, _P(drh), _P(drw), _P(de), _P(wsi.view(torch.float32)),
               N, H, W, C, ks, _stream())
        torch.cuda.synchronize()
        assert bool((wsi[q:] == SENT).all()), "workspace written beyond ydl_local_attn_bwd_ws_bytes"
        assert _pads_nan(dq, C) and _pads_nan(dk, C) and all(_pads_nan(dv[i], C) for i in range(self.mv)), "gradient written outside [0, C)"
        raw = {"dq": dq, "dk": dk, "dv": dv, "drel_h": drh, "drel_w": drw, "de": de}
        got = {"dq": _unrows(dq, N, C, H, W), "dk": _unrows(dk, N, C, H, W),
               "dv": torch.stack([_unrows(dv[i], N, C, H, W) for i in range(self.mv)])}
        if m == 0:
            got.update(drel_h=drh.double().cpu(), drel_w=drw.double().cpu())
        else:
            got["de"] = de.double().cpu()
        return got, {k: v for k, v in raw.items() if v is not None}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_op_against_float64(case, dtype):
    op = Op(case, dtype)
    acc = case[8]
    errs = {"out": _err(op.forward(), op.ref["out"])}
    got, raw = op.backward()
    for name, g in got.items():
        want = op.ref[name]
        if acc and name in ("dq", "dk", "dv"):
            pre = op.pre[name]
            want = want + (torch.stack(pre) if isinstance(pre, list) else pre)
        errs[name] = _err(g, want)
    print(f"[local_attn] {case[0]} {dtype} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for name, e in errs.items():
        bound = (F32_BOUND.get(name, 1e-4)) if dtype == "f32" else 2 * BF16_MEASURED[name]
        assert e < bound, (case[0], dtype, name, e, bound)
    got2, raw2 = op.backward()
    for name in raw:
        a, b = raw[name], raw2[name]
        a, b = (a[..., :case[2]], b[..., :case[2]]) if name in ("dq", "dk", "dv") else (a, b)
        assert torch.equal(a, b), (case[0], dtype, name, "two backward runs differ")


@pytest.mark.parametrize("m,Cg,ks", [(4, 24, 3), (1, 4, 3), (3, 10, 5), (4, 6, 7)])
def test_stem_table(m, Cg, ks):
    L = _L()
    gen = torch.Generator().manual_seed(m * 100 + Cg + ks)
    mix, ea, eb = (torch.randn(*s, generator=gen).double().requires_grad_(True) for s in ((m, Cg), (Cg, ks), (Cg, ks)))
    dE = torch.randn(m, ks * ks, generator=gen).double()
    E = R.stem_table(mix, ea, eb)
    E.backward(dE)
    g = [t.detach().float().cuda() for t in (mix, ea, eb)]
    Eg = torch.empty(m, ks * ks, device="cuda")
    L.call("ydl_attn_stem_table_fwd", _P(g[0]), _P(g[1]), _P(g[2]), _P(Eg), m, Cg, ks, _stream())
    grads = [torch.zeros_like(t) for t in g]
    L.call("ydl_attn_stem_table_bwd", _P(g[0]), _P(g[1]), _P(g[2]), _P(Eg), _P(dE.float().cuda()), _P(grads[0]), _P(grads[1]), _P(grads[2]),
           m, Cg, ks, _stream())
    torch.cuda.synchronize()
    errs = [_err(Eg, E.detach())] + [_err(a, b.grad) for a, b in zip(grads, (mix, ea, eb))]
    print(f"[stem_table] m={m} Cg={Cg} ks={ks} " + " ".join(f"{e:.2e}" for e in errs))
    assert errs[0] < 1e-5 and all(e < 1e-4 for e in errs[1:]), errs


def test_arguments_are_checked():
    L = _L()
    t = torch.zeros(64, device="cuda")
    args = lambda C, ks, m, emb: (L.YDL_F32, _P(t), 8, _P(t), 8, _P(t), 8, 0, m, None, None, emb, _P(t), 8, None, 1, 1, 1, C, ks, _stream())
    for bad in (args(8, 4, 1, None), args(8, 3, 2, None), args(8, 3, 9, _P(t)), args(16, 3, 1, None)):
        with pytest.raises(L.YdlError):
            L.call("ydl_local_attn_fwd", *bad)
