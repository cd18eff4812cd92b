"""The BatchNorm-statistics workspaces of the forward convolution, held to their C-ABI contract (include/ydl.h) kernel by kernel.

Partial rows: ydl_conv_fwd(..., stats_ws, ...) writes ydl_conv_fwd_grid_m rows of (sum, M2) per channel, row b covering
min(block_m, M - b*block_m) pixels, into a workspace of ydl_conv_fwd_stats_ws_bytes; ydl_bn_finalize merges them.  Replica sums:
ydl_conv_fwd_sums adds (sum, sum of squares) into [YDL_BN_REPLICAS][2][Cp], read by ydl_bn_act_fwd_sums.  Every case calls the C ABI
directly (no tape, no cached geometry), records which kernel ran, and checks against float64 on the same operands (the bf16-rounded x
and w in bf16 mode):

* guards — the workspace is allocated at max(2 x query, query + 1 MiB) and filled with a sentinel, as is a tail after y: nothing at or
  beyond row grid_m may change (the rows up to the query's end belong to ydl_bn_finalize's level-1 merge), every promised row is
  written, M2 >= 0;
* the rows reconstruct the f64 sum S = sum_b s_b and sum of squares Q = sum_b (M2_b + s_b^2 / n_b) without assuming a pixel order (the
  rows may cover 2-D patches);
* ydl_bn_finalize / ydl_bn_act_fwd_sums give mean, invstd, scale, shift and the running statistics of f64.

A second input family puts a channel mean of r standard deviations on the conv output (a constant input channel read by the centre
tap), r in {0, 4, 32}: the f32 statistics lose precision as (1 + r^2) where they cancel.

Bounds (mean errors in units of the channel's standard deviation sigma_c, variances relative): about 10x the worst error measured on
an MI355X, capped at 1e-4 (the bound of the analysis: the partial-row merges run in double, the only f32 cancellation is within a
tile of <= 256 pixels).  Replica sums add raw f32 sums of squares: their variance error grows as 3e-7 x r^2 (measured) and
is not asserted at r = 32.  Kernels whose statistics are those of bf16-ROUNDED values (the accumulating point-wise launch on its
transposed-store path) keep the 1e-4 bounds: the rounding alone is 2^-9 per value.  (The weights-in-registers kernel used to be
one of them; it reduces its f32 accumulators now and is held to the f32 bounds.)"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = 0x7FA5A5A5                   # a NaN bit pattern no kernel produces
MIB_FLOATS = (1 << 20) // 4
EPS, MOM = 1e-3, 0.1

# (mean, variance) bounds by statistics form and r (None: the N(0.25, 1) family of the kernel table).  Worst measured: partial rows
# 6.5e-8 / 1.3e-7 (r <= 0), 4.9e-7 / 9.1e-7 (r = 4), 4.2e-6 / 5.7e-5 (r = 32); replica sums 1.5e-7 / 4.3e-7, 9.2e-7 / 7.5e-6
TOLS = {("rows", None): (1e-6, 2e-6), ("rows", 0): (1e-6, 2e-6), ("rows", 4): (5e-6, 1e-5), ("rows", 32): (5e-5, 1e-4),
        ("sums", None): (1e-6, 5e-6), ("sums", 0): (1e-6, 5e-6), ("sums", 4): (1e-5, 1e-4), ("sums", 32): (1e-4, None)}
BF16_STATS_TOL = (1e-4, 1e-4)       # measured 1.4e-5 / 4.7e-5


def _L():
    from yolo_dual_amd import _lib as L
    return L


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sentinel(n, dev="cuda"):
    return torch.full((n,), SENT, dtype=torch.int32, device=dev)


class Case:
    """one geometry: operands (host, f32 values exact in the compute dtype) and the f64 reference of y = conv(x, w) [+ y0]"""

    def __init__(self, dtype, N, c1, c2, k, s, H, W, r=None, accumulate=0, ldy=None, ldw=0, ldx=None, seed=0):
        L = _L()
        self.dt = L.YDL_BF16 if dtype == "bf16" else L.YDL_F32
        self.tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.N, self.c1, self.c2, self.k, self.s, self.H, self.W = N, c1, c2, k, s, H, W
        self.p = k // 2
        self.Ho, self.Wo = (H + 2 * self.p - k) // s + 1, (W + 2 * self.p - k) // s + 1
        self.M = N * self.Ho * self.Wo
        self.cp_in = (c1 + 7) // 8 * 8
        self.cp = (c2 + 7) // 8 * 8
        self.ldx = ldx or self.cp_in
        self.ldy = ldy or self.cp
        self.ldw = ldw
        self.accumulate = accumulate
        rs = np.random.RandomState(seed + 7 * c1 + 13 * c2 + H)
        x = np.zeros((N, H, W, self.ldx), np.float32)
        x[..., :c1] = rs.standard_normal((N, H, W, c1)) + 0.25
        K = k * k * c1
        w = np.zeros((c2, k, k, self.cp_in), np.float32)
        w[..., :c1] = rs.standard_normal((c2, k, k, c1)) / np.sqrt(K)
        if r is not None:
            # offset family: input channel 0 is the constant 1, read by the centre tap only (every output pixel sees it, borders too),
            # with a per-channel weight of r x the spread the other weights give the output
            x[..., 0] = 1.0
            w[:, :, :, 0] = 0.0
            sig = np.sqrt((w[..., 1:c1].astype(np.float64) ** 2).reshape(c2, -1).sum(1) * (1 + 0.25 ** 2))
            w[:, k // 2, k // 2, 0] = r * sig * rs.uniform(0.9, 1.1, c2)
        self.x = torch.from_numpy(x).to(self.tdt)
        self.w = torch.from_numpy(w).to(self.tdt)
        self.y0 = torch.from_numpy(rs.standard_normal((self.M, c2)).astype(np.float32)).to(self.tdt) if accumulate else None
        self.gamma = torch.from_numpy(rs.uniform(0.5, 1.5, c2).astype(np.float32))
        self.beta = torch.from_numpy(rs.uniform(-0.3, 0.3, c2).astype(np.float32))
        self.geom = L.ConvGeom(N, H, W, c1, self.Ho, self.Wo, c2, k, s, self.p, self.ldx, self.ldy, ldw)
        self._ref = None

    # ---- float64 reference: im2col GEMM on the device, one image at a time
    def ref(self):
        if self._ref is None:
            dev = torch.device("cuda")
            xg = self.x.to(dev).double()[..., :self.cp_in].permute(0, 3, 1, 2)
            wm = self.w.to(dev).double().permute(0, 3, 1, 2).reshape(self.c2, -1)
            ys = []
            for n in range(self.N):
                cols = F.unfold(xg[n:n + 1], self.k, padding=self.p, stride=self.s)[0]
                ys.append((wm @ cols).t())
            y = torch.cat(ys)
            if self.y0 is not None:
                y = y + self.y0.to(dev).double()
            mean = y.mean(0)
            var = ((y - mean) ** 2).mean(0)
            self._ref = dict(S=y.sum(0), Q=(y * y).sum(0), mean=mean, var=var)
        return self._ref

    # ---- device operands
    def operands(self):
        dev = torch.device("cuda")
        xg = self.x.reshape(-1).to(dev)
        if self.ldw:
            w = torch.zeros(self.c2, self.ldw, dtype=self.tdt)
            w[:, :self.k * self.k * self.cp_in] = self.w.reshape(self.c2, -1)
            # the other column blocks of the wider matrix carry values that must not be read
            w[:, self.k * self.k * self.cp_in:] = 3.0
            wg = w.to(dev)
        else:
            wg = self.w.reshape(-1).to(dev)
        es = 2 if self.tdt == torch.bfloat16 else 4
        ny = self.M * self.ldy
        tail = MIB_FLOATS * 4 // es
        ybuf = torch.zeros(ny + tail, dtype=self.tdt, device=dev)
        if self.y0 is not None:
            ybuf[:ny].view(self.M, self.ldy)[:, :self.c2] = self.y0.to(dev)
        if es == 2:
            ybuf[ny:].view(torch.int16).fill_(0x7FA5)
        else:
            ybuf[ny:].view(torch.int32).fill_(SENT)
        return xg, wg, ybuf, ny

    def y_tail_intact(self, ybuf, ny):
        if self.tdt == torch.bfloat16:
            return bool((ybuf[ny:].view(torch.int16) == 0x7FA5).all())
        return bool((ybuf[ny:].view(torch.int32) == SENT).all())

    def achieved_r(self):
        R = self.ref()
        return float((R["mean"].abs() / R["var"].sqrt()).median())


def _bn_ref(R, gamma, beta, M):
    dev = R["mean"].device
    g, b = gamma.to(dev).double(), beta.to(dev).double()
    invstd = 1.0 / torch.sqrt(R["var"] + EPS)
    scale = g * invstd
    shift = b - R["mean"] * scale
    rm = MOM * R["mean"]
    rv = (1 - MOM) * 1.0 + MOM * R["var"] * M / (M - 1)
    return dict(mean=R["mean"], invstd=invstd, scale=scale, shift=shift, rm=rm, rv=rv)


def _bn_errors(got, R, gamma, beta, M):
    """worst errors of the coefficient vectors: mean in sigma, the rest relative (shift in units of |beta| + |scale| sigma)"""
    ref = _bn_ref(R, gamma, beta, M)
    sig = R["var"].sqrt()
    g = {k: v.double() for k, v in got.items()}
    var_from_invstd = 1.0 / g["invstd"] ** 2 - EPS
    e = dict(mean=float(((g["mean"] - ref["mean"]).abs() / sig).max()),
             var=float(((var_from_invstd - R["var"]).abs() / R["var"]).max()),
             invstd=float(((g["invstd"] - ref["invstd"]).abs() / ref["invstd"]).max()),
             scale=float(((g["scale"] - ref["scale"]).abs() / ref["scale"].abs()).max()),
             shift=float(((g["shift"] - ref["shift"]).abs() /
                          (beta.to(sig.device).double().abs() + ref["scale"].abs() * (ref["mean"].abs() + sig))).max()),
             rm=float(((g["rm"] - ref["rm"]).abs() / (MOM * sig)).max()),
             rv=float(((g["rv"] - ref["rv"]).abs() / (MOM * R["var"])).max()))
    return e


def _coef_buffers(c2):
    dev = torch.device("cuda")
    out = {k: torch.zeros(c2, device=dev) for k in ("mean", "invstd", "scale", "shift", "rm")}
    out["rv"] = torch.ones(c2, device=dev)
    return out


def run_partial_rows(case, knobs=()):
    """ydl_conv_fwd with partial rows + ydl_bn_finalize; returns (kernel name, fwd finalize-kernel name, measured errors); raises
    AssertionError on a contract violation"""
    L = _L()
    lib = L.lib()
    gp = ctypes.byref(case.geom)
    for key, val in knobs:
        L.debug_set(key, val)
    try:
        q = lib.ydl_conv_fwd_stats_ws_bytes(gp, case.dt)
        gm, bm = lib.ydl_conv_fwd_grid_m(gp, case.dt), lib.ydl_conv_fwd_block_m(gp, case.dt)
        assert q > 0 and q % 4 == 0 and gm > 0 and bm > 0, (q, gm, bm)
        assert gm * bm >= case.M > (gm - 1) * bm, (gm, bm, case.M)
        qf = q // 4
        nws = max(2 * qf, qf + MIB_FLOATS)
        wsi = _sentinel(nws)
        ws = wsi.view(torch.float32)
        xg, wg, ybuf, ny = case.operands()
        L.call("ydl_conv_fwd", gp, case.dt, _P(xg), _P(wg), _P(ybuf), _P(ws), case.accumulate, _stream())
        torch.cuda.synchronize()
        kern = L.last_kernel(0)
    finally:
        for key, _ in knobs:
            L.debug_set(key, -1 if key == 19 else 1)
    cp, c2 = case.cp, case.c2
    rows_end = gm * 2 * cp
    # nothing beyond the promised rows: the finalize's room and everything after the query
    assert bool((wsi[rows_end:] == SENT).all()), (kern, "written beyond grid_m rows", int((wsi[rows_end:] != SENT).sum()))
    assert case.y_tail_intact(ybuf, ny), (kern, "written beyond y")
    rows = ws[:rows_end].view(gm, 2, cp)
    rowsi = wsi[:rows_end].view(gm, 2, cp)[:, :, :c2]
    assert not bool((rowsi == SENT).any()), (kern, "promised row not written", int((rowsi == SENT).sum()))
    assert bool(torch.isfinite(rows[:, :, :c2]).all()), (kern, "non-finite partial")
    assert float(rows[:, 1, :c2].min()) >= 0.0, (kern, "negative M2")
    # S and Q from the rows, with the per-row pixel counts of the contract
    R = case.ref()
    nb = torch.full((gm,), float(bm), dtype=torch.float64, device=rows.device)
    nb[-1] = case.M - (gm - 1) * bm
    s = rows[:, 0, :c2].double()
    S = s.sum(0)
    Q = (rows[:, 1, :c2].double() + s * s / nb[:, None]).sum(0)
    sig = R["var"].sqrt()
    errs = dict(S=float(((S - R["S"]).abs() / (case.M * sig)).max()),
                Q=float(((Q - R["Q"]).abs() / R["Q"]).max()))
    # finalize with the queried geometry
    cb = _coef_buffers(c2)
    gam, bet = case.gamma.cuda(), case.beta.cuda()
    L.call("ydl_bn_finalize", _P(ws), gm, bm, case.M, c2, _P(gam), _P(bet), EPS, MOM, _P(cb["rm"]), _P(cb["rv"]), _P(cb["mean"]),
           _P(cb["invstd"]), _P(cb["scale"]), _P(cb["shift"]), 1, _stream())
    torch.cuda.synchronize()
    # the finalize's level-1 rows stay inside the room the query reserved
    assert bool((wsi[qf:] == SENT).all()), (kern, L.last_kernel(3), "finalize wrote beyond ydl_conv_fwd_stats_ws_bytes")
    errs.update(_bn_errors(cb, R, case.gamma, case.beta, case.M))
    return kern, L.last_kernel(3), errs


def run_replica_sums(case, knobs=()):
    """ydl_conv_fwd_sums + ydl_bn_act_fwd_sums; returns (kernel name, measured errors)"""
    L = _L()
    cp, c2 = case.cp, case.c2
    slab = 8 * 2 * cp
    bufi = _sentinel(slab + MIB_FLOATS)
    bufi[:slab] = 0
    sums = bufi.view(torch.float32)
    gp = ctypes.byref(case.geom)
    for key, val in knobs:
        L.debug_set(key, val)
    try:
        xg, wg, ybuf, ny = case.operands()
        L.call("ydl_conv_fwd_sums", gp, case.dt, _P(xg), _P(wg), _P(ybuf), _P(sums), case.accumulate, _stream())
        torch.cuda.synchronize()
        kern = L.last_kernel(0)
    finally:
        for key, _ in knobs:
            L.debug_set(key, -1 if key == 19 else 1)
    assert bool((bufi[slab:] == SENT).all()), (kern, "written beyond the replica slab")
    assert case.y_tail_intact(ybuf, ny), (kern, "written beyond y")
    R = case.ref()
    tot = sums[:slab].view(8, 2, cp)[:, :, :c2].double().sum(0)
    sig = R["var"].sqrt()
    errs = dict(S=float(((tot[0] - R["S"]).abs() / (case.M * sig)).max()),
                Q=float(((tot[1] - R["Q"]).abs() / R["Q"]).max()))
    cb = _coef_buffers(c2)
    gam, bet = case.gamma.cuda(), case.beta.cuda()
    out = torch.zeros(case.M * cp, dtype=case.tdt, device="cuda")
    y = ybuf[:ny]
    L.call("ydl_bn_act_fwd_sums", case.dt, _P(y), case.ldy, _P(sums), cp, case.M, _P(gam), _P(bet), EPS, MOM, _P(cb["rm"]), _P(cb["rv"]),
           _P(cb["mean"]), _P(cb["invstd"]), _P(cb["scale"]), _P(cb["shift"]), 1, None, 0, 0, L.ACT_NONE, _P(out), cp, case.M, c2, cp,
           _stream())
    torch.cuda.synchronize()
    errs.update(_bn_errors(cb, R, case.gamma, case.beta, case.M))
    return kern, errs


# (tag, dtype, N, c1, c2, k, s, H, W, extra Case arguments, debug knobs, expected kernel-name prefix with partial rows)
K19_OFF = ((19, 0),)
ROWS = [
    # the thin-input stem kernel (12 -> 64 on a 16-channel stride; 13 images of 50 x 128: ragged segments)
    ("stem", "bf16", 13, 12, 64, 3, 1, 50, 128, dict(ldx=16), (), "stem_kernel<bf16,16,64>"),
    # point-wise streaming kernel: every K-row width and wave count
    ("pw_f32_rb128", "f32", 4, 32, 128, 1, 1, 160, 160, {}, (), "pw_kernel<f32,128,8,4,"),
    ("pw_f32_rb256", "f32", 4, 64, 128, 1, 1, 160, 160, {}, (), "pw_kernel<f32,256,8,4,"),
    ("pw_f32_rb512_ct4", "f32", 4, 128, 64, 1, 1, 160, 160, {}, (), "pw_kernel<f32,512,4,4,"),
    ("pw_f32_rb512_nw8", "f32", 4, 128, 128, 1, 1, 160, 160, {}, (), "pw_kernel<f32,512,8,8,"),
    ("pw_bf16_rb128", "bf16", 4, 64, 128, 1, 1, 160, 160, {}, (), "pw_kernel<bf16,128,4,4,"),
    ("pw_bf16_rb256", "bf16", 4, 128, 128, 1, 1, 160, 160, {}, (), "pw_kernel<bf16,256,4,4,"),
    ("pw_bf16_rb512", "bf16", 4, 256, 64, 1, 1, 160, 160, {}, (), "pw_kernel<bf16,512,4,4,"),
    ("pw_bf16_rb512_nw8", "bf16", 4, 256, 256, 1, 1, 160, 160, {}, (), "pw_kernel<bf16,512,8,8,"),
    # ... accumulating (the statistics include the previous y) and a column block of a wider weight matrix (the commuted concat)
    ("pw_bf16_acc", "bf16", 4, 128, 128, 1, 1, 128, 128, dict(accumulate=1), (), "pw_kernel<bf16,256,4,4,"),
    ("pw_f32_acc_ldw", "f32", 4, 64, 128, 1, 1, 160, 160, dict(accumulate=1, ldw=200), (), "pw_kernel<f32,256,8,4,"),
    ("pw_bf16_ldw", "bf16", 4, 64, 128, 1, 1, 160, 160, dict(ldw=192), (), "pw_kernel<bf16,128,4,4,"),
    # register-staged tiles, f32
    ("tile_f32_128x128", "f32", 4, 128, 128, 3, 1, 160, 160, {}, (), "igemm_kernel<f32,128,128,8"),
    ("tile_f32_128x64", "f32", 4, 64, 64, 3, 1, 160, 160, {}, (), "igemm_kernel<f32,128,64,4"),
    ("tile_f32_128x16", "f32", 2, 32, 16, 3, 1, 64, 72, {}, (), "igemm_kernel<f32,128,16"),
    ("tile_f32_64x128_c130", "f32", 2, 32, 130, 3, 1, 100, 100, {}, (), "igemm_kernel<f32,64,128"),
    ("tile_f32_64x64", "f32", 2, 32, 64, 3, 1, 48, 48, {}, (), "igemm_kernel<f32,64,64"),
    ("tile_f32_s2", "f32", 4, 128, 256, 3, 2, 160, 160, {}, (), "igemm_kernel<f32,128,64,4"),
    ("tile_f32_ldw", "f32", 2, 64, 96, 1, 1, 40, 40, dict(ldw=136), (), "igemm_kernel<f32,"),
    # > 1024 partial rows: ydl_bn_finalize's two-level merge
    ("tile_f32_two_level", "f32", 4, 16, 32, 3, 1, 192, 192, {}, (), "igemm_kernel<f32,128,"),
    # register-staged tiles, bf16 (Cin not a multiple of 64)
    ("tile_bf16_128x128", "bf16", 4, 96, 128, 3, 1, 160, 160, {}, (), "igemm_kernel<bf16,128,128,8"),
    ("tile_bf16_128x64", "bf16", 4, 96, 64, 3, 1, 160, 160, {}, (), "igemm_kernel<bf16,128,64,4"),
    ("tile_bf16_128x16", "bf16", 2, 32, 16, 3, 1, 64, 72, {}, (), "igemm_kernel<bf16,128,16"),
    ("tile_bf16_64x128_c130", "bf16", 2, 32, 130, 3, 1, 100, 100, {}, (), "igemm_kernel<bf16,64,128"),
    ("tile_bf16_64x64", "bf16", 2, 32, 64, 3, 1, 48, 48, {}, (), "igemm_kernel<bf16,64,64"),
    # LDS-DMA ring kernels on maps that are not multiples of 8 x 16
    ("ring7", "bf16", 2, 64, 128, 3, 1, 152, 152, {}, K19_OFF, "igemm2_kernel<128,128,8,4,2>"),
    ("ring7_persistent", "bf16", 8, 64, 128, 3, 1, 152, 152, {}, (), "igemm2_kernel<128,128,8,4,2>:persistent"),
    ("ring9", "bf16", 1, 128, 128, 3, 1, 72, 88, {}, (), "igemm2_kernel<64,128,4,2,3>"),
    ("ring13", "bf16", 4, 128, 64, 3, 1, 152, 152, {}, (), "igemm2_kernel<128,64,8,4,2>"),
    ("ring15", "bf16", 4, 128, 128, 3, 1, 152, 152, {}, K19_OFF, "igemm2_kernel<256,128,8,4,3,stg>"),
    ("ring24", "bf16", 4, 128, 128, 3, 1, 152, 152, {}, (), "igemm2l_kernel<256,128,8+4,3>"),
    ("ring25", "bf16", 2, 128, 128, 3, 1, 72, 88, {}, (), "igemm2l_kernel<128,128,8+4,3>"),
    ("ring29_c150", "bf16", 3, 64, 150, 3, 1, 75, 83, dict(ldy=152), (), "igemm2l_kernel<128,128,4+4,2>"),
    ("ring29_acc", "bf16", 2, 64, 128, 3, 1, 152, 152, dict(accumulate=1), (), "igemm2l_kernel<128,128,4+4,2>"),
    # patch-form kernels (halo_ok): BN = 128 from ids 24, 15 (loaders off), 29 and 7; BN = 64 from id 13
    ("patch24", "bf16", 4, 128, 128, 3, 1, 160, 160, {}, (), "igemm2h_kernel<128,128,2>"),
    ("patch15", "bf16", 4, 128, 128, 3, 1, 160, 160, {}, K19_OFF, "igemm2h_kernel<128,128,2>"),
    ("patch29_onep", "bf16", 2, 64, 128, 3, 1, 160, 160, {}, (), "igemm2h_kernel<128,128,2>"),
    ("patch7_onep", "bf16", 2, 64, 128, 3, 1, 160, 160, {}, K19_OFF, "igemm2h_kernel<128,128,2>"),
    ("patch13_onep", "bf16", 8, 64, 64, 3, 1, 96, 160, {}, (), "igemm2h_kernel<128,64,2>"),
    ("patch13_s3", "bf16", 4, 128, 64, 3, 1, 160, 160, {}, (), "igemm2h_kernel<128,64,3>"),
    # the weights-in-registers kernel writes no partial rows: this geometry takes it only with replica sums
    ("wreg_refused", "bf16", 8, 64, 64, 3, 1, 160, 160, {}, (), "igemm2h_kernel<128,64,2>"),
]
ROW_IDS = [r[0] for r in ROWS]
ROW = {r[0]: r for r in ROWS}


def make_case(tag, r=None):
    _t, dtype, N, c1, c2, k, s, H, W, extra, knobs, expect = ROW[tag]
    return Case(dtype, N, c1, c2, k, s, H, W, r=r, **extra), knobs, expect


def _check_errs(errs, tag, mode, r=None, bf16_stats=False):
    mean_tol, var_tol = BF16_STATS_TOL if bf16_stats else TOLS[(mode, r)]
    assert errs["S"] < mean_tol and errs["mean"] < mean_tol and errs["rm"] < mean_tol, (tag, mode, r, errs)
    if var_tol is None:
        return
    for key in ("Q", "var", "invstd", "scale", "rv"):
        assert errs[key] < var_tol, (tag, mode, r, key, errs)
    assert errs["shift"] < mean_tol + var_tol, (tag, mode, r, errs)


@pytest.mark.parametrize("tag", ROW_IDS)
def test_partial_rows_contract(tag):
    case, knobs, expect = make_case(tag)
    kern, fin, errs = run_partial_rows(case, knobs)
    assert kern.startswith(expect), (tag, kern, "expected", expect)
    if tag == "tile_f32_two_level":
        assert fin == "bn_finalize<two-level>", fin
    _check_errs(errs, tag, "rows", bf16_stats=tag in BF16_STATS)


# replica sums, same table: the same kernels, but for the weights-in-registers kernel, which takes its geometry only here
SUMS_EXPECT = {"wreg_refused": "igemm2w_kernel<64"}
# statistics of bf16-rounded values: (tag, form)
BF16_STATS = {"pw_bf16_acc"}
BF16_STATS_SUMS = {"pw_bf16_acc"}


@pytest.mark.parametrize("tag", ROW_IDS)
def test_replica_sums_contract(tag):
    case, knobs, expect = make_case(tag)
    kern, errs = run_replica_sums(case, knobs)
    assert kern.startswith(SUMS_EXPECT.get(tag, expect.split(":")[0])), (tag, kern)
    _check_errs(errs, tag, "sums", bf16_stats=tag in BF16_STATS_SUMS)


# the r axis: one row per kernel family
R_ROWS = ["stem", "pw_f32_rb256", "pw_bf16_rb256", "tile_f32_128x64", "tile_bf16_128x64", "ring24", "ring13", "patch24", "patch13_s3"]


@pytest.mark.parametrize("r", [0, 4, 32])
@pytest.mark.parametrize("tag", R_ROWS)
def test_offset_mean_statistics(tag, r):
    case, knobs, expect = make_case(tag, r=r)
    ra = case.achieved_r()
    if r:
        assert r / 2 <= ra <= 2 * r, (tag, r, ra)
    else:
        assert ra < 1.0, (tag, ra)
    kern, _fin, errs = run_partial_rows(case, knobs)
    assert kern.startswith(expect), (tag, kern)
    _check_errs(errs, tag, "rows", r)
    kern, errs = run_replica_sums(case, knobs)
    _check_errs(errs, tag, "sums", r)




# ---- the other workspaces the ABI sizes: the same guard around each (allocated at max(2 x query, query + 1 MiB), sentinel-filled,
# nothing at or beyond the query may change), float64 references where the value is not pinned elsewhere

def _guarded_ws(nbytes):
    q = nbytes // 4
    assert nbytes > 0 and nbytes % 4 == 0 and q >= 1, nbytes
    wsi = _sentinel(max(2 * q, q + MIB_FLOATS))
    return wsi, wsi.view(torch.float32), q


def _intact(wsi, q):
    return bool((wsi[q:] == SENT).all())


def run_bn_stats(dtype, npix, C, ldy, r):
    """ydl_bn_stats + ydl_bn_finalize; returns (finalize kernel, errors)"""
    L = _L()
    lib = L.lib()
    dt, tdt = (L.YDL_BF16, torch.bfloat16) if dtype == "bf16" else (L.YDL_F32, torch.float32)
    rs = np.random.RandomState(npix + C)
    y = rs.standard_normal((npix, ldy)).astype(np.float32) + r * rs.uniform(0.8, 1.2, ldy).astype(np.float32)
    yt = torch.from_numpy(y).to(tdt)
    bm = lib.ydl_bn_stats_block_m()
    gm = (npix + bm - 1) // bm
    cp = (C + 7) // 8 * 8
    wsi, ws, q = _guarded_ws(lib.ydl_bn_stats_ws_bytes(npix, C))
    assert q >= (gm + (gm + 63) // 64) * 2 * cp
    yg = yt.cuda()
    L.call("ydl_bn_stats", dt, _P(yg), ldy, _P(ws), npix, C, _stream())
    torch.cuda.synchronize()
    assert bool((wsi[gm * 2 * cp:] == SENT).all()), "written beyond the nblocks rows"
    rows = ws[:gm * 2 * cp].view(gm, 2, cp)[:, :, :C].double()
    assert not bool((wsi[:gm * 2 * cp].view(gm, 2, cp)[:, :, :C] == SENT).any()), "promised row not written"
    assert float(rows[:, 1].min()) >= 0.0
    yr = yt[:, :C].cuda().double()
    mean = yr.mean(0)
    var = ((yr - mean) ** 2).mean(0)
    R = dict(S=yr.sum(0), Q=(yr * yr).sum(0), mean=mean, var=var)
    nb = torch.full((gm,), float(bm), dtype=torch.float64, device="cuda")
    nb[-1] = npix - (gm - 1) * bm
    S = rows[:, 0].sum(0)
    Q = (rows[:, 1] + rows[:, 0] ** 2 / nb[:, None]).sum(0)
    sig = var.sqrt()
    errs = dict(S=float(((S - R["S"]).abs() / (npix * sig)).max()), Q=float(((Q - R["Q"]).abs() / R["Q"]).max()))
    cb = _coef_buffers(C)
    gam, bet = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    L.call("ydl_bn_finalize", _P(ws), gm, bm, npix, C, _P(gam), _P(bet), EPS, MOM, _P(cb["rm"]), _P(cb["rv"]), _P(cb["mean"]),
           _P(cb["invstd"]), _P(cb["scale"]), _P(cb["shift"]), 1, _stream())
    torch.cuda.synchronize()
    assert _intact(wsi, q), "finalize wrote beyond ydl_bn_stats_ws_bytes"
    errs.update(_bn_errors(cb, R, torch.ones(C), torch.zeros(C), npix))
    return L.last_kernel(3), errs


# (dtype, npix, C, ldy, r): npix below / at / above a multiple of block_m (64), more than 1024 rows (two-level finalize), C % 8 != 0
BN_STATS = [("f32", 64 * 37 - 5, 64, 64, 0), ("f32", 64 * 37, 64, 64, 4), ("f32", 64 * 37 + 1, 64, 64, 32),
            ("f32", 64 * 1024 + 64 * 70 + 17, 48, 48, 4), ("f32", 5000, 20, 24, 32), ("f32", 3, 8, 8, 0),
            ("bf16", 64 * 37 - 5, 64, 64, 0), ("bf16", 64 * 37, 64, 64, 4), ("bf16", 64 * 37 + 1, 64, 64, 32),
            ("bf16", 64 * 1024 + 64 * 70 + 17, 48, 48, 4), ("bf16", 5000, 20, 24, 32), ("bf16", 3, 8, 8, 0)]
# (mean, variance) bounds by r, about 10x the worst measured: mean 4.3e-8 / 4.1e-7 / 3.0e-6 (r = 0 / 4 / 32); variance 4e-7 at every r,
# running variance 8.8e-7 (the f32 rounding of its update) and 3.3e-6 at npix = 3 (unbiased factor 3/2)
BN_STATS_TOLS = {0: (5e-7, 3e-5), 4: (5e-6, 1e-5), 32: (3e-5, 1e-5)}


@pytest.mark.parametrize("dtype,npix,C,ldy,r", BN_STATS)
def test_bn_stats_contract(dtype, npix, C, ldy, r):
    fin, errs = run_bn_stats(dtype, npix, C, ldy, r)
    gm = (npix + _L().lib().ydl_bn_stats_block_m() - 1) // _L().lib().ydl_bn_stats_block_m()
    assert fin == ("bn_finalize<two-level>" if gm > 1024 else "bn_finalize<one-level>"), (npix, fin)
    if npix > 1:
        mean_tol, var_tol = BN_STATS_TOLS[r]
        assert errs["S"] < mean_tol and errs["mean"] < mean_tol and errs["rm"] < mean_tol, (dtype, npix, C, r, errs)
        for key in ("Q", "var", "invstd", "scale", "rv"):
            assert errs[key] < var_tol, (dtype, npix, C, r, key, errs)


def run_bn_act_bwd(dtype, npix, C):
    """ydl_bn_act_bwd (no activation, no residual) on its workspace of ydl_bn_bwd_ws_bytes; returns (partials, errors of dgamma /
    dbeta against float64 sums of dz = dout and dz * xhat, xhat from the stored y and the saved mean / invstd)"""
    L = _L()
    lib = L.lib()
    dt, tdt, V = (L.YDL_BF16, torch.bfloat16, 8) if dtype == "bf16" else (L.YDL_F32, torch.float32, 4)
    cp = (C + V - 1) // V * V
    cp = (cp + 7) // 8 * 8
    rs = np.random.RandomState(npix + 3 * C)
    y = torch.zeros(npix, cp)
    y[:, :C] = torch.from_numpy((rs.standard_normal((npix, C)) * 1.5 + 0.5).astype(np.float32))
    dout = torch.zeros(npix, cp)
    dout[:, :C] = torch.from_numpy((rs.standard_normal((npix, C)) + 0.1).astype(np.float32))
    y, dout = y.to(tdt), dout.to(tdt)
    yd = y[:, :C].double()
    mean = torch.zeros(cp)
    invstd = torch.zeros(cp)
    mean[:C] = yd.mean(0).float()
    invstd[:C] = (1.0 / torch.sqrt(yd.var(0, unbiased=False) + EPS)).float()
    gamma = torch.zeros(cp)
    gamma[:C] = torch.from_numpy(rs.uniform(0.5, 1.5, C).astype(np.float32))
    scale = gamma * invstd
    shift = torch.zeros(cp)
    shift[:C] = torch.from_numpy(rs.uniform(-0.3, 0.3, C).astype(np.float32))
    nblk = min(max((npix + 256 // (cp // V) - 1) // (256 // (cp // V)), 1), 1024) if cp // V <= 256 else min(max(npix, 1), 1024)
    wsi, ws, q = _guarded_ws(lib.ydl_bn_bwd_ws_bytes(npix, cp))
    dev = torch.device("cuda")
    g = {k: v.to(dev) for k, v in dict(y=y, dout=dout, mean=mean, invstd=invstd, gamma=gamma, scale=scale, shift=shift).items()}
    dy = torch.zeros(npix, cp, dtype=tdt, device=dev)
    dgamma = torch.zeros(cp, device=dev)
    dbeta = torch.zeros(cp, device=dev)
    L.call("ydl_bn_act_bwd", dt, _P(g["y"]), cp, _P(g["dout"]), cp, None, 0, _P(g["gamma"]), _P(g["mean"]), _P(g["invstd"]),
           _P(g["scale"]), _P(g["shift"]), L.RES_NONE, L.ACT_NONE, _P(dy), cp, None, 0, _P(dgamma), _P(dbeta), 0, _P(ws), npix, C, cp,
           _stream())
    torch.cuda.synchronize()
    assert _intact(wsi, q), "written beyond ydl_bn_bwd_ws_bytes"
    dz = dout[:, :C].double().to(dev)
    xhat = (y[:, :C].double().to(dev) - mean[:C].double().to(dev)) * invstd[:C].double().to(dev)
    rb, rg = dz.sum(0), (dz * xhat).sum(0)
    # in units of the sums' natural scale: sqrt(npix) x rms of the summands
    sb, sg = (dz * dz).sum(0).sqrt(), ((dz * xhat) ** 2).sum(0).sqrt()
    errs = dict(dbeta=float(((dbeta[:C].double() - rb).abs() / sb).max()), dgamma=float(((dgamma[:C].double() - rg).abs() / sg).max()))
    return nblk, errs


# npix giving 1 partial, fewer than BWD_MAX_PARTIALS (1024) and exactly BWD_MAX_PARTIALS (the grid is clamped there)
BN_BWD = [("bf16", 20, 64), ("bf16", 500 * 32 - 7, 64), ("bf16", 1024 * 32 + 999, 64),
          ("f32", 3, 40), ("f32", 300 * 25 + 11, 40), ("f32", 1024 * 25 * 3 + 5, 40)]
BN_BWD_TOL = 1.5e-5                 # in units of sqrt(sum of squared summands); measured 1.4e-6 (f32, 1024 partials)


@pytest.mark.parametrize("dtype,npix,C", BN_BWD)
def test_bn_act_bwd_workspace(dtype, npix, C):
    nblk, errs = run_bn_act_bwd(dtype, npix, C)
    assert errs["dbeta"] < BN_BWD_TOL and errs["dgamma"] < BN_BWD_TOL, (dtype, npix, C, nblk, errs)


def run_wgrad_det(dtype, N, c1, c2, k, s, H, W, knobs=()):
    """ydl_conv_wgrad_det with its slab of ydl_conv_wgrad_ws_bytes; returns (kernel, error of dw against float64 in units of the
    largest |dw|)"""
    L = _L()
    lib = L.lib()
    case = Case(dtype, N, c1, c2, k, s, H, W)
    rs = np.random.RandomState(c1 + c2 + H)
    dev = torch.device("cuda")
    V = 8 if dtype == "bf16" else 4
    ldy = (c2 + 7) // 8 * 8
    dyh = torch.zeros(case.M, ldy)
    dyh[:, :c2] = torch.from_numpy(rs.standard_normal((case.M, c2)).astype(np.float32))
    dyh = dyh.to(case.tdt)
    g = L.ConvGeom(N, H, W, c1, case.Ho, case.Wo, c2, k, s, case.p, case.ldx, ldy, 0)
    gp = ctypes.byref(g)
    assert ldy % V == 0
    for key, val in knobs:
        L.debug_set(key, val)
    try:
        wsi, ws, q = _guarded_ws(lib.ydl_conv_wgrad_ws_bytes(gp, case.dt))
        nw = c2 * k * k * case.cp_in
        dwi = _sentinel(nw + MIB_FLOATS)
        dwi[:nw] = 0
        dw = dwi.view(torch.float32)
        xg, dyg = case.x.reshape(-1).to(dev), dyh.to(dev)
        L.call("ydl_conv_wgrad_det", gp, case.dt, _P(xg), _P(dyg), _P(dw), _P(ws), _stream())
        torch.cuda.synchronize()
        kern = L.last_kernel(2)
    finally:
        for key, _ in knobs:
            L.debug_set(key, {0: 1, 4: 1}.get(key, -1))
    assert _intact(wsi, q), (kern, "written beyond ydl_conv_wgrad_ws_bytes")
    assert _intact(dwi, nw), (kern, "written beyond dw")
    xd = case.x.to(dev).double()[..., :case.cp_in].permute(0, 3, 1, 2)
    dyd = dyh.to(dev).double()[:, :c2]
    ref = torch.zeros(c2, case.cp_in * k * k, dtype=torch.float64, device=dev)
    L0 = case.Ho * case.Wo
    for n in range(N):
        cols = F.unfold(xd[n:n + 1], k, padding=case.p, stride=s)[0]
        ref += dyd[n * L0:(n + 1) * L0].t() @ cols.t()
    ref = ref.view(c2, case.cp_in, k * k).permute(0, 2, 1).reshape(c2, -1)
    got = dw[:nw].view(c2, -1).double()
    return kern, float((got - ref).abs().max() / ref.abs().max())


# one geometry per weight-gradient kernel family of the deterministic path: (tag, dtype, N, c1, c2, k, s, H, W, knobs, kernel)
WGRAD = [
    ("wgrad_f32", "f32", 2, 64, 96, 3, 1, 48, 48, (), "wgrad_kernel<f32>"),
    ("wgrad_f32_s2_1x1", "f32", 2, 40, 24, 1, 2, 37, 29, (), "wgrad_kernel<f32>"),
    ("wgrad_bf16_tr", "bf16", 2, 16, 64, 3, 1, 48, 64, (), "wgrad_kernel<bf16,tr>"),
    ("wgrad_bf16_scalar", "bf16", 2, 16, 64, 3, 1, 48, 64, ((0, 0),), "wgrad_kernel<bf16,scalar>"),
    ("wgrad3s_64", "bf16", 4, 64, 64, 3, 1, 96, 96, (), "wgrad3s_kernel<64>"),
    ("wgrad3s_128", "bf16", 4, 64, 128, 3, 1, 96, 96, (), "wgrad3s_kernel<128>"),
    ("wgrad3_128", "bf16", 4, 64, 128, 3, 1, 96, 96, ((18, 0),), "wgrad3_kernel<128>"),
    ("wgrad2_128", "bf16", 4, 64, 128, 3, 1, 96, 96, ((4, 0),), "wgrad2_kernel<128>"),
]
WGRAD_TOL = {"f32": 5e-6, "bf16": 5e-6}     # of max |dw|; measured 4.0e-7 / 4.9e-7


@pytest.mark.parametrize("case", WGRAD, ids=[c[0] for c in WGRAD])
def test_wgrad_det_workspace(case):
    tag, dtype, N, c1, c2, k, s, H, W, knobs, expk = case
    kern, err = run_wgrad_det(dtype, N, c1, c2, k, s, H, W, knobs)
    assert kern == expk, (tag, kern)
    assert err < WGRAD_TOL[dtype], (tag, err)


# guard only (values pinned by the deformable / DCNv3 / loss tests): one large and one ragged shape each
@pytest.mark.parametrize("dtype,N,H,W,C,ld,k", [("bf16", 4, 64, 64, 64, 64, 3), ("f32", 3, 37, 53, 20, 20, 3),
                                                 ("bf16", 2, 29, 31, 20, 24, 5), ("f32", 1, 3, 5, 12, 12, 7)])
def test_dwconv_wgrad_workspace(dtype, N, H, W, C, ld, k):
    L = _L()
    dt, tdt = (L.YDL_BF16, torch.bfloat16) if dtype == "bf16" else (L.YDL_F32, torch.float32)
    dev = torch.device("cuda")
    x = torch.randn(N * H * W, ld, device=dev).to(tdt)
    dy = torch.randn(N * H * W, ld, device=dev).to(tdt)
    wsi, ws, q = _guarded_ws(L.lib().ydl_dwconv_wgrad_ws_bytes(C, k))
    ndw = C * k * k
    dwi = _sentinel(ndw + MIB_FLOATS)
    dwi[:ndw] = 0
    L.call("ydl_dwconv_wgrad", dt, _P(x), ld, _P(dy), ld, _P(dwi), _P(ws), N, H, W, C, k, k // 2, _stream())
    torch.cuda.synchronize()
    assert _intact(wsi, q) and _intact(dwi, ndw)
    assert bool(torch.isfinite(dwi[:ndw].view(torch.float32)).all())


@pytest.mark.parametrize("dtype,npix,C,ld", [("bf16", 1 << 20, 128, 128), ("f32", 12345, 20, 24), ("f32", 777, 21, 21),
                                            ("bf16", 5, 3, 8)])
def test_channel_sum_workspace(dtype, npix, C, ld):
    L = _L()
    dt, tdt = (L.YDL_BF16, torch.bfloat16) if dtype == "bf16" else (L.YDL_F32, torch.float32)
    x = torch.randn(npix, ld, device="cuda").to(tdt)
    wsi, ws, q = _guarded_ws(L.lib().ydl_channel_sum_ws_bytes(C))
    outi = _sentinel(C + MIB_FLOATS)
    L.call("ydl_channel_sum", dt, _P(x), ld, _P(outi), _P(ws), npix, C, 0, _stream())
    torch.cuda.synchronize()
    assert _intact(wsi, q) and _intact(outi, C)
    ref = x[:, :C].double().sum(0)
    assert float((outi[:C].view(torch.float32).double() - ref).abs().max()) < 1e-3 * float(x[:, :C].double().abs().sum(0).max())


@pytest.mark.parametrize("N,C,H,W", [(4, 12, 320, 320), (3, 20, 37, 53), (1, 1, 1, 3)])
def test_seg_loss_workspace(N, C, H, W):
    L = _L()
    dev = torch.device("cuda")
    pred = torch.softmax(torch.randn(N, C, H, W, device=dev), 1).contiguous()
    target = torch.randint(0, C, (N, H, W), device=dev, dtype=torch.int64)
    nf = L.lib().ydl_seg_loss_ws_floats(N, C)
    wsi, ws, q = _guarded_ws(nf * 4)
    lossi = _sentinel(3 + MIB_FLOATS)
    losses = lossi.view(torch.float32)
    dpred = torch.zeros_like(pred)
    st = (C * H * W, H * W, W, 1)
    L.call("ydl_seg_loss_fwd", _P(pred), *st, _P(target), H, W, None, L.LOSS_DICE, 0.0, 1.0, N, C, H, W, _P(ws), _P(losses), _stream())
    L.call("ydl_seg_loss_bwd", _P(pred), *st, _P(target), H, W, None, L.LOSS_DICE, 0.0, 1.0, N, C, H, W, _P(ws), None, _P(dpred), _stream())
    torch.cuda.synchronize()
    assert _intact(wsi, q) and _intact(lossi, 3)
    assert bool(torch.isfinite(losses[:3]).all()) and bool(torch.isfinite(dpred).all())
