"""Launch census: the convolution and BatchNorm launches of one real training step, each distinct one checked on its own.

``record_step`` builds a workload of bench.py the way bench.py does (bf16 throughput mode, default switches, the workload's own batch
and size), runs two eager warm-up steps and records every C-ABI call of one forward + loss + backward through ``_lib.set_recorder``:
entry point, arguments by value (the ydl_conv_geom copied at call time), NULL-ness of the optional pointers, and the kernel
instantiation ``ydl_debug_last_kernel`` reports for it.  Calls are reduced to distinct cases (pointer values are not part of the key).

``check_case`` replays one distinct case through the C ABI on fresh operands with exactly the recorded strides and compares every
element with a float64 reference that shares nothing with the kernels: im2col (F.unfold / F.fold) + float64 matmul per image for the
convolutions, a float64 restatement for the BatchNorm launches.  The same routine on the squares and on the absolute values of the
operands gives per element Q = sqrt(sum (a_i b_i)^2) and A = sum |a_i b_i|, from which the bounds are DERIVED (nothing is measured):

* f32 accumulation of K terms: e_acc = 4 sqrt(K) 2^-24 Q (sequential f32 summation of zero-mean terms has an rms error of
  sqrt(K) 2^-24 Q / sqrt(6); blocked MFMA accumulation and atomic split-K only do better; 4 is about ten standard deviations), and in
  any case the rigorous worst case (K + 1) 2^-24 A: the smaller of the two is the bound;
* a value stored in bf16: one round-to-nearest of the f32 result, 2^-8 |ref| (1 + 2^-6) + e_acc; a value stored in f32: e_acc.
  (bf16 keeps 8 significant bits: half a unit in the last place is up to 2^-8 of the value.  The issue this census answers wrote 2^-9
  for this term, under which a correctly rounded copy of the float64 reference fails — its own acceptance test; the unit roundoff of
  the format is what "one round-to-nearest" derives.  A deviation of 2^-7 |ref| is still caught.);
* a second rounding where the kernel source has one: pw_kernel's LDS-transposed accumulate store (",ts" with accumulate) and the
  accumulating one-pass point-wise backward (pwbw_kernel<.., acc>) round the launch's own contribution to bf16 before the add,
  2^-8 |own contribution| more.

The reference routines and the comparison run on any device: tests/test_census_reference_cpu.py holds them to torch's own float64
convolution gradients and to autograd without a GPU."""
from __future__ import annotations

import collections
import ctypes
import math
import os
import sys
import zlib

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U24, U8 = 2.0 ** -24, 2.0 ** -8          # unit roundoffs of f32 and bf16 (round to nearest)
BF16_STORE = U8 * (1.0 + 2.0 ** -6)
CANARY = 7.0
SENT = 0x7FA5A5A5                   # a NaN bit pattern no kernel produces (tests/test_gpu_bn_statistics.py)
TAIL = 1 << 16                      # guard elements behind every output buffer
BN_BWD_TOL = 1.5e-5                 # dgamma / dbeta, in units of sqrt(sum of squared summands) (tests/test_gpu_bn_statistics.py)
ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2
RES_NONE, RES_AFTER_ACT, RES_BEFORE_ACT, RES_GRAD_ACCUMULATE = 0, 1, 2, 16

Geom = collections.namedtuple("Geom", "N Hi Wi Cin Ho Wo Cout k s p ldx ldy ldw")

CONV_ENTRIES = ("ydl_conv_fwd", "ydl_conv_fwd_sums", "ydl_conv_dgrad", "ydl_conv_dgrad_bnred", "ydl_conv_wgrad", "ydl_conv_wgrad_det",
                "ydl_conv_bwd_pw")
BN_ENTRIES = ("ydl_bn_act_fwd_sums", "ydl_bn_act_bwd_sums", "ydl_bn_act_bwd_apply_sums", "ydl_bn_act_fwd", "ydl_bn_act_bwd",
              "ydl_bn_finalize")
# which ydl_debug_last_kernel families an entry point sets
KERNEL_FAMILIES = {"ydl_conv_fwd": (0,), "ydl_conv_fwd_sums": (0,), "ydl_conv_dgrad": (1,), "ydl_conv_dgrad_bnred": (1,),
                   "ydl_conv_wgrad": (2,), "ydl_conv_wgrad_det": (2,), "ydl_conv_bwd_pw": (1, 2), "ydl_bn_finalize": (3,)}


class CensusFailure(AssertionError):
    pass


def r8(c: int) -> int:
    return (c + 7) // 8 * 8


# =====================================================================================================================
# float64 references (any device)
# =====================================================================================================================
def _nchw(buf: torch.Tensor, N: int, H: int, W: int, ld: int, Cp: int) -> torch.Tensor:
    """rows of ``ld`` elements, NHWC -> float64 [N, Cp, H, W] of the first Cp channels"""
    return buf.reshape(-1)[:N * H * W * ld].view(N, H, W, ld)[..., :Cp].double().permute(0, 3, 1, 2)


def _triple(fn, a, b, prior=None):
    """(own, ref, Q, A) of one bilinear routine: own = fn(a, b), ref = own + prior, Q = sqrt(fn(a^2, b^2) + prior^2),
    A = fn(|a|, |b|) + |prior|"""
    own = fn(a, b)
    q2 = fn(a * a, b * b)
    ab = fn(a.abs(), b.abs())
    ref = own
    if prior is not None:
        prior = prior.double()
        ref, q2, ab = own + prior, q2 + prior * prior, ab + prior.abs()
    return own, ref, q2.clamp_min(0).sqrt(), ab


def conv_fwd_ref(g: Geom, xbuf, wbuf, col0: int = 0, prior=None):
    """y = conv(x, w) [+ prior] as im2col + matmul per image.  xbuf: rows of g.ldx; wbuf: [Cout] rows of (g.ldw or k*k*Cin_p) elements,
    the launch's block starting at column col0, laid out [k*k][Cin_p].  -> (own, ref, Q, A), each [N*Ho*Wo, Cout] float64"""
    kk, cp = g.k * g.k, r8(g.Cin)
    xn = _nchw(xbuf, g.N, g.Hi, g.Wi, g.ldx, cp)
    ldw = g.ldw or kk * cp
    w = wbuf.reshape(-1)[:g.Cout * ldw].view(g.Cout, ldw)[:, col0:col0 + kk * cp].double().reshape(g.Cout, kk, cp)
    wm = w.permute(0, 2, 1).reshape(g.Cout, cp * kk)             # unfold orders its rows (channel, tap)

    def fn(x, m):
        return torch.cat([(m @ F.unfold(x[n:n + 1], g.k, padding=g.p, stride=g.s)[0]).t() for n in range(g.N)])
    return _triple(fn, xn, wm, prior)


def conv_dgrad_ref(g: Geom, dybuf, wtbuf, prior=None):
    """dx = conv_transpose(dy, wt) [+ prior] as matmul + col2im per image.  dybuf: rows of g.ldy; wtbuf: [Cin][k*k][Cout_p] dense.
    -> (own, ref, Q, A), each [N*Hi*Wi, Cin] float64"""
    kk, cop = g.k * g.k, r8(g.Cout)
    L = g.Ho * g.Wo
    dyn = dybuf.reshape(-1)[:g.N * L * g.ldy].view(g.N, L, g.ldy)[..., :cop].double()
    wt = wtbuf.reshape(-1)[:g.Cin * kk * cop].view(g.Cin * kk, cop).double()          # rows already ordered (channel, tap)

    def fn(d, m):
        out = []
        for n in range(g.N):
            cols = m @ d[n].t()
            img = F.fold(cols[None], (g.Hi, g.Wi), g.k, padding=g.p, stride=g.s)[0]
            out.append(img.permute(1, 2, 0).reshape(g.Hi * g.Wi, g.Cin))
        return torch.cat(out)
    return _triple(fn, dyn, wt, prior)


def conv_wgrad_ref(g: Geom, xbuf, dybuf, prior=None):
    """dw[Cout][k*k][Cin_p] = sum over pixels dy^T im2col(x) [+ prior] -> (own, ref, Q, A), each [Cout, k*k*Cin_p] float64"""
    kk, cp = g.k * g.k, r8(g.Cin)
    L = g.Ho * g.Wo
    xn = _nchw(xbuf, g.N, g.Hi, g.Wi, g.ldx, cp)
    dyn = dybuf.reshape(-1)[:g.N * L * g.ldy].view(g.N, L, g.ldy)[..., :g.Cout].double()

    def fn(x, d):
        acc = torch.zeros(g.Cout, cp * kk, dtype=torch.float64, device=x.device)
        for n in range(g.N):
            acc += d[n].t() @ F.unfold(x[n:n + 1], g.k, padding=g.p, stride=g.s)[0].t()
        return acc.view(g.Cout, cp, kk).permute(0, 2, 1).reshape(g.Cout, kk * cp)
    return _triple(fn, xn, dyn, prior)


def dgrad_terms(g: Geom, device) -> torch.Tensor:
    """summands of one input-gradient element, per pixel of one image [Hi*Wi]: (taps of the pixel's stride-parity class) x Cout"""
    def taps(n, par_len):
        idx = torch.arange(n, device=device)
        cnt = torch.zeros(n, dtype=torch.float64, device=device)
        for r in range(g.k):
            cnt += ((idx + g.p - r) % g.s == 0).double()
        return cnt
    th, tw = taps(g.Hi, g.s), taps(g.Wi, g.s)
    return (th[:, None] * tw[None, :]).reshape(-1) * g.Cout


def acc_bound(K, Q, A):
    """f32 accumulation of K terms: min(4 sqrt(K) 2^-24 Q, (K + 1) 2^-24 A); K a number or a tensor broadcastable to Q"""
    K = K if torch.is_tensor(K) else torch.tensor(float(K), dtype=torch.float64, device=Q.device)
    return torch.minimum(4.0 * K.sqrt() * U24 * Q, (K + 1.0) * U24 * A)


def stored_bound(ref, e_acc, bf16: bool, extra=None):
    tol = e_acc + (BF16_STORE * ref.abs() if bf16 else 0.0)
    return tol if extra is None else tol + extra


def worst(got, ref, tol):
    """(largest |got - ref| / tol, number of elements over their bound, flat index of the worst).  An element with a zero bound
    must be exact; a non-finite value is over any bound."""
    got, ref = got.double(), ref.double()
    diff = (got - ref).abs()
    diff = torch.where(torch.isfinite(got), diff, torch.full_like(diff, float("inf")))
    ratio = torch.where(tol > 0, diff / tol.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))
    if ratio.numel() == 0:
        return 0.0, 0, -1
    i = int(ratio.reshape(-1).argmax())
    return float(ratio.reshape(-1)[i]), int((ratio > 1.0).sum()), i


def act_f64(z, act: int):
    if act == ACT_SILU:
        return z * torch.sigmoid(z)
    if act == ACT_RELU:
        return z.clamp_min(0)
    return z


def bn_coeffs_ref(rows1, rows2, count, gamma, beta, eps, momentum, rm0, rv0, replication):
    """coefficients from replica rows AS GIVEN (summed in float64): rows1 / rows2 [replicas, C] hold sum and sum of squares"""
    s1, s2 = rows1.double().sum(0), rows2.double().sum(0)
    n = float(count)
    mean = s1 / n
    m2 = (s2 - s1 * mean).clamp_min(0)
    var = m2 / n
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    nl = n * replication
    unb = m2 * replication / (nl - 1.0) if nl > 1.0 else var
    out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, s2=s2, unb=unb)
    if rm0 is not None:
        out["rm"] = (1.0 - momentum) * rm0.double() + momentum * mean
        out["rv"] = (1.0 - momentum) * rv0.double() + momentum * unb
    return out


def bn_apply_ref(y, scale, shift, act: int, res_mode: int, res=None):
    """out = act(y*scale + shift [+ res]) [+ res] per YDL_RES_*; y [npix, C] float64"""
    z = y * scale + shift
    if res_mode == RES_BEFORE_ACT:
        z = z + res
    o = act_f64(z, act)
    if res_mode == RES_AFTER_ACT:
        o = o + res
    return o


def bn_bwd_ref(y, dout, mean, invstd, scale, shift, act: int, res_mode: int, out=None, res=None, sums=None, dres_prior=None):
    """float64 restatement of the BatchNorm + activation backward: dz = dout * act'(z), xhat = (y - mean) * invstd,
    dbeta = sum dz, dgamma = sum dz * xhat, dy = scale * (dz - dbeta / n - xhat * dgamma / n); dres = dout (joined after the activation)
    or dz (joined before it), plus ``dres_prior`` with YDL_RES_GRAD_ACCUMULATE.  ``res`` enters z when the residual is joined before
    the activation; without it (the kernels' backward has no such operand) ReLU takes its mask from the saved output ``out``.  ``sums`` = (sum dz, sum dz*xhat) given from outside
    (the apply pass alone).  -> dict(dz, xhat, dbeta, dgamma, dy, dres, sq_b, sq_g)"""
    rmode = res_mode & 15
    n = float(y.shape[0])
    z = y * scale + shift
    if rmode == RES_BEFORE_ACT and res is not None:
        z = z + res
    if act == ACT_SILU:
        sg = torch.sigmoid(z)
        dz = dout * (sg * (1.0 + z * (1.0 - sg)))
    elif act == ACT_RELU:
        # the kernels take the mask from the saved output, which is the activation's own output unless a residual was added behind it
        live = (out > 0) if (rmode == RES_BEFORE_ACT and res is None) else (z > 0)
        dz = torch.where(live, dout, torch.zeros_like(dout))
    else:
        dz = dout
    xhat = (y - mean) * invstd
    db, dg = dz.sum(0), (dz * xhat).sum(0)
    r = dict(dz=dz, xhat=xhat, z=z, dbeta=db, dgamma=dg, sq_b=(dz * dz).sum(0).sqrt(), sq_g=((dz * xhat) ** 2).sum(0).sqrt())
    if sums is not None:
        db, dg = sums
    r["dy"] = scale * (dz - db / n - xhat * dg / n)
    r["kb"], r["kg"] = db / n, dg / n
    dres = None
    if rmode == RES_AFTER_ACT:
        dres = dout
    elif rmode == RES_BEFORE_ACT:
        dres = dz
    if dres is not None and dres_prior is not None:
        dres = dres + dres_prior
    r["dres"] = dres
    return r


# =====================================================================================================================
# recording
# =====================================================================================================================
def _pv(a) -> int:
    if a is None:
        return 0
    if isinstance(a, ctypes.c_void_p):
        return a.value or 0
    return int(a)


def _geom_of(arg) -> Geom:
    src = arg._obj if hasattr(arg, "_obj") else arg
    return Geom(*[int(getattr(src, f)) for f in Geom._fields])


def _case_of(name: str, a) -> dict:
    """the recorded call by value: every integer argument, NULL-ness of the optional pointers, which pointers coincide"""
    if name in ("ydl_conv_fwd", "ydl_conv_fwd_sums"):
        return dict(entry=name, g=_geom_of(a[0]), dt=int(a[1]), stats=bool(_pv(a[5])), acc=int(a[6]))
    if name == "ydl_conv_dgrad":
        return dict(entry=name, g=_geom_of(a[0]), dt=int(a[1]), acc=int(a[5]))
    if name in ("ydl_conv_wgrad", "ydl_conv_wgrad_det"):
        return dict(entry=name, g=_geom_of(a[0]), dt=int(a[1]))
    if name == "ydl_conv_bwd_pw":
        return dict(entry=name, g=_geom_of(a[0]), dt=int(a[1]), lddx=int(a[6]), acc=int(a[7]))
    if name == "ydl_bn_act_fwd_sums":
        return dict(entry=name, dt=int(a[0]), ldy=int(a[2]), sums_ld=int(a[4]), count=int(a[5]), gamma=bool(_pv(a[6])), beta=bool(_pv(a[7])),
                    eps=float(a[8]), momentum=float(a[9]), running=bool(_pv(a[10])), replication=int(a[16]), res=bool(_pv(a[17])),
                    ldr=int(a[18]), res_mode=int(a[19]), act=int(a[20]), ldo=int(a[22]), npix=int(a[23]), C=int(a[24]), Cp=int(a[25]),
                    alias=(_pv(a[21]) == _pv(a[1]), bool(_pv(a[17])) and _pv(a[21]) == _pv(a[17])))
    if name in ("ydl_bn_act_bwd_sums", "ydl_bn_act_bwd_apply_sums", "ydl_bn_act_bwd"):
        o = 1 if name == "ydl_bn_act_bwd" else 0        # ydl_bn_act_bwd has gamma in front of mean
        y, dout, dy, dres = _pv(a[1]), _pv(a[3]), _pv(a[13 + o]), _pv(a[15 + o])
        return dict(entry=name, dt=int(a[0]), ldy=int(a[2]), lddo=int(a[4]), out=bool(_pv(a[5])), ldo=int(a[6]), res_mode=int(a[11 + o]),
                    act=int(a[12 + o]), lddy=int(a[14 + o]), dres=bool(dres), lddr=int(a[16 + o]), dgamma=bool(_pv(a[17 + o])),
                    dbeta=bool(_pv(a[18 + o])), accp=int(a[19 + o]), npix=int(a[21 + o]), C=int(a[22 + o]), Cp=int(a[23 + o]),
                    alias=(dy == dout, dy == y, bool(dres) and dres == dout, bool(dres) and dres == dy))
    if name == "ydl_bn_act_fwd":
        return dict(entry=name, dt=int(a[0]), ldy=int(a[2]), res=bool(_pv(a[5])), ldr=int(a[6]), res_mode=int(a[7]), act=int(a[8]),
                    ldo=int(a[10]), npix=int(a[11]), Cp=int(a[12]),
                    alias=(_pv(a[9]) == _pv(a[1]), bool(_pv(a[5])) and _pv(a[9]) == _pv(a[5])))
    # an entry point of the two families without a checker (ydl_conv_dgrad_bnred, ydl_bn_finalize): kept, and reported as a failure
    return dict(entry=name, unknown=True)


def case_key(case: dict):
    return tuple(sorted(case.items()))


class Census:
    """recorder object for ``_lib.set_recorder``: ``add`` sees every C-ABI call before it runs, so the kernel name of a call is read
    when the NEXT call arrives (or at ``flush``)"""

    def __init__(self):
        self.cases = collections.OrderedDict()       # key -> dict(case=, count=, kernels=set())
        self.total = collections.Counter()           # "conv" / "bn" launches seen
        self._pending = None

    def _settle(self):
        if self._pending is not None:
            from yolo_dual_amd import _lib as L
            slot, fams = self._pending
            slot["kernels"].add("|".join(L.last_kernel(f) for f in fams))
            self._pending = None

    def add(self, name, args):
        self._settle()
        if name not in CONV_ENTRIES and name not in BN_ENTRIES:
            return
        self.total["conv" if name in CONV_ENTRIES else "bn"] += 1
        case = _case_of(name, args)
        slot = self.cases.setdefault(case_key(case), dict(case=case, count=0, kernels=set()))
        slot["count"] += 1
        self._pending = (slot, KERNEL_FAMILIES.get(name, ()))

    def edge(self, src, dst):             # cross-stream edges are of no interest here
        pass

    def flush(self):
        self._settle()


def record_step(workload: str) -> Census:
    """the model, loss and optimizer of bench.py's workload, two eager warm-up steps, then one recorded forward + loss + backward"""
    import bench
    import yolo_dual_amd as ydl
    from yolo_dual_amd import _lib as L
    wl = bench.WORKLOADS[workload]
    bs, size = wl["bs"], wl["size"]
    dev = torch.device("cuda", torch.cuda.current_device())
    ydl.set_compute_dtype("bf16")
    torch.manual_seed(0)
    if wl["model"] == "ResNet50Seg":
        model = ydl.ResNet50Seg({"nc": 12}).to(dev).train()
        out_hw = 640
    else:
        model = getattr(ydl, wl["model"])(bench.load_cfg(wl["yaml"], wl["swap"])).to(dev).train()
        out_hw = 640 if size == 1024 else size
        model.img_size = [out_hw, out_hw]
    cw = torch.tensor(bench.CW, dtype=torch.float32) if wl["cw"] else None
    crit = ydl.SegmentationLoss(12, 0.0, cw, wl["loss"], sync=False)
    opt = ydl.FlatSGDEMA(model, lr=0.01, momentum=0.937, weight_decay=5e-4 * bs / 64.0)
    g = torch.Generator(device=dev).manual_seed(1234)
    imgs = torch.rand(bs, 3, size, size, device=dev, generator=g)
    tgts = torch.randint(0, 12, (bs, out_hw, out_hw), device=dev, generator=g)

    def fwd_bwd():
        opt.zero_grad()
        out = model(imgs)
        loss, _items = crit(out, tgts)
        loss.backward()

    for _ in range(2):
        fwd_bwd()
        opt.step(grad_scale=1.0)
    torch.cuda.synchronize()
    cen = Census()
    L.set_recorder(cen)
    try:
        fwd_bwd()
        cen.flush()
    finally:
        L.set_recorder(None)
    opt.step(grad_scale=1.0)
    torch.cuda.synchronize()
    del model, crit, opt, imgs, tgts
    torch.cuda.empty_cache()
    return cen


# =====================================================================================================================
# one distinct launch through the C ABI
# =====================================================================================================================
def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tdt(dt):
    return torch.bfloat16 if dt == 1 else torch.float32


class Rows:
    """an NHWC operand of ``npix`` rows at stride ``ld``: columns [0, C) random (or the canary when ``fill`` is False: an output every
    element of which must be written), [C, round_up(C, 8)) zero as the model keeps them, the rest the canary; a sentinel guard behind
    the last row"""

    def __init__(self, npix, ld, C, tdt, gen, scale=1.0, fill=True, offset=0.0):
        dev = gen.device
        self.npix, self.ld, self.C, self.tdt = npix, ld, C, tdt
        self.n = npix * ld
        self.flat = torch.full((self.n + TAIL,), CANARY, dtype=tdt, device=dev)
        self.v = self.flat[:self.n].view(npix, ld)
        if fill:
            self.v[:, :C] = (torch.randn(npix, C, device=dev, generator=gen) * scale + offset).to(tdt)
        self.v[:, C:r8(C)] = 0
        self._guard().fill_(0x7FA5 if tdt == torch.bfloat16 else SENT)

    def _guard(self):
        return self.flat[self.n:].view(torch.int16 if self.tdt == torch.bfloat16 else torch.int32)

    def logical(self):
        return self.v[:, :self.C].double()

    def check_guards(self, what):
        if not bool((self._guard() == (0x7FA5 if self.tdt == torch.bfloat16 else SENT)).all()):
            raise CensusFailure(f"{what}: written behind the last row")
        if self.ld > r8(self.C) and not bool((self.v[:, r8(self.C):].float() == CANARY).all()):
            raise CensusFailure(f"{what}: written outside [0, round_up(C, 8)) of a row")


class Floats:
    """an f32 output vector of n elements (``init``: a tensor, or None for zeros) with a sentinel guard behind it"""

    def __init__(self, n, dev, init=None):
        self.n = n
        self.raw = torch.full((n + TAIL,), SENT, dtype=torch.int32, device=dev)
        self.v = self.raw.view(torch.float32)[:n]
        if init is None:
            self.v.zero_()
        else:
            self.v.copy_(init)

    def check_guards(self, what):
        if not bool((self.raw[self.n:] == SENT).all()):
            raise CensusFailure(f"{what}: written behind its end")


def _seed(case) -> int:
    return zlib.crc32(repr(case_key(case)).encode())


def _weights(L, g: Geom, dt, tdt, gen, for_dgrad=False):
    """master (f32, representable in the compute dtype) -> w / wt through ydl_weight_prep; the compute copies are checked against the
    master here so that the references can be built from the master alone"""
    dev = gen.device
    kk, cip, cop = g.k * g.k, r8(g.Cin), r8(g.Cout)
    fan = kk * (g.Cout if for_dgrad else g.Cin)
    master = (torch.randn(g.Cout, kk, g.Cin, device=dev, generator=gen) / math.sqrt(fan)).to(tdt).float().contiguous()
    w = torch.full((g.Cout, kk, cip), CANARY, dtype=tdt, device=dev)
    wt = torch.full((g.Cin, kk, cop), CANARY, dtype=tdt, device=dev)
    L.call("ydl_weight_prep", dt, _P(master), _P(w), _P(wt), g.Cout, kk, g.Cin, _stream())
    wr = torch.zeros(g.Cout, kk, cip, device=dev)
    wr[..., :g.Cin] = master
    wtr = torch.zeros(g.Cin, kk, cop, device=dev)
    wtr[..., :g.Cout] = master.permute(2, 1, 0)
    if not (torch.equal(w.float(), wr) and torch.equal(wt.float(), wtr)):
        raise CensusFailure("ydl_weight_prep: compute copies differ from the master weight")
    return wr.to(tdt), wtr.to(tdt), w, wt


def _col0(ldw, width):
    """first column of the launch's block inside a wider weight matrix (a multiple of 8: 16-byte aligned in every dtype)"""
    return (ldw - width) // 16 * 8


def _result(kernel, ratio, over, detail=""):
    return dict(kernel=kernel, ratio=ratio, over=over, detail=detail)


def _merge(parts):
    """[(what, (ratio, over, index))] -> (largest ratio, total over, description of the failing parts)"""
    ratio = max(p[1][0] for p in parts)
    over = sum(p[1][1] for p in parts)
    bad = "; ".join(f"{w}: {r[1]} elements over, worst {r[0]:.3g} x bound at flat index {r[2]}" for w, r in parts if r[1])
    return ratio, over, bad


def check_conv_fwd(L, case, gen):
    g, dt, tdt = case["g"], case["dt"], _tdt(case["dt"])
    bf16 = dt == 1
    dev = gen.device
    kk, cip, cop = g.k * g.k, r8(g.Cin), r8(g.Cout)
    M = g.N * g.Ho * g.Wo
    x = Rows(g.N * g.Hi * g.Wi, g.ldx, g.Cin, tdt, gen)
    wr, _wtr, w, _wt = _weights(L, g, dt, tdt, gen)
    col0 = 0
    if g.ldw:
        if g.k != 1:
            raise CensusFailure("ldw != 0 with k != 1: a column block exists for 1x1 weight matrices only")
        col0 = _col0(g.ldw, cip)
        wide = torch.full((g.Cout, g.ldw), CANARY, dtype=tdt, device=dev)
        wide[:, col0:col0 + cip] = w.view(g.Cout, cip)
        wbuf, wptr = wide, ctypes.c_void_p(wide.data_ptr() + col0 * wide.element_size())
    else:
        wbuf, wptr = w, _P(w)
    y = Rows(M, g.ldy, g.Cout, tdt, gen, fill=bool(case["acc"]))
    prior = y.logical() if case["acc"] else None
    sums = Floats(8 * 2 * cop, dev) if case["stats"] else None
    gs = L.ConvGeom(*g)
    L.call(case["entry"], ctypes.byref(gs), dt, _P(x.flat), wptr, _P(y.flat), _P(sums.raw) if sums else None, case["acc"], _stream())
    torch.cuda.synchronize()
    kernel = L.last_kernel(0)
    own, ref, Q, A = conv_fwd_ref(g, x.flat, wbuf, col0, prior)
    extra = None
    if case["acc"] and kernel.startswith("pw_kernel") and kernel.endswith(",ts>"):
        # pw_kernel's LDS-transposed accumulate store rounds the launch's own contribution to bf16 before the add (csrc/igemm.hip)
        extra = U8 * own.abs()
    tol = stored_bound(ref, acc_bound(kk * g.Cin, Q, A), bf16, extra)
    parts = [("y", worst(y.logical(), ref, tol))]
    y.check_guards(f"{kernel}: y")
    if sums is not None:
        sums.check_guards(f"{kernel}: replica sums")
        rows = sums.v.view(8, 2, cop)[:, :, :g.Cout].double()
        if not bool(torch.isfinite(rows).all()):
            raise CensusFailure(f"{kernel}: non-finite replica row")
        tot = rows.sum(0)
        r1, r2 = ref.sum(0), (ref * ref).sum(0)
        # the project's bounds of test_accumulating_pointwise_forward_with_statistics_through_the_c_abi
        e1 = float(((tot[0] - r1).abs() / r2.sqrt()).max()) / 5e-3
        e2 = float(((tot[1] - r2).abs() / r2).max()) / 2e-3
        parts.append(("replica sum (worst channel error / 5e-3 sqrt(sum of squares))", (e1, int(e1 > 1), 0)))
        parts.append(("replica sum of squares (worst relative error / 2e-3)", (e2, int(e2 > 1), 0)))
    return _result(kernel, *_merge(parts))


def check_conv_dgrad(L, case, gen):
    g, dt, tdt = case["g"], case["dt"], _tdt(case["dt"])
    dy = Rows(g.N * g.Ho * g.Wo, g.ldy, g.Cout, tdt, gen)
    _wr, wtr, _w, wt = _weights(L, g, dt, tdt, gen, for_dgrad=True)
    dx = Rows(g.N * g.Hi * g.Wi, g.ldx, g.Cin, tdt, gen, fill=bool(case["acc"]))
    prior = dx.logical() if case["acc"] else None
    gs = L.ConvGeom(*g)
    L.call("ydl_conv_dgrad", ctypes.byref(gs), dt, _P(dy.flat), _P(wt), _P(dx.flat), case["acc"], _stream())
    torch.cuda.synchronize()
    kernel = L.last_kernel(1)
    own, ref, Q, A = conv_dgrad_ref(g, dy.flat, wtr, prior)
    K = dgrad_terms(g, gen.device).repeat(g.N)[:, None]
    extra = U8 * own.abs() if (case["acc"] and kernel.startswith("pw_kernel") and kernel.endswith(",ts>")) else None
    tol = stored_bound(ref, acc_bound(K, Q, A), dt == 1, extra)
    parts = [("dx", worst(dx.logical(), ref, tol))]
    dx.check_guards(f"{kernel}: dx")
    return _result(kernel, *_merge(parts))


def _dw_buffer(g: Geom, dev):
    """the weight-gradient target: dense [Cout][k*k*Cin_p], or the column block of a wider matrix (ldw), zero inside, canary around"""
    kk, cip = g.k * g.k, r8(g.Cin)
    width = kk * cip
    ldw = g.ldw or width
    col0 = _col0(ldw, width) if g.ldw else 0
    init = torch.full((g.Cout, ldw), CANARY, device=dev)
    init[:, col0:col0 + width] = 0
    buf = Floats(g.Cout * ldw, dev, init.reshape(-1))
    return buf, ldw, col0, width


def _check_dw(buf, ldw, col0, width, g, ref, tol, kernel):
    v = buf.v.view(g.Cout, ldw)
    buf.check_guards(f"{kernel}: dw")
    outside = torch.ones(ldw, dtype=torch.bool, device=v.device)
    outside[col0:col0 + width] = False
    if not bool((v[:, outside] == CANARY).all()):
        raise CensusFailure(f"{kernel}: dw written outside its column block")
    return worst(v[:, col0:col0 + width], ref, tol)


def check_conv_wgrad(L, case, gen):
    g, dt, tdt = case["g"], case["dt"], _tdt(case["dt"])
    dev = gen.device
    x = Rows(g.N * g.Hi * g.Wi, g.ldx, g.Cin, tdt, gen)
    dy = Rows(g.N * g.Ho * g.Wo, g.ldy, g.Cout, tdt, gen)
    buf, ldw, col0, width = _dw_buffer(g, dev)
    gs = L.ConvGeom(*g)
    dwp = ctypes.c_void_p(buf.raw.data_ptr() + 4 * col0)
    ws = None
    if case["entry"] == "ydl_conv_wgrad_det":
        q = L.lib().ydl_conv_wgrad_ws_bytes(ctypes.byref(gs), dt) // 4
        ws = Floats(max(q, 4), dev)
        L.call("ydl_conv_wgrad_det", ctypes.byref(gs), dt, _P(x.flat), _P(dy.flat), dwp, _P(ws.raw), _stream())
    else:
        L.call("ydl_conv_wgrad", ctypes.byref(gs), dt, _P(x.flat), _P(dy.flat), dwp, _stream())
    torch.cuda.synchronize()
    kernel = L.last_kernel(2)
    if ws is not None:
        ws.check_guards(f"{kernel}: workspace")
    _own, ref, Q, A = conv_wgrad_ref(g, x.flat, dy.flat)
    tol = stored_bound(ref, acc_bound(g.N * g.Ho * g.Wo, Q, A), False)
    return _result(kernel, *_merge([("dw", _check_dw(buf, ldw, col0, width, g, ref, tol, kernel))]))


def check_conv_bwd_pw(L, case, gen):
    g, dt, tdt = case["g"], case["dt"], _tdt(case["dt"])
    dev = gen.device
    M = g.N * g.Ho * g.Wo
    x = Rows(M, g.ldx, g.Cin, tdt, gen)
    dy = Rows(M, g.ldy, g.Cout, tdt, gen)
    _wr, wtr, _w, wt = _weights(L, g, dt, tdt, gen, for_dgrad=True)
    dx = Rows(M, case["lddx"], g.Cin, tdt, gen, fill=bool(case["acc"]))
    prior = dx.logical() if case["acc"] else None
    buf, ldw, col0, width = _dw_buffer(g, dev)
    gs = L.ConvGeom(*g)
    dwp = ctypes.c_void_p(buf.raw.data_ptr() + 4 * col0)
    L.call("ydl_conv_bwd_pw", ctypes.byref(gs), dt, _P(x.flat), _P(dy.flat), _P(wt), _P(dx.flat), case["lddx"], case["acc"], dwp, _stream())
    torch.cuda.synchronize()
    kernel = L.last_kernel(1) + "|" + L.last_kernel(2)
    gd = g._replace(ldx=case["lddx"])
    own, ref, Q, A = conv_dgrad_ref(gd, dy.flat, wtr, prior)
    # pwbw_kernel<.., ACC> (csrc/wgrad.hip): compute() packs the launch's own input gradient to bf16 (f2bf) into the LDS staging tile,
    # store_rows() unpacks it, adds the previous dx and packs again — the same second rounding as pw_kernel's transposed accumulate
    # store, 2^-8 |own contribution|
    extra = U8 * own.abs() if case["acc"] else None
    tol = stored_bound(ref, acc_bound(g.Cout, Q, A), dt == 1, extra)
    parts = [("dx", worst(dx.logical(), ref, tol))]
    dx.check_guards(f"{kernel}: dx")
    _own, refw, Qw, Aw = conv_wgrad_ref(g, x.flat, dy.flat)
    tolw = stored_bound(refw, acc_bound(M, Qw, Aw), False)
    parts.append(("dw", _check_dw(buf, ldw, col0, width, g, refw, tolw, kernel)))
    return _result(kernel, *_merge(parts))


def _split_rows(total, gen):
    """a float64 column total split across the eight replica rows and rounded to f32: [8, C]"""
    frac = torch.rand(8, total.shape[0], device=total.device, generator=gen, dtype=torch.float64) + 0.25
    frac = frac / frac.sum(0)
    return (frac * total).float()


def check_bn_act_fwd_sums(L, case, gen):
    dt, tdt, dev = case["dt"], _tdt(case["dt"]), gen.device
    npix, C, Cp = case["npix"], case["C"], case["Cp"]
    out_is_y, out_is_res = case["alias"]
    if out_is_res or case["count"] != npix:
        raise CensusFailure("ydl_bn_act_fwd_sums: an operand pattern the census does not reproduce (out aliases res, or count != npix)")
    if out_is_y and case["ldo"] != case["ldy"]:
        raise CensusFailure("ydl_bn_act_fwd_sums: in-place call with different strides")
    rmode, act = case["res_mode"], case["act"]
    y = Rows(npix, case["ldy"], C, tdt, gen, scale=1.5, offset=0.5)
    yd = y.logical()
    res = Rows(npix, case["ldr"], C, tdt, gen) if case["res"] else None
    rd = res.logical() if res is not None else None
    sld = case["sums_ld"]
    c0 = (sld - Cp) // 8 * 4
    wide = torch.full((16, sld), CANARY, device=dev)
    wide[0::2, c0:c0 + C] = _split_rows(yd.sum(0), gen)
    wide[1::2, c0:c0 + C] = _split_rows((yd * yd).sum(0), gen)
    wide[:, c0 + C:c0 + Cp] = 0
    gamma = (torch.rand(C, device=dev, generator=gen) + 0.5) if case["gamma"] else None
    beta = (torch.rand(C, device=dev, generator=gen) * 0.6 - 0.3) if case["beta"] else None
    rm0 = torch.randn(C, device=dev, generator=gen) * 0.1 if case["running"] else None
    rv0 = torch.rand(C, device=dev, generator=gen) + 0.5 if case["running"] else None
    rm = Floats(C, dev, rm0) if rm0 is not None else None
    rv = Floats(C, dev, rv0) if rv0 is not None else None
    co = {k: Floats(Cp, dev, torch.full((Cp,), CANARY, device=dev)) for k in ("mean", "invstd", "scale", "shift")}
    out = y if out_is_y else Rows(npix, case["ldo"], C, tdt, gen, fill=False)
    L.call("ydl_bn_act_fwd_sums", dt, _P(y.flat), case["ldy"], ctypes.c_void_p(wide.data_ptr() + 4 * c0), sld, case["count"], _P(gamma), _P(beta),
           case["eps"], case["momentum"], _P(rm.raw) if rm else None, _P(rv.raw) if rv else None, _P(co["mean"].raw), _P(co["invstd"].raw),
           _P(co["scale"].raw), _P(co["shift"].raw), case["replication"], _P(res.flat) if res else None, case["ldr"], rmode, act,
           _P(out.flat), case["ldo"], npix, C, Cp, _stream())
    torch.cuda.synchronize()
    one, zero = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    R = bn_coeffs_ref(wide[0::2, c0:c0 + C], wide[1::2, c0:c0 + C], case["count"], gamma if gamma is not None else one,
                      beta if beta is not None else zero, case["eps"], case["momentum"], rm0, rv0, case["replication"])
    n = float(case["count"])
    # the variance from f32 sums: 4 x 2^-24 x E[y^2] (the subtraction E[y^2] - mean^2), carried through invstd, scale and shift;
    # every stored f32 coefficient adds one rounding (2^-24 relative, taken twice)
    gam = (gamma if gamma is not None else one).double().abs()
    bet = (beta if beta is not None else zero).double().abs()
    t_var = 4.0 * U24 * R["s2"] / n
    t_mean = 2.0 * U24 * R["mean"].abs() + U24 * R["s2"].sqrt() / n
    t_inv = 0.5 * R["invstd"] / (R["var"] + case["eps"]) * t_var + 2.0 * U24 * R["invstd"]
    t_scale = gam * t_inv + 2.0 * U24 * R["scale"].abs()
    t_shift = R["mean"].abs() * t_scale + R["scale"].abs() * t_mean + 2.0 * U24 * (bet + (R["mean"] * R["scale"]).abs())
    parts = []
    for k, t in (("mean", t_mean), ("invstd", t_inv), ("scale", t_scale), ("shift", t_shift)):
        co[k].check_guards(f"ydl_bn_act_fwd_sums: {k}")
        parts.append((k, worst(co[k].v[:C], R[k], t)))
    if rm is not None:
        mom = case["momentum"]
        rm.check_guards("ydl_bn_act_fwd_sums: running_mean")
        rv.check_guards("ydl_bn_act_fwd_sums: running_var")
        parts.append(("running_mean", worst(rm.v, R["rm"], mom * t_mean + 3.0 * U24 * (rm0.double().abs() + mom * R["mean"].abs()))))
        parts.append(("running_var", worst(rv.v, R["rv"], mom * t_var * 2.0 + 3.0 * U24 * (rv0.double().abs() + mom * R["unb"].abs()))))
    ref = bn_apply_ref(yd, R["scale"], R["shift"], act, rmode, rd)
    ra = rd.abs() if rd is not None else 0.0
    # a few f32 ulps for the fast exponential and reciprocal (SiLU has slope <= 1.1), plus the coefficient tolerances carried through
    tol = (BF16_STORE if dt == 1 else 0.0) * ref.abs() + 8.0 * U24 * 1.1 * ((yd * R["scale"]).abs() + R["shift"].abs() + ra) \
        + 1.1 * (yd.abs() * t_scale + t_shift)
    parts.append(("out", worst(out.logical(), ref, tol)))
    out.check_guards("ydl_bn_act_fwd_sums: out")
    return _result("", *_merge(parts))


def check_bn_act_fwd(L, case, gen):
    dt, tdt, dev = case["dt"], _tdt(case["dt"]), gen.device
    npix, Cp = case["npix"], case["Cp"]
    out_is_y, out_is_res = case["alias"]
    if out_is_res or (out_is_y and case["ldo"] != case["ldy"]):
        raise CensusFailure("ydl_bn_act_fwd: an operand pattern the census does not reproduce")
    y = Rows(npix, case["ldy"], Cp, tdt, gen, scale=1.5, offset=0.5)
    yd = y.logical()
    res = Rows(npix, case["ldr"], Cp, tdt, gen) if case["res"] else None
    rd = res.logical() if res is not None else None
    scale = torch.rand(Cp, device=dev, generator=gen) + 0.5
    shift = torch.rand(Cp, device=dev, generator=gen) * 0.6 - 0.3
    out = y if out_is_y else Rows(npix, case["ldo"], Cp, tdt, gen, fill=False)
    L.call("ydl_bn_act_fwd", dt, _P(y.flat), case["ldy"], _P(scale), _P(shift), _P(res.flat) if res else None, case["ldr"], case["res_mode"],
           case["act"], _P(out.flat), case["ldo"], npix, Cp, _stream())
    torch.cuda.synchronize()
    ref = bn_apply_ref(yd, scale.double(), shift.double(), case["act"], case["res_mode"], rd)
    ra = rd.abs() if rd is not None else 0.0
    tol = (BF16_STORE if dt == 1 else 0.0) * ref.abs() + 8.0 * U24 * 1.1 * ((yd * scale.double()).abs() + shift.double().abs() + ra)
    parts = [("out", worst(out.logical(), ref, tol))]
    out.check_guards("ydl_bn_act_fwd: out")
    return _result("", *_merge(parts))


def check_bn_act_bwd(L, case, gen):
    entry = case["entry"]
    dt, tdt, dev = case["dt"], _tdt(case["dt"]), gen.device
    npix, C, Cp = case["npix"], case["C"], case["Cp"]
    rmode, act = case["res_mode"] & 15, case["act"]
    dres_acc = bool(case["res_mode"] & RES_GRAD_ACCUMULATE)
    dy_is_dout, dy_is_y, dres_is_dout, dres_is_dy = case["alias"]
    if dy_is_y or dres_is_dout or dres_is_dy or (dy_is_dout and case["lddy"] != case["lddo"]):
        raise CensusFailure(f"{entry}: an aliasing pattern the census does not reproduce {case['alias']}")
    if rmode == RES_BEFORE_ACT and act == ACT_SILU:
        raise CensusFailure(f"{entry}: a residual joined before SiLU cannot be differentiated without the residual operand")
    if rmode == RES_AFTER_ACT and act == ACT_RELU:
        raise CensusFailure(f"{entry}: ReLU with a residual added behind it: the saved output is not the activation's mask")
    y = Rows(npix, case["ldy"], C, tdt, gen, scale=1.5, offset=0.5)
    dout = Rows(npix, case["lddo"], C, tdt, gen, offset=0.1)
    yd, dd = y.logical(), dout.logical()
    vec = lambda t: torch.cat([t.float(), torch.zeros(Cp - C, device=dev)])
    mean = vec(yd.mean(0))
    invstd = vec(1.0 / torch.sqrt(yd.var(0, unbiased=False) + 1e-3))
    gamma = vec(torch.rand(C, device=dev, generator=gen) + 0.5)
    scale = gamma * invstd
    shift = vec(torch.rand(C, device=dev, generator=gen) * 0.6 - 0.3)
    m64, i64, s64, f64 = (t[:C].double() for t in (mean, invstd, scale, shift))
    out, od = None, None
    if case["out"]:
        # the saved output of the forward (ReLU takes its mask from it): act(z [+ r]) for some residual r joined before the activation
        out = Rows(npix, case["ldo"], C, tdt, gen, fill=False)
        z = yd * s64 + f64
        if rmode == RES_BEFORE_ACT:
            z = z + torch.randn(npix, C, device=dev, generator=gen, dtype=torch.float64)
        out.v[:, :C] = act_f64(z, act).to(tdt)
        od = out.logical()
    dres = Rows(npix, case["lddr"], C, tdt, gen, fill=dres_acc) if case["dres"] else None
    dres_prior = dres.logical() if (dres is not None and dres_acc) else None
    dy = dout if dy_is_dout else Rows(npix, case["lddy"], C, tdt, gen, fill=False)
    pg0 = torch.randn(C, device=dev, generator=gen) if case["accp"] else torch.full((C,), CANARY, device=dev)
    pb0 = torch.randn(C, device=dev, generator=gen) if case["accp"] else torch.full((C,), CANARY, device=dev)
    dgamma = Floats(C, dev, pg0) if case["dgamma"] else None
    dbeta = Floats(C, dev, pb0) if case["dbeta"] else None
    R = bn_bwd_ref(yd, dd, m64, i64, s64, f64, act, rmode, out=od, dres_prior=dres_prior)
    given = None
    if entry == "ydl_bn_act_bwd":
        q = L.lib().ydl_bn_bwd_ws_bytes(npix, Cp) // 4
        ws = Floats(max(q, 4), dev)
        L.call(entry, dt, _P(y.flat), case["ldy"], _P(dout.flat), case["lddo"], _P(out.flat) if out else None, case["ldo"], _P(gamma), _P(mean),
               _P(invstd), _P(scale), _P(shift), case["res_mode"], act, _P(dy.flat), case["lddy"], _P(dres.flat) if dres else None, case["lddr"],
               _P(dgamma.raw) if dgamma else None, _P(dbeta.raw) if dbeta else None, case["accp"], _P(ws.raw), npix, C, Cp, _stream())
        torch.cuda.synchronize()
        ws.check_guards(f"{entry}: workspace")
    else:
        sums = Floats(8 * 2 * Cp, dev)
        if entry == "ydl_bn_act_bwd_apply_sums":
            # the reduce pass ran elsewhere: feed its float64 result split across the replica rows, rounded to f32, and take the
            # reference FROM the f32 rows as given
            sv = sums.v.view(8, 2, Cp)
            sv[:, 0, :C] = _split_rows(R["dbeta"], gen)
            sv[:, 1, :C] = _split_rows(R["dgamma"], gen)
            given = (sv[:, 0, :C].double().sum(0), sv[:, 1, :C].double().sum(0))
            R = bn_bwd_ref(yd, dd, m64, i64, s64, f64, act, rmode, out=od, dres_prior=dres_prior, sums=given)
        L.call(entry, dt, _P(y.flat), case["ldy"], _P(dout.flat), case["lddo"], _P(out.flat) if out else None, case["ldo"], _P(mean), _P(invstd),
               _P(scale), _P(shift), case["res_mode"], act, _P(dy.flat), case["lddy"], _P(dres.flat) if dres else None, case["lddr"],
               _P(dgamma.raw) if dgamma else None, _P(dbeta.raw) if dbeta else None, case["accp"], _P(sums.raw), npix, C, Cp, _stream())
        torch.cuda.synchronize()
        sums.check_guards(f"{entry}: replica sums")
    n = float(npix)
    t_b, t_g = BN_BWD_TOL * R["sq_b"], BN_BWD_TOL * R["sq_g"]
    rb, rg = (given if given is not None else (R["dbeta"], R["dgamma"]))
    parts = []
    for name, buf, refv, t, p0 in (("dgamma", dgamma, rg, t_g, pg0), ("dbeta", dbeta, rb, t_b, pb0)):
        if buf is None:
            continue
        buf.check_guards(f"{entry}: {name}")
        total = refv + (p0.double() if case["accp"] else 0.0)
        # the project's BN_BWD_TOL on the sum, plus the f32 roundings of the stored value and of the add onto the prior contents
        parts.append((name, worst(buf.v, total, t + 2.0 * U24 * (total.abs() + refv.abs()))))
    # f32 evaluation of dz (fast sigmoid: a few ulps; an argument error of 2^-23 |z| meets |silu''| <= 1/2), xhat and the two products
    e_f32 = 16.0 * U24 * s64.abs() * (R["dz"].abs() * (1.0 + R["z"].abs()) + R["kb"].abs() + (R["xhat"] * R["kg"]).abs())
    store = BF16_STORE if dt == 1 else 0.0
    tol = store * R["dy"].abs() + s64.abs() * (t_b + R["xhat"].abs() * t_g) / n + e_f32
    parts.append(("dy", worst(dy.logical(), R["dy"], tol)))
    dy.check_guards(f"{entry}: dy")
    if dres is not None:
        e_dz = 16.0 * U24 * R["dz"].abs() * (1.0 + R["z"].abs()) if rmode == RES_BEFORE_ACT else 0.0
        parts.append(("dres", worst(dres.logical(), R["dres"], store * R["dres"].abs() + e_dz)))
        dres.check_guards(f"{entry}: dres")
    return _result("", *_merge(parts))


CHECKERS = {"ydl_conv_fwd": check_conv_fwd, "ydl_conv_fwd_sums": check_conv_fwd, "ydl_conv_dgrad": check_conv_dgrad,
            "ydl_conv_wgrad": check_conv_wgrad, "ydl_conv_wgrad_det": check_conv_wgrad, "ydl_conv_bwd_pw": check_conv_bwd_pw,
            "ydl_bn_act_fwd_sums": check_bn_act_fwd_sums, "ydl_bn_act_fwd": check_bn_act_fwd, "ydl_bn_act_bwd_sums": check_bn_act_bwd,
            "ydl_bn_act_bwd_apply_sums": check_bn_act_bwd, "ydl_bn_act_bwd": check_bn_act_bwd}


def check_case(case: dict) -> dict:
    """run one distinct launch on fresh operands -> dict(kernel, ratio = worst |error| / bound, over = elements over their bound,
    detail); raises CensusFailure for an overrun, a launch the census cannot reproduce or an entry point without a checker"""
    from yolo_dual_amd import _lib as L
    entry = case["entry"]
    if case.get("unknown") or entry not in CHECKERS:
        raise CensusFailure(f"{entry}: the census has no checker for this entry point")
    if entry == "ydl_conv_fwd" and case["stats"]:
        raise CensusFailure("ydl_conv_fwd with partial-row statistics: the census has no checker for this form")
    gen = torch.Generator(torch.device("cuda", torch.cuda.current_device())).manual_seed(_seed(case))
    return CHECKERS[entry](L, case, gen)


def describe(case: dict) -> str:
    """geometry, strides and flags of a case in one table cell"""
    if "g" in case:
        g = case["g"]
        s = (f"N{g.N} {g.Hi}x{g.Wi}x{g.Cin}->{g.Ho}x{g.Wo}x{g.Cout} k{g.k}s{g.s}p{g.p} ldx{g.ldx} ldy{g.ldy} ldw{g.ldw}")
        for k in ("lddx", "acc", "stats"):
            if k in case:
                s += f" {k}={int(case[k])}"
        return s
    skip = ("entry", "eps", "momentum")
    return " ".join(f"{k}={int(v) if isinstance(v, bool) else v}" for k, v in case.items() if k not in skip)
