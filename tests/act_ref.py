"""float64 reference of the Conv activations (torch tensors, any device), shared by tests/test_act_ref_cpu.py, which pins it to torch
autograd, and tests/test_gpu_act_kernels.py, which holds the kernels to it per element.

  * the three point-wise activations of the streaming BatchNorm kernels (YDL_ACT_LEAKY / HSWISH / MISH of include/ydl.h): value, first
    and second derivative, kinks, Lipschitz constant;
  * AconC forward and backward: out = d * sigmoid(beta * d) + p2 * z with d = (p1 - p2) * z;
  * the max merge of FReLU with torch's tie rule (half to each operand);
  * the operands of the kernel cases, drawn on the CPU from a seed so that the CPU test can check the kink condition of the very
    tensors the GPU test uses;
  * ``compare``: the worst |got - ref| / tol over the elements that are not left out."""
import math

import torch

ACT_NONE, ACT_SILU, ACT_RELU, ACT_LEAKY, ACT_HSWISH, ACT_MISH = 0, 1, 2, 3, 4, 5
U24, U8 = 2.0 ** -24, 2.0 ** -8
BF16_STORE = U8 * (1.0 + 2.0 ** -6)

# Lipschitz constants: max |act'| is 1 for LeakyReLU (slope < 1), 1.5 for Hardswish (at z = 3) and 1.0886 for Mish
LIPSCHITZ = {ACT_LEAKY: 1.0, ACT_HSWISH: 1.5, ACT_MISH: 1.1}
KINKS = {ACT_LEAKY: (0.0,), ACT_HSWISH: (-3.0, 3.0), ACT_MISH: ()}

# (pixels, channels C, padded channels Cp, row stride) of the kernel cases: a stride wider than the channels, a channel tail, and a
# pixel count that needs more than one CTA in the reduce passes
SHAPES = {"70x24_ld32": (70, 24, 24, 32), "70x20_cp24": (70, 20, 24, 24), "2046x16": (2046, 16, 16, 16)}
SLOPE = 0.1


def _softplus(z):
    return torch.where(z > 30.0, z, torch.log1p(torch.exp(torch.clamp(z, max=30.0))))


def act(z, code, slope=0.0):
    z = z.double()
    if code == ACT_LEAKY:
        return torch.where(z > 0, z, slope * z)
    if code == ACT_HSWISH:
        return z * torch.clamp(z + 3.0, 0.0, 6.0) / 6.0
    if code == ACT_MISH:
        return z * torch.tanh(_softplus(z))
    raise ValueError(code)


def dact(z, code, slope=0.0):
    """act'(z); at a kink the value of the side the kernels take (z > 0 is the positive side, |z| > 3 the outer one)"""
    z = z.double()
    if code == ACT_LEAKY:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    if code == ACT_HSWISH:
        return torch.where(z < -3.0, torch.zeros_like(z), torch.where(z > 3.0, torch.ones_like(z), (2.0 * z + 3.0) / 6.0))
    if code == ACT_MISH:
        t = torch.tanh(_softplus(z))
        return t + z * torch.sigmoid(z) * (1.0 - t * t)
    raise ValueError(code)


def d2act(z, code, slope=0.0):
    """act''(z) away from the kinks"""
    z = z.double()
    if code == ACT_LEAKY:
        return torch.zeros_like(z)
    if code == ACT_HSWISH:
        return torch.where(z.abs() < 3.0, torch.full_like(z, 1.0 / 3.0), torch.zeros_like(z))
    if code == ACT_MISH:
        t, s = torch.tanh(_softplus(z)), torch.sigmoid(z)
        dt = s * (1.0 - t * t)
        return 2.0 * dt + z * (s * (1.0 - s) * (1.0 - t * t) - 2.0 * t * dt * s)
    raise ValueError(code)


def max_d2(code):
    """the largest |act''| in float64, over a dense grid of [-30, 30]"""
    return float(d2act(torch.linspace(-30.0, 30.0, 600001, dtype=torch.float64), code).abs().max())


def near_kink(z, code, dz):
    """elements whose z lies within the argument error dz of a kink of the activation: left out of a comparison"""
    m = torch.zeros_like(z, dtype=torch.bool)
    for k in KINKS[code]:
        m |= (z - k).abs() <= dz
    return m


def acon_fwd(z, p1, p2, beta):
    z, p1, p2, beta = (t.double() for t in (z, p1, p2, beta))
    d = (p1 - p2) * z
    return d * torch.sigmoid(beta * d) + p2 * z


def acon_bwd(z, dout, p1, p2, beta):
    """-> dict(dz, dp1, dp2, dbeta and, for the bounds, the summands' absolute sums a1, a2, ab and root sums of squares q1, q2, qb)"""
    z, dout, p1, p2, beta = (t.double() for t in (z, dout, p1, p2, beta))
    d = (p1 - p2) * z
    s = torch.sigmoid(beta * d)
    g = s * (1.0 + beta * d * (1.0 - s))
    t1, t2, tb = dout * z * g, dout * z * (1.0 - g), dout * d * d * s * (1.0 - s)
    r = dict(dz=dout * ((p1 - p2) * g + p2), dp1=t1.sum(0), dp2=t2.sum(0), dbeta=tb.sum(0), d=d, g=g)
    for k, t in (("1", t1), ("2", t2), ("b", tb)):
        r["a" + k], r["q" + k] = t.abs().sum(0), (t * t).sum(0).sqrt()
    return r


def max2_fwd(a, b):
    return torch.maximum(a.double(), b.double())


def max2_bwd(a, b, dout, tie=0.5):
    """(da, db): dout to the larger operand; on a tie ``tie`` of it to a and the rest to b (torch.max(a, b): one half each)"""
    a, b, dout = a.double(), b.double(), dout.double()
    da = torch.where(a > b, dout, torch.where(a == b, tie * dout, torch.zeros_like(dout)))
    return da, dout - da


def compare(got, ref, tol, skip=None):
    """(worst |got - ref| / tol, elements over their bound, fraction left out).  A zero bound demands equality; a non-finite value is
    over any bound; ``skip`` marks elements that are not compared."""
    got, ref = got.double(), ref.double()
    tol = torch.as_tensor(tol, dtype=torch.float64, device=ref.device).expand_as(ref)
    diff = (got - ref).abs()
    diff = torch.where(torch.isfinite(got), diff, torch.full_like(diff, float("inf")))
    ratio = torch.where(tol > 0, diff / tol.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))
    left = 0.0
    if skip is not None:
        ratio = torch.where(skip, torch.zeros_like(ratio), ratio)
        left = float(skip.double().mean())
    return float(ratio.max()) if ratio.numel() else 0.0, int((ratio > 1.0).sum()), left


def acc_bound(K, Q, A):
    """f32 accumulation of K terms, as tests/census.py: min(4 sqrt(K) 2^-24 Q, (K + 1) 2^-24 A)"""
    return torch.minimum(4.0 * math.sqrt(K) * U24 * Q, (K + 1.0) * U24 * A)


def _round(t, bf16):
    return t.to(torch.bfloat16).double() if bf16 else t.float().double()


def bn_case(shape, code, bf16, seed=0):
    """the operands of one streaming BatchNorm case, float64 tensors on the CPU holding values of the storage type: y, dout and res
    [npix, C], and f32 mean, invstd, scale, shift [C].  Same draws as tests/census.py's BatchNorm checks."""
    npix, C, _Cp, _ld = SHAPES[shape]
    gen = torch.Generator().manual_seed(9000 + 97 * seed + 7 * code + (1 if bf16 else 0) + 13 * sorted(SHAPES).index(shape))
    y = _round(torch.randn(npix, C, generator=gen, dtype=torch.float64) * 1.5 + 0.5, bf16)
    dout = _round(torch.randn(npix, C, generator=gen, dtype=torch.float64) + 0.1, bf16)
    res = _round(torch.randn(npix, C, generator=gen, dtype=torch.float64), bf16)
    mean = y.mean(0).float().double()
    invstd = (1.0 / torch.sqrt(y.var(0, unbiased=False) + 1e-3)).float().double()
    gamma = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double()
    scale = (gamma.float() * invstd.float()).double()
    shift = (torch.rand(C, generator=gen, dtype=torch.float64) * 0.6 - 0.3).float().double()
    return dict(y=y, dout=dout, res=res, mean=mean, invstd=invstd, scale=scale, shift=shift)


def bn_fwd_ref(c, code, slope, with_res):
    """-> (out, z, argument error of z, tolerance without the store term).  out = act(y*scale + shift) [+ res]."""
    z = c["y"] * c["scale"] + c["shift"]
    out = act(z, code, slope) + (c["res"] if with_res else 0.0)
    mag = (c["y"] * c["scale"]).abs() + c["shift"].abs() + (c["res"].abs() if with_res else 0.0)
    dz = 8.0 * U24 * mag
    return out, z, dz, LIPSCHITZ[code] * dz + 8.0 * U24 * out.abs()


def bn_bwd_ref(c, code, slope):
    """float64 BatchNorm + activation backward -> dict(z, dz, xhat, dbeta, dgamma, dy, kb, kg, sq_b, sq_g)"""
    n = float(c["y"].shape[0])
    z = c["y"] * c["scale"] + c["shift"]
    dz = c["dout"] * dact(z, code, slope)
    xhat = (c["y"] - c["mean"]) * c["invstd"]
    db, dg = dz.sum(0), (dz * xhat).sum(0)
    return dict(z=z, dz=dz, xhat=xhat, dbeta=db, dgamma=dg, kb=db / n, kg=dg / n, dy=c["scale"] * (dz - db / n - xhat * dg / n),
                sq_b=(dz * dz).sum(0).sqrt(), sq_g=((dz * xhat) ** 2).sum(0).sqrt())


def acon_case(shape, bf16, seed=0):
    npix, C, _Cp, _ld = SHAPES[shape]
    gen = torch.Generator().manual_seed(9500 + 97 * seed + (1 if bf16 else 0) + 13 * sorted(SHAPES).index(shape))
    z = _round(torch.randn(npix, C, generator=gen, dtype=torch.float64) * 1.5 + 0.2, bf16)
    dout = _round(torch.randn(npix, C, generator=gen, dtype=torch.float64) + 0.1, bf16)
    p1 = torch.randn(C, generator=gen, dtype=torch.float64).float().double()
    p2 = torch.randn(C, generator=gen, dtype=torch.float64).float().double()
    beta = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double()
    return dict(z=z, dout=dout, p1=p1, p2=p2, beta=beta)


def max2_case(shape, bf16, seed=0):
    """a, b, dout with exact ties planted: every 5th element of b equals a's"""
    npix, C, _Cp, _ld = SHAPES[shape]
    gen = torch.Generator().manual_seed(9700 + 97 * seed + (1 if bf16 else 0) + 13 * sorted(SHAPES).index(shape))
    a = _round(torch.randn(npix, C, generator=gen, dtype=torch.float64), bf16)
    b = _round(torch.randn(npix, C, generator=gen, dtype=torch.float64), bf16)
    dout = _round(torch.randn(npix, C, generator=gen, dtype=torch.float64), bf16)
    tie = (torch.arange(npix * C).view(npix, C) % 5) == 0
    b = torch.where(tie, a, b)
    return dict(a=a, b=b, dout=dout, tie=tie)
