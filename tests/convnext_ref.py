"""Plain-torch float64 reference of the ConvNeXt pieces: the three kernels' formulas on [npix, C] rows, LayerNorm2d, CNBlock, the
patchify convolutions and the three backbone rows.  Written from the definition (torchvision's ``convnext_tiny``, restated in the
README): nn.Conv2d, F.layer_norm, nn.Linear, F.gelu(approximate='none').  torchvision itself is not installed where the tests run, so
parity with its own classes is not pinned; the state_dict keys and shapes are its.  Not collected.

``store=True`` rounds every tensor a bf16 implementation stores to bf16 (value forward, gradient backward) and the GEMM weights forward:
the reference's own error under bf16 storage, the floor the bf16 tests are held against."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

U24, U8 = 2.0 ** -24, 2.0 ** -8
BF16_STORE = U8 * (1.0 + 2.0 ** -6)
DIMS, DEPTHS = (96, 192, 384, 768), (3, 3, 9, 3)


def rnd(t, bf16):
    """float64 holding values of the storage type"""
    return t.to(torch.bfloat16).double() if bf16 else t.float().double()


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' formulas on rows [npix, C], float64; the ``wrong`` switches exist for tests/test_convnext_ref_cpu.py
# ---------------------------------------------------------------------------------------------------------------------
def ln_fwd(x, pre_bias, gamma, beta, eps, ddof=0):
    u = x if pre_bias is None else x + pre_bias
    C = u.shape[1]
    mu = u.mean(1, keepdim=True)
    var = ((u - mu) ** 2).sum(1, keepdim=True) / (C - ddof)
    r = 1.0 / torch.sqrt(var + eps)
    xh = (u - mu) * r
    return dict(y=xh * gamma + beta, mu=mu[:, 0], r=r[:, 0], xh=xh, u=u)


def ln_bwd(x, pre_bias, gamma, mu, r, dy):
    """from the STORED statistics (mu, r), as the kernel reads them"""
    u = x if pre_bias is None else x + pre_bias
    xh = (u - mu[:, None]) * r[:, None]
    g = dy * gamma
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dx = r[:, None] * (g - m1 - xh * m2)
    return dict(dx=dx, dgamma=(dy * xh).sum(0), dbeta=dy.sum(0), dpre_bias=dx.sum(0), xh=xh, g=g, m1=m1, m2=m2)


def gelu_fwd(z, bias, approximate="none"):
    u = z + bias
    if approximate == "tanh":
        return 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u ** 3)))
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def gelu_parts(u):
    cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    return cdf, pdf


def gelu_bwd(z, bias, dy):
    u = z + bias
    cdf, pdf = gelu_parts(u)
    dz = dy * (cdf + u * pdf)
    return dict(dz=dz, dbias=dz.sum(0), u=u, cdf=cdf, pdf=pdf)


def _keep_rows(keep, npix, hw):
    if keep is None:
        return torch.ones(npix, 1, dtype=torch.float64)
    return keep.double().repeat_interleave(hw)[:, None]


def scale_res_fwd(y, gamma, keep, x, hw):
    return x + _keep_rows(keep, y.shape[0], hw) * gamma * y


def scale_res_bwd(dout, y, gamma, keep, hw, keep_in_dgamma=True):
    k = _keep_rows(keep, y.shape[0], hw)
    return dict(dy=k * gamma * dout, dgamma=((k if keep_in_dgamma else 1.0) * dout * y).sum(0), dx=dout, k=k)


def compare(got, ref, tol):
    """(worst |got - ref| / tol, elements over their bound); a zero bound demands equality, a non-finite value is over any bound"""
    got, ref = got.double(), ref.double()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(ref)
    diff = (got - ref).abs()
    diff = torch.where(torch.isfinite(got), diff, torch.full_like(diff, float("inf")))
    ratio = torch.where(tol > 0, diff / tol.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))
    return (float(ratio.max()) if ratio.numel() else 0.0), int((ratio > 1.0).sum())


# ---------------------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------------------
class _RoundBoth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _rd(store):
    return _RoundBoth.apply if store else (lambda t: t)


def _wr(w, store):
    """a GEMM weight as the bf16 path reads it: rounded on the way forward, the f32 master receives the gradient"""
    return w + (w.to(torch.bfloat16).to(w.dtype) - w).detach() if store else w


class LayerNorm2d(nn.Module):
    def __init__(self, C, eps=1e-6, store=False):
        super().__init__()
        self.weight, self.bias, self.eps, self.store = nn.Parameter(torch.ones(C)), nn.Parameter(torch.zeros(C)), eps, store

    def forward(self, x):
        y = F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), self.weight, self.bias, self.eps).permute(0, 3, 1, 2)
        return _rd(self.store)(y)


class PatchConv2d(nn.Conv2d):
    def __init__(self, c1, c2, k, store=False):
        super().__init__(c1, c2, k, k)
        self.store = store

    def forward(self, x):
        rd = _rd(self.store)
        if not self.store:
            return super().forward(x)
        if x.shape[1] == 3:                  # the image: the edge conversion stores it in bf16
            x = rd(x)
        return rd(F.conv2d(x, _wr(self.weight, True), self.bias, self.stride))


class CNBlock(nn.Module):
    """x + keep * layer_scale * fc2(GELU(fc1(LN(dwconv7x7(x))))).  ``keep``: the per-sample factors bernoulli(1 - p) / (1 - p) of
    stochastic depth in "row" mode, given by the caller (``fixed_keep``), drawn in train mode with p > 0, absent otherwise."""

    def __init__(self, dim, layer_scale=1e-6, stochastic_depth_prob=0.0, store=False):
        super().__init__()
        self.block = nn.Sequential(nn.Conv2d(dim, dim, 7, padding=3, groups=dim), nn.Identity(), nn.LayerNorm(dim, eps=1e-6),
                                   nn.Linear(dim, 4 * dim), nn.GELU(), nn.Linear(4 * dim, dim), nn.Identity())
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * layer_scale)
        self.p, self.store, self.fixed_keep = stochastic_depth_prob, store, None

    def branch(self, x):
        dw, ln, fc1, fc2 = self.block[0], self.block[2], self.block[3], self.block[5]
        rd, st = _rd(self.store), self.store
        t = rd(F.conv2d(x, dw.weight, None, 1, 3, 1, x.shape[1])) + dw.bias.view(1, -1, 1, 1)
        t = rd(F.layer_norm(t.permute(0, 2, 3, 1), (x.shape[1],), ln.weight, ln.bias, ln.eps))
        t = rd(F.linear(t, _wr(fc1.weight, st))) + fc1.bias
        t = rd(F.gelu(t, approximate="none"))
        t = rd(F.linear(t, _wr(fc2.weight, st), fc2.bias))
        return t.permute(0, 3, 1, 2)

    def forward(self, x):
        t = self.layer_scale * self.branch(x)
        keep = self.fixed_keep
        if keep is None and self.training and self.p > 0:
            keep = torch.empty(x.shape[0], dtype=x.dtype).bernoulli_(1.0 - self.p) / (1.0 - self.p)
        if keep is not None:
            t = t * keep.to(t.dtype).view(-1, 1, 1, 1)
        return _rd(self.store)(x + t)


def stem(c1, c2, k=4, store=False):
    return nn.Sequential(PatchConv2d(c1, c2, k, store), LayerNorm2d(c2, store=store))


def down(c1, c2, store=False):
    return nn.Sequential(LayerNorm2d(c1, store=store), PatchConv2d(c1, c2, 2, store))


def _stage(i, sd, ls, store):
    first = sum(DEPTHS[:i])
    return nn.Sequential(*(CNBlock(DIMS[i], ls, sd * (first + j) / (sum(DEPTHS) - 1.0), store) for j in range(DEPTHS[i])))


class _Row(nn.Module):
    def __init__(self, parts):
        super().__init__()
        self.model = nn.Sequential(*parts)

    def forward(self, x):
        return self.model(x)


def convnext_tiny1(stochastic_depth_prob=0.1, layer_scale=1e-6, store=False):
    sd, ls = stochastic_depth_prob, layer_scale
    return _Row([stem(3, DIMS[0], 4, store), _stage(0, sd, ls, store), down(DIMS[0], DIMS[1], store), _stage(1, sd, ls, store)])


def convnext_tiny2(stochastic_depth_prob=0.1, layer_scale=1e-6, store=False):
    return _Row([down(DIMS[1], DIMS[2], store), _stage(2, stochastic_depth_prob, layer_scale, store)])


def convnext_tiny3(stochastic_depth_prob=0.1, layer_scale=1e-6, store=False):
    return _Row([down(DIMS[2], DIMS[3], store), _stage(3, stochastic_depth_prob, layer_scale, store)])
