"""Plain-torch float64 reference of the squeeze-excitation pieces: the kernels' closed formulas on [N, HW, C] rows with the bounds the
kernel tests hold them to, SqueezeExcitation, Conv2dNormActivation, InvertedResidual, MBConv and the six backbone rows.  Written from
the definition (torchvision's ``mobilenet_v3_small`` and ``efficientnet_b0``, restated in DESIGN.md): nn.Conv2d, nn.BatchNorm2d,
F.adaptive_avg_pool2d, F.hardsigmoid, F.silu.  torchvision itself is not installed where the tests run, so parity with its own classes
is not pinned; the state_dict keys and shapes are its.  Not collected.

``store=True`` rounds to bf16 wherever a bf16 implementation stores: every dense convolution weight on the way forward, every
convolution output (before its BatchNorm), every BatchNorm + activation (+ residual) output, the gated tensor x * g and a block's
output, each with its incoming gradient.  The pooled vector, the gate and the SE parameters stay in f32, as the kernels keep them."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.convnext_ref import BF16_STORE, U8, U24, _rd, _wr, compare, rnd            # noqa: F401  (re-exported for the tests)

K_EXP = 4          # roundings of a value formed with one expf, one addition and one division or product (act, sigmoid)
K_DEXP = 6         # ... of a derivative formed with one expf and up to five further operations
TINY = 2.0 ** -126  # the smallest normal f32: where expf over- or underflows, a value loses its relative precision to at most this


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' formulas, float64; the ``wrong`` switches exist for tests/test_se_ref_cpu.py
# ---------------------------------------------------------------------------------------------------------------------
def act_fwd(h, act):
    return torch.relu(h) if act == "relu" else h * torch.sigmoid(h)


def act_grad(h, act):
    if act == "relu":
        return (h > 0).to(h.dtype)
    s = torch.sigmoid(h)
    return s * (1 + h * (1 - s))


def gate_fwd(z, gate):
    return torch.clamp(z + 3, 0, 6) / 6 if gate == "hardsigmoid" else torch.sigmoid(z)


def gate_grad(z, gate, live_at_3=False, from_gate=None):
    """d scale / d z.  Hardsigmoid: 1/6 for -3 < z < 3 and 0 otherwise (ATen's rule; ``live_at_3`` takes the closed interval).
    ``from_gate``: a stored gate to differentiate the sigmoid from, g (1 - g), in place of z."""
    if gate == "hardsigmoid":
        inside = (z >= -3) & (z <= 3) if live_at_3 else (z > -3) & (z < 3)
        return inside.to(z.dtype) / 6
    if from_gate is not None:
        return from_gate * (1 - from_gate)
    e = torch.exp(-z.abs())                          # g (1 - g) without the cancellation in 1 - g: exact relative precision at any |z|
    return e / (1 + e) ** 2


def pool_fwd(x):
    """x [N, HW, C] -> mean over HW"""
    return x.mean(1)


def excite_fwd(p, w1, b1, w2, b2, act, gate):
    h = p @ w1.T + b1
    a = act_fwd(h, act)
    z = a @ w2.T + b2
    return dict(h=h, a=a, z=z, g=gate_fwd(z, gate))


def excite_bwd(dgate, p, h, z, w1, w2, act, gate, live_at_3=False, from_gate=None):
    dz = dgate * gate_grad(z, gate, live_at_3, from_gate)
    a = act_fwd(h, act)
    dh = (dz @ w2) * act_grad(h, act)
    return dict(dz=dz, dh=dh, dpooled=dh @ w1, dw1=dh.T @ p, db1=dh.sum(0), dw2=dz.T @ a, db2=dz.sum(0))


def scale_bwd(dy, g, dpooled, drop_pooled=False):
    """dy [N, HW, C] -> dx = dy * g[n, c] + dpooled[n, c] / HW"""
    dx = dy * g[:, None, :]
    return dx if drop_pooled else dx + dpooled[:, None, :] / dy.shape[1]


def se_all(x, dout, w1, b1, w2, b2, act, gate):
    """the whole gate both ways on rows x, dout [N, HW, C] -> out, dx and the four parameter gradients"""
    p = pool_fwd(x)
    f = excite_fwd(p, w1, b1, w2, b2, act, gate)
    b = excite_bwd((dout * x).sum(1), p, f["h"], f["z"], w1, w2, act, gate)
    return dict(out=x * f["g"][:, None, :], dx=scale_bwd(dout, f["g"], b["dpooled"]), p=p, **f, **b)


# bounds of the kernel tests, in the project's form 2 K 2^-24 S: S is the kernel's own expression on absolute values, K the length of
# its summation chain.  Every stage is compared on the operands the kernel itself read (its own stored pooled, h, z, dz, dh).
def chain_dot(C):
    """a wave's dot product over C terms: ceil(C / 64) fused multiply-adds per lane, six butterfly additions, the bias or factor"""
    return (C + 63) // 64 + 6 + 1


def bound(K, S):
    """2 K 2^-24 S, plus K quanta of the subnormal range (2^-149) wherever S is not zero: below 2^-126 an f32 rounding is absolute, not
    relative.  S == 0 keeps a zero bound (products with an exact zero are exact)."""
    S = torch.as_tensor(S, dtype=torch.float64)
    return 2.0 * K * U24 * S + K * 2.0 ** -149 * (S > 0)


def bound_h(p, w1, b1):
    return bound(chain_dot(p.shape[1]), p.abs() @ w1.abs().T + b1.abs())


def bound_z(h, w2, b2, act):
    a = act_fwd(h, act).abs()
    under = TINY * (h.abs() @ w2.abs().T) if act == "silu" else 0.0
    return bound(w2.shape[1] + 1, a @ w2.abs().T + b2.abs()) + bound(K_EXP, a @ w2.abs().T) + under


def bound_gate(z, gate):
    if gate == "hardsigmoid":
        return bound(3, (z.abs() + 3) / 6)             # the addition z + 3, the clamp (exact) and the division
    return bound(K_EXP, gate_fwd(z, gate)) + TINY


def bound_dz(dgate_parts, z, gate):
    """dgate_parts [N, S, C]"""
    S = dgate_parts.abs().sum(1)
    return bound(dgate_parts.shape[1] - 1 + K_DEXP, S * gate_grad(z, gate)) + (TINY * S if gate == "sigmoid" else 0.0)


def bound_dh(dz, h, w2, act):
    S = dz.abs() @ w2.abs()
    return bound(chain_dot(dz.shape[1]) + K_DEXP, S * act_grad(h, act).abs()) + (TINY * (1 + h.abs()) * S if act == "silu" else 0.0)


def bound_dpooled(dh, w1):
    return bound(dh.shape[1], dh.abs() @ w1.abs())


def bound_param(N, S, extra=0):
    """a sum over N samples added into a stored value: N products and additions, the addition into the destination"""
    return bound(N + 1 + extra, S)


def bound_scale_bwd(dy, g, dpooled, old, bf16):
    hw = dy.shape[1]
    S = dy.abs() * g.abs()[:, None, :] + dpooled.abs()[:, None, :] / hw + (0 if old is None else old.abs())
    ref = scale_bwd(dy, g, dpooled) + (0 if old is None else old)
    return bound(4, S) + (BF16_STORE * ref.abs() if bf16 else 0)


# ---------------------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------------------
class SqueezeExcitation(nn.Module):
    def __init__(self, C, Cs, activation="relu", scale_activation="sigmoid", store=False):
        super().__init__()
        self.fc1, self.fc2 = nn.Conv2d(C, Cs, 1), nn.Conv2d(Cs, C, 1)
        self.act, self.gate, self.store = activation, scale_activation, store

    def forward(self, x):
        s = self.fc1(F.adaptive_avg_pool2d(x, 1))
        s = F.relu(s) if self.act == "relu" else F.silu(s)
        s = self.fc2(s)
        s = F.hardsigmoid(s) if self.gate == "hardsigmoid" else torch.sigmoid(s)
        return _rd(self.store)(x * s)


_ACTS = {"relu": F.relu, "re": F.relu, "hardswish": F.hardswish, "hs": F.hardswish, "silu": F.silu, "none": lambda t: t}


class Conv2dNormActivation(nn.Sequential):
    """keys 0.weight, 1.*; ``res`` is added behind the BatchNorm and the sum stored once"""

    def __init__(self, c1, c2, k=3, s=1, g=1, activation="relu", eps=1e-5, momentum=0.1, store=False):
        super().__init__(nn.Conv2d(c1, c2, k, s, (k - 1) // 2, groups=g, bias=False), nn.BatchNorm2d(c2, eps=eps, momentum=momentum))
        self.fn, self.store, self.dense = _ACTS[str(activation).lower()], store, g == 1

    def forward(self, x, res=None):
        conv, bn = self[0], self[1]
        rd = _rd(self.store)
        if self.store and x.shape[1] == 3:               # the image: the edge conversion stores it in bf16
            x = rd(x)
        w = _wr(conv.weight, self.store and self.dense)
        y = self.fn(bn(rd(F.conv2d(x, w, None, conv.stride, conv.padding, 1, conv.groups))))
        return rd(y if res is None else y + res)


def make_divisible(v, divisor=8):
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


class InvertedResidual(nn.Module):
    def __init__(self, cin, k, exp, cout, use_se, activation, stride, store=False):
        super().__init__()
        bn = dict(eps=1e-3, momentum=0.01, store=store)
        layers = [] if exp == cin else [Conv2dNormActivation(cin, exp, 1, activation=activation, **bn)]
        layers.append(Conv2dNormActivation(exp, exp, k, stride, exp, activation=activation, **bn))
        if use_se:
            layers.append(SqueezeExcitation(exp, make_divisible(exp // 4, 8), "relu", "hardsigmoid", store))
        layers.append(Conv2dNormActivation(exp, cout, 1, activation="none", **bn))
        self.block = nn.Sequential(*layers)
        self.res = stride == 1 and cin == cout

    def forward(self, x):
        h = x
        for m in self.block[:-1]:
            h = m(h)
        return self.block[-1](h, x if self.res else None)


class MBConv(nn.Module):
    """``fixed_keep``: the per-sample factors bernoulli(1 - p) / (1 - p) of stochastic depth, given by the caller; drawn in train mode
    with p > 0, absent otherwise.  With keep factors the projection's output is stored before the residual is joined."""

    def __init__(self, ratio, k, stride, cin, cout, stochastic_depth_prob=0.0, store=False):
        super().__init__()
        exp = cin * ratio
        layers = [] if exp == cin else [Conv2dNormActivation(cin, exp, 1, activation="silu", store=store)]
        layers.append(Conv2dNormActivation(exp, exp, k, stride, exp, activation="silu", store=store))
        layers.append(SqueezeExcitation(exp, max(1, cin // 4), "silu", "sigmoid", store))
        layers.append(Conv2dNormActivation(exp, cout, 1, activation="none", store=store))
        self.block = nn.Sequential(*layers)
        self.res, self.p, self.store, self.fixed_keep = stride == 1 and cin == cout, stochastic_depth_prob, store, None

    def forward(self, x):
        h = x
        for m in self.block[:-1]:
            h = m(h)
        keep = self.fixed_keep
        if keep is None and self.res and self.training and self.p > 0:
            keep = torch.empty(x.shape[0], dtype=x.dtype).bernoulli_(1.0 - self.p) / (1.0 - self.p)
        if not self.res or keep is None:
            return self.block[-1](h, x if self.res else None)
        return _rd(self.store)(x + self.block[-1](h) * keep.to(x.dtype).view(-1, 1, 1, 1))


MNV3S = ((16, 3, 16, 16, True, "RE", 2), (16, 3, 72, 24, False, "RE", 2), (24, 3, 88, 24, False, "RE", 1), (24, 5, 96, 40, True, "HS", 2),
         (40, 5, 240, 40, True, "HS", 1), (40, 5, 240, 40, True, "HS", 1), (40, 5, 120, 48, True, "HS", 1), (48, 5, 144, 48, True, "HS", 1),
         (48, 5, 288, 96, True, "HS", 2), (96, 5, 576, 96, True, "HS", 1), (96, 5, 576, 96, True, "HS", 1))
EFFB0 = ((1, 3, 1, 32, 16, 1), (6, 3, 2, 16, 24, 2), (6, 5, 2, 24, 40, 2), (6, 3, 2, 40, 80, 3), (6, 5, 1, 80, 112, 3),
         (6, 5, 2, 112, 192, 4), (6, 3, 1, 192, 320, 1))


def mnv3s_features(store=False):
    bn = dict(eps=1e-3, momentum=0.01, store=store)
    return ([Conv2dNormActivation(3, 16, 3, 2, activation="hardswish", **bn)] + [InvertedResidual(*row, store=store) for row in MNV3S]
            + [Conv2dNormActivation(96, 576, 1, activation="hardswish", **bn)])


def effb0_features(stochastic_depth_prob=0.2, store=False):
    out, j, total = [Conv2dNormActivation(3, 32, 3, 2, activation="silu", store=store)], 0, sum(r[5] for r in EFFB0)
    for ratio, k, s, cin, cout, reps in EFFB0:
        stage = []
        for r in range(reps):
            stage.append(MBConv(ratio, k, s if r == 0 else 1, cin if r == 0 else cout, cout, stochastic_depth_prob * j / total, store))
            j += 1
        out.append(nn.Sequential(*stage))
    return out + [Conv2dNormActivation(320, 1280, 1, activation="silu", store=store)]


class _Row(nn.Module):
    def __init__(self, parts):
        super().__init__()
        self.model = nn.Sequential(*parts)

    def forward(self, x):
        return self.model(x)


def MobileNetV3s1(store=False):
    return _Row(mnv3s_features(store)[:4])


def MobileNetV3s2(store=False):
    return _Row(mnv3s_features(store)[4:9])


def MobileNetV3s3(store=False):
    return _Row(mnv3s_features(store)[9:])


def efficientnet_b01(stochastic_depth_prob=0.2, store=False):
    return _Row(effb0_features(stochastic_depth_prob, store)[:4])


def efficientnet_b02(stochastic_depth_prob=0.2, store=False):
    return _Row(effb0_features(stochastic_depth_prob, store)[4:6])


def efficientnet_b03(stochastic_depth_prob=0.2, store=False):
    return _Row(effb0_features(stochastic_depth_prob, store)[6:])
