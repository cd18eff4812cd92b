"""Closed form of dense multi-head self-attention (the core of TransformerLayer, models/common.py:79-93: nn.MultiheadAttention without
mask or dropout) and of its gradients, written out by hand in plain torch, in whatever dtype its inputs have (float64 in the tests).

Tokens are rows: q, k, v are (N, S, C); head h is the channel block [h*d, (h+1)*d), d = C // heads.  Per (sample, head):

    s_ij = scale * q_i . k_j        P = softmax_j(s)        out_i = sum_j P_ij v_j        lse_i = log sum_j exp(s_ij)

    dV = P^T dO       dP = dO V^T       dS = P * (dP - rowsum(dO * out))       dQ = scale * dS K       dK = scale * dS^T Q

The layer compositions below restate TransformerLayer / TransformerBlock / C3TR on top of it, with the reference's parameter names."""
import torch
import torch.nn.functional as F


def _heads(t, heads):
    N, S, C = t.shape
    return t.reshape(N, S, heads, C // heads).permute(0, 2, 1, 3)          # (N, heads, S, d)


def _rows(t):
    N, h, S, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(N, S, h * d)


def mha(q, k, v, heads, scale):
    """-> out (N, S, C), lse (N, heads, S)"""
    qh, kh, vh = _heads(q, heads), _heads(k, heads), _heads(v, heads)
    s = scale * (qh @ kh.transpose(-1, -2))
    mx = s.max(-1, keepdim=True).values
    e = torch.exp(s - mx)
    den = e.sum(-1, keepdim=True)
    return _rows((e / den) @ vh), (mx + torch.log(den)).squeeze(-1)


def mha_grad(q, k, v, dout, heads, scale):
    """-> dq, dk, dv (N, S, C), by the closed form above (no autograd)"""
    qh, kh, vh, doh = _heads(q, heads), _heads(k, heads), _heads(v, heads), _heads(dout, heads)
    s = scale * (qh @ kh.transpose(-1, -2))
    P = torch.softmax(s, -1)
    out = P @ vh
    dv = P.transpose(-1, -2) @ doh
    dP = doh @ vh.transpose(-1, -2)
    dS = P * (dP - (doh * out).sum(-1, keepdim=True))
    return _rows(scale * (dS @ kh)), _rows(scale * (dS.transpose(-1, -2) @ qh)), _rows(dv)


# ---------------------------------------------------------------------------------------------------------------------
# the layers, on (N, S, C) token rows; p: parameters under the reference's names, pre: the prefix of this module's names
# ---------------------------------------------------------------------------------------------------------------------
def transformer_layer(x, p, pre, heads):
    C = x.shape[-1]
    w, b = p[pre + "ma.in_proj_weight"], p[pre + "ma.in_proj_bias"]
    q = F.linear(F.linear(x, p[pre + "q.weight"]), w[:C], b[:C])
    k = F.linear(F.linear(x, p[pre + "k.weight"]), w[C:2 * C], b[C:2 * C])
    v = F.linear(F.linear(x, p[pre + "v.weight"]), w[2 * C:], b[2 * C:])
    a, _ = mha(q, k, v, heads, (C // heads) ** -0.5)
    x = F.linear(a, p[pre + "ma.out_proj.weight"], p[pre + "ma.out_proj.bias"]) + x
    return F.linear(F.linear(x, p[pre + "fc1.weight"]), p[pre + "fc2.weight"]) + x


def conv_bn_silu(x, p, pre, eps=1e-5):
    """Conv (models/common.py:47-58) with a 1x1 kernel in train mode, on (N, C, H, W)"""
    w = p[pre + "conv.weight"]
    y = F.conv2d(x, w, padding=w.shape[-1] // 2)
    y = F.batch_norm(y, None, None, p[pre + "bn.weight"], p[pre + "bn.bias"], True, 0.0, eps)
    return F.silu(y)


def transformer_block(x, p, pre, heads, layers):
    """x: (N, C1, H, W) -> (N, C2, H, W)"""
    if pre + "conv.conv.weight" in p:
        x = conv_bn_silu(x, p, pre + "conv.")
    N, C, H, W = x.shape
    t = x.flatten(2).permute(0, 2, 1)                       # token rows: one sample's H*W pixels
    t = t + F.linear(t, p[pre + "linear.weight"], p[pre + "linear.bias"])
    for i in range(layers):
        t = transformer_layer(t, p, f"{pre}tr.{i}.", heads)
    return t.permute(0, 2, 1).reshape(N, C, H, W)


def c3tr(x, p, pre, n):
    y1 = transformer_block(conv_bn_silu(x, p, pre + "cv1."), p, pre + "m.", 4, n)
    y2 = conv_bn_silu(x, p, pre + "cv2.")
    return conv_bn_silu(torch.cat((y1, y2), 1), p, pre + "cv3.")
