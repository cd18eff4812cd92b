"""Restatement of the local self-attention of AttentionConv / AttentionStem (models/common.py:1509-1627) in plain torch, closed
form, in whatever dtype its inputs have (float64 in the tests; the bench runs it in the compute dtype as the baseline).

Per sample n, channel c and pixel (h, w), independently, over the taps t = i*ks + j reading position (h + i - p, w + j - p), p = ks // 2
(K and V count as 0 outside the image, the tap stays in the softmax):

    logit_t = Q[c] * (K_t[c] + r[c, t])        r[c, (i, j)] = rel_h[c, i] for c < C/2, rel_w[c - C/2, j] otherwise   (None: 0)
    P       = softmax over the ks*ks taps
    out[c]  = sum_t P_t * sum_m E[m, t] * V^m_t[c]                                                               (None: E = 1)

``groups`` of the reference only reshapes; it has no arithmetic effect.  Gradients come from autograd on this composition."""
import torch
import torch.nn.functional as F


def _taps(t: torch.Tensor, ks: int) -> torch.Tensor:
    """(N, C, H, W) -> (N, C, H, W, ks*ks): tap i*ks + j holds t at (h + i - p, w + j - p), zero outside"""
    p = ks // 2
    H, W = t.shape[-2:]
    tp = F.pad(t, [p, p, p, p])
    return torch.stack([tp[..., i:i + H, j:j + W] for i in range(ks) for j in range(ks)], dim=-1)


def stem_table(emb_mix: torch.Tensor, emb_a: torch.Tensor, emb_b: torch.Tensor) -> torch.Tensor:
    """E[m, i*ks + j] = softmax over m of (emb_mix @ emb_a)[m, i] + (emb_mix @ emb_b)[m, j]"""
    la, lb = emb_mix @ emb_a, emb_mix @ emb_b
    return torch.softmax((la[:, :, None] + lb[:, None, :]).reshape(la.shape[0], -1), dim=0)


def local_attention(q, k, vs, ks, rel_h=None, rel_w=None, emb=None):
    """q, k: (N, C, H, W); vs: the m value tensors; rel_h / rel_w: (C/2, ks); emb: (m, ks*ks)"""
    C = q.shape[1]
    kt = _taps(k, ks)
    if rel_h is not None:
        r = torch.cat([rel_h.reshape(C // 2, ks, 1).expand(-1, -1, ks), rel_w.reshape(C // 2, 1, ks).expand(-1, ks, -1)], 0)
        kt = kt + r.reshape(1, C, 1, 1, ks * ks)
    P = torch.softmax(q.unsqueeze(-1) * kt, dim=-1)
    u = 0
    for m, v in enumerate(vs):
        vt = _taps(v, ks)
        u = u + (vt if emb is None else vt * emb[m])
    return (P * u).sum(-1)


def _proj(x, w):
    return F.conv2d(x, w.reshape(w.shape[0], w.shape[1], 1, 1))


def attention_conv(x, p: dict, ks: int):
    """p: the module's parameters under the reference's names"""
    q, k, v = _proj(x, p["query_conv.weight"]), _proj(x, p["key_conv.weight"]), _proj(x, p["value_conv.weight"])
    C = q.shape[1]
    return local_attention(q, k, [v], ks, p["rel_h"].reshape(C // 2, ks), p["rel_w"].reshape(C // 2, ks))


def attention_stem(x, p: dict, ks: int, m: int):
    q, k = _proj(x, p["query_conv.weight"]), _proj(x, p["key_conv.weight"])
    vs = [_proj(x, p[f"value_conv.{i}.weight"]) for i in range(m)]
    return local_attention(q, k, vs, ks, emb=stem_table(p["emb_mix"], p["emb_a"], p["emb_b"]))
