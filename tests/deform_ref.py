"""Pure-torch restatement of torchvision.ops.deform_conv2d (NCHW, any dtype; the tests run it in f64).

y = ho*s - p + i*d + offset[2(g*K + k)], x = wo*s - p + j*d + offset[2(g*K + k) + 1] (k = i*kw + j, (dy, dx) interleaved);
value = bilinear over the four corners, each corner outside the image counted as 0 (validity per corner only, the convention of
yolo_dual_amd/csrc/deform.hip), times mask[g*K + k]; out[co] = bias[co] + sum_{c,k} weight[co, c, i, j] * value.
Differentiable through autograd in every argument."""
import torch


def deform_conv2d_ref(x, offset, weight, bias=None, stride=1, padding=0, dilation=1, mask=None):
    s = (stride, stride) if isinstance(stride, int) else tuple(stride)
    p = (padding, padding) if isinstance(padding, int) else tuple(padding)
    d = (dilation, dilation) if isinstance(dilation, int) else tuple(dilation)
    N, C, H, W = x.shape
    Cout, _, kh, kw = weight.shape
    K = kh * kw
    Ho = (H + 2 * p[0] - (d[0] * (kh - 1) + 1)) // s[0] + 1
    Wo = (W + 2 * p[1] - (d[1] * (kw - 1) + 1)) // s[1] + 1
    G = offset.shape[1] // (2 * K)
    Cg = C // G
    ho = torch.arange(Ho, dtype=x.dtype).view(Ho, 1)
    wo = torch.arange(Wo, dtype=x.dtype).view(1, Wo)
    xf = x.reshape(N, C, H * W)
    cols = []                                                    # [N, C, K, Ho, Wo]
    for g in range(G):
        xg = xf[:, g * Cg:(g + 1) * Cg]
        taps = []
        for k in range(K):
            i, j = divmod(k, kw)
            y = ho * s[0] - p[0] + i * d[0] + offset[:, 2 * (g * K + k)]
            xx = wo * s[1] - p[1] + j * d[1] + offset[:, 2 * (g * K + k) + 1]
            y0, x0 = torch.floor(y.detach()), torch.floor(xx.detach())
            ly, lx = y - y0, xx - x0
            val = 0
            for dy_, dx_, wgt in ((0, 0, (1 - ly) * (1 - lx)), (0, 1, (1 - ly) * lx), (1, 0, ly * (1 - lx)), (1, 1, ly * lx)):
                yy, xc = y0 + dy_, x0 + dx_
                ok = (yy >= 0) & (yy < H) & (xc >= 0) & (xc < W)
                idx = (yy.clamp(0, H - 1) * W + xc.clamp(0, W - 1)).long().view(N, 1, Ho * Wo).expand(N, Cg, Ho * Wo)
                v = torch.gather(xg, 2, idx).view(N, Cg, Ho, Wo)
                val = val + v * (wgt * ok.to(x.dtype)).unsqueeze(1)
            if mask is not None:
                val = val * mask[:, g * K + k].unsqueeze(1)
            taps.append(val)
        cols.append(torch.stack(taps, 2))
    col = torch.cat(cols, 1)                                     # [N, C, K, Ho, Wo]
    out = torch.einsum("nckhw,ock->nohw", col, weight.reshape(Cout, C, K))
    if bias is not None:
        out = out + bias.view(1, Cout, 1, 1)
    return out
