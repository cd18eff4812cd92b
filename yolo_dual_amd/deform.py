"""Deformable convolution (``torchvision.ops.deform_conv2d``) on the HIP kernels, stand-alone autograd form.

Same signature as torchvision's functional op: ``deform_conv2d(input, offset, weight, bias=None, stride=1, padding=0,
dilation=1, mask=None)`` on NCHW tensors; ``offset`` holds (dy, dx) interleaved per kernel point and offset group.  The
op runs in column form (include/ydl.h, ydl_deform_gather): the gather kernel writes the modulated samples, the 1x1
implicit GEMM multiplies them by the KRSC weight (the bias rides along as one more weight column), and the backward kernel
turns d col into the input, offset and mask gradients.  Weight groups > 1 are not implemented.  grad_input is accumulated
with f32 atomics (not bitwise deterministic, like the DCNv3 op).  Inside a model, the same kernels run through
``Tape.deform_conv`` (yolo_dual_amd.modules.DeformConv2d)."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple, Union

import torch

from . import _lib as L
from .tape import _p, _stream, round_up

_Pair = Union[int, Tuple[int, int]]


def _pair(v: _Pair) -> Tuple[int, int]:
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return L.YDL_F32
    if t.dtype == torch.bfloat16:
        return L.YDL_BF16
    raise TypeError("deform_conv2d HIP kernels take float32 or bfloat16 tensors")


def _nhwc(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return t.detach().to(dtype).permute(0, 2, 3, 1).contiguous()


class DeformConv2dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias, stride, padding, dilation):
        if input.device.type != "cuda":
            raise RuntimeError("deform_conv2d: not implemented on the CPU (GPU only, no fallback)")
        dt, tdt = _dt(input), input.dtype
        N, C, H, W = input.shape
        Cout, Cw, kh, kw = weight.shape
        if Cw != C:
            raise NotImplementedError("deform_conv2d: weight groups > 1 are not implemented (every reference call site uses 1)")
        (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
        K = kh * kw
        Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
        Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
        G = offset.shape[1] // (2 * K)
        if G < 1 or offset.shape[1] != 2 * G * K or C % G != 0 or tuple(offset.shape[2:]) != (Ho, Wo) or offset.shape[0] != N:
            raise ValueError(f"offset must be (N, 2*G*{K}, {Ho}, {Wo}) with G dividing {C}, got {tuple(offset.shape)}")
        if mask is not None and tuple(mask.shape) != (N, G * K, Ho, Wo):
            raise ValueError(f"mask must be {(N, G * K, Ho, Wo)}, got {tuple(mask.shape)}")
        x = _nhwc(input, tdt)
        off = _nhwc(offset, tdt)
        msk = _nhwc(mask, tdt) if mask is not None else None
        kc = K * C + (1 if bias is not None else 0)
        ldc, cout_p = round_up(kc, 8), round_up(Cout, 8)
        npix = N * Ho * Wo
        dev = input.device
        st = _stream()
        col = torch.empty((npix, ldc), dtype=tdt, device=dev)
        L.call("ydl_deform_gather", dt, _p(x), C, _p(off), off.shape[-1], _p(msk), msk.shape[-1] if msk is not None else 0, 0,
               _p(col), ldc, int(bias is not None), N, H, W, C, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, G, st)
        master = weight.detach().float().permute(0, 2, 3, 1).reshape(Cout, K * C)
        if bias is not None:
            master = torch.cat([master, bias.detach().float().view(Cout, 1)], 1)
        master = master.contiguous()
        w = torch.empty((Cout, 1, ldc), dtype=tdt, device=dev)
        wt = torch.empty((kc, 1, cout_p), dtype=tdt, device=dev)
        L.call("ydl_weight_prep", dt, _p(master), _p(w), _p(wt), Cout, 1, kc, st)
        geom = L.ConvGeom(N, Ho, Wo, kc, Ho, Wo, Cout, 1, 1, 0, ldc, cout_p, 0)
        y = torch.empty((N, Ho, Wo, cout_p), dtype=tdt, device=dev)
        L.call("ydl_conv_fwd", ctypes.byref(geom), dt, _p(col), _p(w), _p(y), None, 0, st)
        ctx.save_for_backward(x, off, msk, col, wt)
        ctx.geom = (N, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, G, Ho, Wo, kc, ldc, cout_p)
        ctx.has_bias, ctx.has_mask = bias is not None, mask is not None
        ctx.dtypes = (input.dtype, offset.dtype, mask.dtype if mask is not None else None, weight.dtype)
        return y[..., :Cout].permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def backward(ctx, grad_out):
        x, off, msk, col, wt = ctx.saved_tensors
        N, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, G, Ho, Wo, kc, ldc, cout_p = ctx.geom
        dt, tdt = _dt(x), x.dtype
        dev = x.device
        st = _stream()
        K = kh * kw
        dy = torch.zeros((N, Ho, Wo, cout_p), dtype=tdt, device=dev)
        dy[..., :Cout] = grad_out.detach().to(tdt).permute(0, 2, 3, 1)
        geom = L.ConvGeom(N, Ho, Wo, kc, Ho, Wo, Cout, 1, 1, 0, ldc, cout_p, 0)
        dcol = torch.empty((N * Ho * Wo, ldc), dtype=tdt, device=dev)
        L.call("ydl_conv_dgrad", ctypes.byref(geom), dt, _p(dy), _p(wt), _p(dcol), 0, st)
        dw_ = torch.zeros((Cout, 1, ldc), dtype=torch.float32, device=dev)
        L.call("ydl_conv_wgrad", ctypes.byref(geom), dt, _p(col), _p(dy), _p(dw_), st)
        gin = torch.zeros((N, H, W, C), dtype=torch.float32, device=dev)
        goff = torch.empty((N, Ho, Wo, 2 * G * K), dtype=torch.float32, device=dev)
        gmsk = torch.empty((N, Ho, Wo, G * K), dtype=torch.float32, device=dev) if ctx.has_mask else None
        L.call("ydl_deform_bwd", dt, _p(x), C, _p(off), off.shape[-1], _p(msk), msk.shape[-1] if msk is not None else 0, 0,
               _p(dcol), ldc, _p(gin), _p(goff), _p(gmsk), N, H, W, C, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, G, st)
        tin, toff, tmsk, tw = ctx.dtypes
        dwk = dw_[:, 0, :K * C].reshape(Cout, kh, kw, C).permute(0, 3, 1, 2).to(tw)
        db = dw_[:, 0, K * C].to(tw) if ctx.has_bias else None
        return (gin.permute(0, 3, 1, 2).to(tin), goff.permute(0, 3, 1, 2).to(toff),
                gmsk.permute(0, 3, 1, 2).to(tmsk) if gmsk is not None else None, dwk, db, None, None, None)


def deform_conv2d(input: torch.Tensor, offset: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                  stride: _Pair = (1, 1), padding: _Pair = (0, 0), dilation: _Pair = (1, 1),
                  mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``torchvision.ops.deform_conv2d`` on the HIP kernels (float32 or bfloat16 tensors on the GPU)"""
    return DeformConv2dFunction.apply(input, offset, mask, weight, bias, _pair(stride), _pair(padding), _pair(dilation))
