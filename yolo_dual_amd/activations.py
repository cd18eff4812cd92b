"""The activation layers a ``Conv`` can carry, with the constructor signatures, parameter shapes and ``state_dict`` keys of the
reference's ``utils/activations.py``.

Inside a ``Conv`` none of these modules is *called*: ``modules._act_code`` maps the module to what the HIP path runs.

  * ``SiLU`` / ``Hardswish`` / ``Mish`` / ``MemoryEfficientMish`` (and ``nn.LeakyReLU(slope)``, ``nn.Hardswish``, ``nn.Mish``) are
    point-wise: they run inside the streaming BatchNorm kernels (``YDL_ACT_*`` of include/ydl.h), forward and backward, for every
    conv family.
  * ``AconC`` runs behind the materialised BatchNorm output through ``ydl_acon_fwd`` / ``ydl_acon_bwd`` (csrc/act.hip).
  * ``FReLU`` is a depth-wise 3x3 ``Conv`` without activation (``Tape.dw_bn_act``) merged with its input by ``ydl_max2_fwd`` /
    ``ydl_max2_bwd``.
  * ``MetaAconC`` holds its parameters, so a checkpoint that has one loads, but a ``Conv`` refuses it.

``forward`` of the parameter-free classes and of ``AconC`` is the plain torch formula for a stand-alone call on a tensor (the CPU
tests compare the kernels' float64 reference against it); ``FReLU`` called stand-alone runs its HIP path."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from .modules import Conv
from .tape import Tape, Var

__all__ = ["SiLU", "Hardswish", "Mish", "MemoryEfficientMish", "FReLU", "AconC", "MetaAconC"]


class SiLU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(x)


class Hardswish(nn.Module):
    def forward(self, x):
        return x * torch.clamp(x + 3.0, 0.0, 6.0) / 6.0


class Mish(nn.Module):
    def forward(self, x):
        return x * torch.tanh(F.softplus(x))


class MemoryEfficientMish(Mish):
    """the reference's variant differs from ``Mish`` only in what autograd saves; on the HIP path both are YDL_ACT_MISH, whose
    backward recomputes the BatchNorm output and saves nothing"""


class AconC(nn.Module):
    """(p1 - p2) x * sigmoid(beta (p1 - p2) x) + p2 x with per-channel p1, p2, beta of shape (1, c1, 1, 1)"""

    def __init__(self, c1: int):
        super().__init__()
        self.p1 = nn.Parameter(torch.randn(1, c1, 1, 1))
        self.p2 = nn.Parameter(torch.randn(1, c1, 1, 1))
        self.beta = nn.Parameter(torch.ones(1, c1, 1, 1))

    def forward(self, x):
        d = (self.p1 - self.p2) * x
        return d * torch.sigmoid(self.beta * d) + self.p2 * x

    def _apply_var(self, tape: Tape, z: Var, out=None) -> Var:
        if z.C != self.p1.shape[1]:
            raise RuntimeError(f"AconC({self.p1.shape[1]}) behind a Conv with {z.C} output channels")
        return tape.acon(z, self, out=out)


class MetaAconC(nn.Module):
    """AconC whose beta is generated per sample by two 1x1 convolutions over the global average.  Parameters only: a ``Conv``
    refuses it (``ydl_acon_fwd`` already reads beta through a per-sample stride; the generator network is not built)."""

    def __init__(self, c1: int, k: int = 1, s: int = 1, r: int = 16):
        super().__init__()
        c2 = max(r, c1 // r)
        self.p1 = nn.Parameter(torch.randn(1, c1, 1, 1))
        self.p2 = nn.Parameter(torch.randn(1, c1, 1, 1))
        self.fc1 = nn.Conv2d(c1, c2, k, s, bias=True)
        self.fc2 = nn.Conv2d(c2, c1, k, s, bias=True)

    def forward(self, x):
        raise NotImplementedError("MetaAconC is not implemented on the HIP path")


class FReLU(Conv):
    """max(x, bn(dwconv3x3(x))): ``conv.weight`` and ``bn.*`` are those of a depth-wise ``Conv(c1, c1, 3, 1, g=c1, act=False)``.
    The reference fixes the padding to 1, so only k = 3 keeps the size."""

    def __init__(self, c1: int, k: int = 3):
        if k != 3:
            raise NotImplementedError(f"FReLU: k={k} is not served (the reference pads by 1 whatever k is, only k=3 keeps the map size)")
        if c1 < 2:
            raise NotImplementedError("FReLU: c1 >= 2 (a depth-wise convolution over one channel is a dense one)")
        super().__init__(c1, c1, 3, 1, None, c1, act=False)

    def _fwd(self, tape: Tape, x: Var, out=None, **_kw) -> Var:
        return self._apply_var(tape, x, out=out)

    def _apply_var(self, tape: Tape, z: Var, out=None) -> Var:
        if z.C != self.c1:
            raise RuntimeError(f"FReLU({self.c1}) behind a Conv with {z.C} output channels")
        z = tape._flat(z)
        self.mark_step(tape)
        t = tape.dw_bn_act(z, self, 1, L.ACT_NONE)
        return tape.max2(z, t, out=out)
