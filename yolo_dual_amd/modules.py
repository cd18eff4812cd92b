"""nn.Module facade with the reference's names, constructor signatures and state_dict layout; all compute runs
through yolo_dual_amd.tape on the HIP kernels.

Both spellings of each block are served:
  * seg-script blocks  — unet-lite/yolo5-seg/seg_diceloss_yolov5.py:388-507, yolov8/seg_jaccardloss_yolov8.py:401-414,
    unet-lite/yolo9-seg/seg_diceloss_yolov9.py:451-510, segment/train.py:50-210
  * stock YOLOv5 blocks — models/common.py:38-64 (Conv), :115-125 (Bottleneck), :161-172 (C3), :223-238 (SPPF),
    :310-317 (Concat)
Every module accepts either a tape ``Var`` (inside a model: one taped region for the whole network) or plain
(N,C,H,W) f32 tensors (stand-alone use: the call becomes its own taped region behind one autograd node).
"""
from __future__ import annotations

import ctypes

import math
from typing import List, Optional, Sequence, Union

import torch
import torch.nn as nn

from . import _lib as L
from . import config
from .tape import Tape, Var, round_up, _p, _stream, zero_

__all__ = ["autopad", "Conv", "C3", "C3Common", "Bottleneck", "C2f", "C3k2", "GAM", "SPPF", "Concat", "Upsample",
           "BasicBlock", "BottleneckBlock", "SegmentHead", "run_region", "Linear", "DCNv3", "DCNV3_YoLo", "Bottleneck_DCNV3",
           "C3_DCNV3", "DeformConv2d", "C3_DCN", "C2f_DCN", "DCNv2",
           "Bottleneck_DCN", "C3_DCNCommon", "AttentionConv", "AttentionStem", "DWConv", "GhostConv", "GhostBottleneck", "C3Ghost",
           "BasicConv", "RFB", "ASPP", "CrossConv", "C3x", "ConvTranspose2d", "DWConvTranspose2d",
           "Focus", "Contract", "Expand", "BottleneckCSP", "BatchNorm2d"]


def autopad(k, p=None, d=1):
    """models/common.py:38-44 / seg_diceloss_yolov5.py:381-385."""
    if d > 1:
        k = d * (k - 1) + 1 if isinstance(k, int) else [d * (x - 1) + 1 for x in k]
    if p is None:
        p = k // 2 if isinstance(k, int) else [x // 2 for x in k]
    return p


# ----------------------------------------------------------------------------------------------------------
# taped region behind ONE torch.autograd node
# ----------------------------------------------------------------------------------------------------------
class _Region(torch.autograd.Function):
    """forward(fn, n_in, *tensors): tensors = n_in external inputs followed by the parameters the region may touch
    (they are inputs only so that autograd schedules this node; their gradients are written into ``p.grad`` by the
    kernels and ``None`` is returned for them)."""

    @staticmethod
    def forward(ctx, fn, n_in, *tensors):
        ins = tensors[:n_in]
        dev = ins[0].device
        if dev.type != "cuda":
            raise RuntimeError("yolo_dual_amd runs on the GPU only: there is no CPU fallback for the HIP kernels "
                               "(move the module and its inputs to cuda)")
        record = any(ctx.needs_input_grad[2:])
        tape = Tape(config.compute_dtype(), dev, fn.training, record)
        tape._slab_hint = getattr(fn, "_ydl_slab_need", 0)
        refresh_weights(fn, tape)
        vs = [tape.input_nchw(t, lazy=not ctx.needs_input_grad[2 + i]) for i, t in enumerate(ins)]
        for i, v in enumerate(vs):
            v.need = bool(ctx.needs_input_grad[2 + i])
        res = fn._fwd(tape, vs if fn.takes_list else vs[0]) if n_in else None
        if isinstance(res, torch.Tensor):           # region already produced its external output (softmax head)
            out_t, out_v = res, None
        else:
            out_v = tape.materialize(res)           # a lazily up-sampled result becomes real at the region edge
            out_t = tape.export_nchw(out_v)
        ctx.tape, ctx.vs, ctx.out_v, ctx.fn = tape, vs, out_v, fn
        ctx.n_extra = len(tensors) - n_in
        return out_t

    @staticmethod
    def backward(ctx, gout):
        tape: Tape = ctx.tape
        if tape is None:
            raise RuntimeError("second backward through a taped region: its activations were released by the first one "
                               "(retain_graph is not supported; run the forward again)")
        if ctx.out_v is not None:
            tape.seed_grad_nchw(ctx.out_v, gout)
        else:
            ctx.fn._seed_external(tape, gout)
        tape.run_backward()
        gins = [tape.grad_nchw(v) if v.need else None for v in ctx.vs]
        if tape._slab_total:
            ctx.fn._ydl_slab_need = tape._slab_total + tape._slab_total // 8 + 1024      # next step: one slab, one memset
        ctx.tape = None
        return (None, None, *gins, *([None] * ctx.n_extra))


def refresh_weights(fn: nn.Module, tape: Tape) -> None:
    """one batched launch re-deriving the compute-layout weights of every stale Conv under ``fn``"""
    convs = getattr(fn, "_ydl_convs", None)
    if convs is None:
        convs = [m for m in fn.modules() if isinstance(m, Conv) and not m.depthwise and not m.grouped and not m.cross and m.d == 1 and m.bn is not None]     # (a dilated Conv's GEMM view is _DeformGemm; a grouped Conv prepares its own block-diagonal copies)
        fn._ydl_convs = convs
        fn._ydl_csp = [m for m in fn.modules() if isinstance(getattr(m, "cv1", None), Conv) and isinstance(getattr(m, "cv2", None), Conv)]
    # sibling pairs that ran fused last time are prepared as ONE matrix (their masters are adjacent), their members not at all
    pairs = [b._pair for b in fn._ydl_csp
             if getattr(b, "_pair", None) is not None and b._pair._wcache.get("key") is not None and b._pair.still_valid()]
    if pairs:
        members = {id(m) for pr in pairs for m in (pr.a, pr.b)}
        units = [m for m in convs if id(m) not in members] + pairs
    else:
        units = convs
    stale = [m for m in units if m._wcache.get("key") != m._wkey(tape)]
    if len(stale) < 2:
        return
    rows, keep = [], []
    for m in stale:
        master = m._master_krsc()
        w, wt = m._wbuffers(tape, master)
        keep.append(master)
        rows.append([master.data_ptr(), w.data_ptr(), wt.data_ptr(), m.c2, m.k * m.k, m.c1, 0, 0])
    sig = tuple(r[0] for r in rows) + tuple(r[1] for r in rows) + (tape.dname,)
    cache = getattr(fn, "_ydl_wdesc", None)
    if cache is None or cache[0] != sig:
        desc = torch.tensor(rows, dtype=torch.int64).to(tape.device)
        fn._ydl_wdesc = (sig, desc)
    desc = fn._ydl_wdesc[1]
    L.call("ydl_weight_prep_batched", tape.dt, _p(desc), len(rows), _stream())
    for m in stale:
        m._wcache["key"] = m._wkey(tape)


def run_region(fn: nn.Module, inputs: Sequence[torch.Tensor]) -> torch.Tensor:
    if torch.is_grad_enabled():
        allp = getattr(fn, "_ydl_params", None)          # walking the module tree costs ~0.5 ms per call on this model
        if allp is None or allp[0] != len(fn._parameters) + sum(1 for _ in fn.children()):
            allp = fn._ydl_params = (len(fn._parameters) + sum(1 for _ in fn.children()), list(fn.parameters()))
        params = [p for p in allp[1] if p.requires_grad]
    else:
        params = []
    out = _Region.apply(fn, len(inputs), *inputs, *params)
    lazy = getattr(getattr(out.grad_fn, "tape", None), "lazy_out", None)
    if lazy is not None:                # replicated output: let SegmentationLoss work at the stored resolution
        lazy.version = out._version
        out._ydl_lazy = lazy
    return out


class YdlModule(nn.Module):
    """base: dispatch between taped (Var) and stand-alone (torch.Tensor) calls"""
    takes_list = False

    def forward(self, x, *a, **kw):
        if isinstance(x, Var):
            return self._fwd(x.tape, x)
        if isinstance(x, (list, tuple)) and x and isinstance(x[0], Var):
            return self._fwd(x[0].tape, x)
        xs = list(x) if isinstance(x, (list, tuple)) else [x]
        return run_region(self, xs)

    def _fwd(self, tape: Tape, x):
        raise NotImplementedError

    def _seed_external(self, tape: Tape, gout: torch.Tensor) -> None:
        raise NotImplementedError


# ----------------------------------------------------------------------------------------------------------
# Conv = Conv2d(bias=False) -> BatchNorm2d -> SiLU
# ----------------------------------------------------------------------------------------------------------
def _launch_wgrad(tape: Tape, gp, x_ptr, dy_ptr, dw_ptr, st, fuse=None) -> bool:
    """dW += dy^T * im2col(x): f32 atomics (throughput mode) or the deterministic slab form (parity mode / config).
    ``fuse`` = (wt_ptr, dx_ptr, lddx, accumulate) of the SAME layer's input gradient: where the one-pass kernel applies (the
    HBM-bound 128 -> 128 1x1 layers, ydl_conv_bwd_pw) both gradients come from one launch and the call returns True.  A fifth
    element holds ydl_conv_bwd_pw_bn's arguments between ``x`` and ``wt``: dy does not exist then (``dy_ptr`` is None), the kernel
    forms it from the BatchNorm backward's operands, and there is no other way to run the layer."""
    if (fuse is not None and not config.deterministic(tape.dname) and config.fuse_pw_backward()
            and L.lib().ydl_conv_bwd_pw_supported(gp, tape.dt)):
        wt_ptr, dx_ptr, lddx, acc = fuse[:4]
        if len(fuse) > 4:
            L.call("ydl_conv_bwd_pw_bn", gp, tape.dt, x_ptr, *fuse[4], wt_ptr, dx_ptr, lddx, acc, dw_ptr, st)
        else:
            L.call("ydl_conv_bwd_pw", gp, tape.dt, x_ptr, dy_ptr, wt_ptr, dx_ptr, lddx, acc, dw_ptr, st)
        return True
    if dy_ptr is None:
        raise RuntimeError("ydl_conv_bwd_pw_bn was planned for a layer the one-pass kernel does not take")
    if config.deterministic(tape.dname):
        nbytes = L.lib().ydl_conv_wgrad_ws_bytes(gp, tape.dt)
        ws = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=tape.device)
        L.call("ydl_conv_wgrad_det", gp, tape.dt, x_ptr, dy_ptr, dw_ptr, _p(ws), st)
        tape._keep.append(ws)          # may be consumed on the side stream: lives until the streams are joined
    else:
        L.call("ydl_conv_wgrad", gp, tape.dt, x_ptr, dy_ptr, dw_ptr, st)
    return False


class _GemmWeights:
    """What the tape needs from the holder of an implicit-GEMM weight, once: the compute-layout copies of the f32 master, the padded
    bias row, the gradient storage and the weight-gradient launch.  The master is seen as a contiguous [rows][taps][cin] f32 array
    (KRSC: an OIHW parameter in channels_last storage, or a [rows, cin] matrix).  A holder supplies

      ``_wparam``       the weight parameter (default ``self.weight``; ``self.bias`` is the bias parameter or None)
      ``_gemm_dims()``  (rows, taps, cin)
      ``_rows``         None, or the slice of the parameters' rows this holder stands for (one Q / K / V block of ``in_proj_weight``)
      ``final``         this holder's backward is the last launch writing its parameters' gradients, so only it reports them to
                        ``config.mark_touched`` (the data-parallel hook may start the all-reduce from there)
      ``_place_grad``   None, or a method that adds a padded gradient into a gradient torch laid out some other way (cold path)

    Holders with a BatchNorm ``self.bn`` behind the GEMM (Conv, _FusedPair, _DeformGemm) also get its coefficient and gradient rows."""
    _rows = None
    final = True
    _place_grad = None
    _wname = "Conv2d"
    k, s, p = 1, 1, 0

    @property
    def _wparam(self) -> nn.Parameter:
        return self.weight

    def _krsc(self, t: torch.Tensor) -> torch.Tensor:
        """[rows][taps][cin] view of the weight or of its gradient (no copy)"""
        if t.dim() == 4:
            return t.permute(0, 2, 3, 1)
        return t if self._rows is None else t[self._rows]

    def _master_krsc(self) -> torch.Tensor:
        p = self._wparam
        w = self._krsc(p.detach())
        if not w.is_contiguous():
            if p.dim() == 4:                           # someone re-assigned .data in OIHW order: re-home it
                p.data = p.data.contiguous(memory_format=torch.channels_last)
                w = self._krsc(p.detach())
            if not w.is_contiguous():
                w = w.contiguous()
        return w

    def _wkey(self, tape: Tape):
        wp = self._wparam
        return (tape.dname, wp.data_ptr(), wp._version, config.weight_epoch())

    def _wbuffers(self, tape: Tape, master: torch.Tensor):
        rows, taps, cin = self._gemm_dims()
        dev = master.device
        w = self._wcache.get("w")
        if w is None or self._wcache.get("dname") != tape.dname or w.device != dev:
            w = torch.empty((rows, taps, round_up(cin, 8)), dtype=tape.tdt, device=dev)
            wt = torch.empty((cin, taps, round_up(rows, 8)), dtype=tape.tdt, device=dev)
            self._wcache.update(w=w, wt=wt, dname=tape.dname, key=None)
        return self._wcache["w"], self._wcache["wt"]

    def compute_weights(self, tape: Tape):
        """compute-dtype copies w [rows][taps][cin_p] / wt [cin][taps][rows_p] of the f32 master weight, refreshed when the
        parameter changed (torch version counter, or the epoch the fused optimizer bumps)"""
        key = self._wkey(tape)
        if self._wcache.get("key") == key:
            return self._wcache["w"], self._wcache["wt"]
        master = self._master_krsc()
        w, wt = self._wbuffers(tape, master)
        L.call("ydl_weight_prep", tape.dt, _p(master), _p(w), _p(wt), *self._gemm_dims(), _stream())
        self._wcache["key"] = key
        return w, wt

    def bias_coeffs(self, device):
        """(ones, bias) padded to a multiple of 8 channels for ydl_bn_act_fwd (scale = 1, shift = bias)"""
        rows = self._bias_len()
        cp = round_up(rows, 8)
        key = (self.bias.data_ptr(), self.bias._version, config.weight_epoch())
        c = self._wcache
        if c.get("ones") is None or c["ones"].device != device:       # created once (a refresh below only rewrites bpad's contents)
            c["ones"] = torch.ones(cp, dtype=torch.float32, device=device)
            c["bpad"] = torch.zeros(cp, dtype=torch.float32, device=device)
            c["bkey"] = None
        if c.get("bkey") != key:
            L.call("ydl_copy2d", L.YDL_F32, _p(self._krsc(self.bias.detach())), rows, _p(c["bpad"]), cp, 1, rows, 0, _stream())
            c["bkey"] = key
        return c["ones"], c["bpad"]

    def _bias_len(self) -> int:
        """length of the bias row: the GEMM's rows, except where the GEMM runs mirrored (ConvTranspose2d)"""
        return self._gemm_dims()[0]

    def _grad_of(self, p: nn.Parameter) -> torch.Tensor:
        """(this holder's rows of) the parameter's gradient"""
        if p.grad is None:
            p.grad = torch.zeros_like(p)       # preserves the KRSC (channels_last) strides of a convolution weight
        return p.grad if self._rows is None else p.grad[self._rows]

    def wgrad(self, tape: Tape, gp, x: Var, dy: Var, st, col0: int = 0, final: bool = True, fuse=None) -> bool:
        """``col0``: first input channel of the block this call covers (gp.ldw = total padded Cin then); ``final``: the
        last launch writing this parameter's gradient (only then may the data-parallel hook see it); ``fuse``: see
        ``_launch_wgrad`` — returns True when the input gradient was produced by the same launch"""
        p = self._wparam
        if not p.requires_grad:                    # frozen: no gradient kernel, never marked touched
            return False
        rows, taps, cin = self._gemm_dims()
        self._grad_of(p)                           # allocates on first use
        gk = self._krsc(p.grad)
        if not gk.is_contiguous() and self._place_grad is None:
            raise RuntimeError(f"{self._wname} weight gradient must be KRSC-contiguous")
        cin_p = round_up(cin, 8)
        done = False
        if cin_p == cin and gk.is_contiguous():
            done = _launch_wgrad(tape, gp, _p(x.t), _p(dy.t) if dy is not None else None, ctypes.c_void_p(gk.data_ptr() + 4 * col0), st, fuse)
        else:
            assert col0 == 0 and final
            tmp = zero_(torch.empty((rows, taps, cin_p), dtype=torch.float32, device=gk.device), st)
            _launch_wgrad(tape, gp, _p(x.t), _p(dy.t), _p(tmp), st)
            if gk.is_contiguous():
                L.call("ydl_wgrad_unpad", _p(tmp), _p(gk), rows, taps, cin, 1, st)
            else:
                self._place_grad(p.grad, tmp)
        if final and self.final:
            config.mark_touched(p)
        return done

    def pw_bn_ready(self) -> bool:
        """``wgrad`` would hand ``fuse`` to the kernel as it is (no padded staging buffer, no re-homed gradient): the condition
        under which the tape may leave dy to ydl_conv_bwd_pw_bn"""
        p = self._wparam
        rows, taps, cin = self._gemm_dims()
        return bool(p.requires_grad and cin % 8 == 0 and self._krsc(self._grad_of(p)).is_contiguous())

    # -- the BatchNorm behind the GEMM ---------------------------------------------------------------------
    def mark_step(self, tape: Tape) -> None:
        if tape.train:
            self.bn._nbt_pending += 1

    def coeffs(self, device):
        cp = round_up(self._gemm_dims()[0], 8)
        buf = torch.empty((4, cp), dtype=torch.float32, device=device)
        if cp != self._gemm_dims()[0]:
            zero_(buf)
        return {"mean": buf[0], "invstd": buf[1], "scale": buf[2], "shift": buf[3]}

    def grad_slot(self, tape: Tape, which: str):
        """gradient storage of gamma / beta; ``touch_bn`` must be called AFTER the kernel writing it is enqueued (the
        data-parallel hook may launch the bucket's all-reduce from inside mark_touched)"""
        p = self.bn.weight if which == "gamma" else self.bn.bias
        return self._grad_of(p), 1

    def touch_bn(self) -> None:
        if self.bn.weight.requires_grad:
            config.mark_touched(self.bn.weight)
        if self.bn.bias.requires_grad:
            config.mark_touched(self.bn.bias)


class _BNHolder(nn.BatchNorm2d):
    """Parameter/buffer holder with nn.BatchNorm2d's state_dict layout.  ``num_batches_tracked`` is advanced on the
    host and flushed into the buffer whenever the state is read, so the hot loop launches no extra kernel."""

    def __init__(self, c):
        super().__init__(c)
        self._nbt_pending = 0
        self.register_state_dict_pre_hook(_BNHolder._flush_hook)

    @staticmethod
    def _flush_hook(module, prefix, keep_vars):
        module.flush()

    def flush(self):
        if self._nbt_pending:
            self.num_batches_tracked += self._nbt_pending
            self._nbt_pending = 0

    def forward(self, x):  # pragma: no cover - never used: BN is fused into the conv epilogue + apply kernels
        raise RuntimeError("BatchNorm is fused into yolo_dual_amd.Conv; call the Conv module")


def _act_code(act) -> int:
    """the activation of a Conv as the code the tape carries: a YDL_ACT_* code of the streaming BatchNorm kernels (LeakyReLU as an
    ``ActCode`` that holds its slope), or ACT_ACON / ACT_FRELU for the two layers that run behind an ACT_NONE Conv.  Matched by type."""
    from . import activations as A
    if act is True or isinstance(act, (nn.SiLU, A.SiLU)):
        return L.ACT_SILU
    if act is False or act is None or isinstance(act, nn.Identity):
        return L.ACT_NONE
    if isinstance(act, nn.ReLU):
        return L.ACT_RELU
    if isinstance(act, nn.LeakyReLU):
        slope = float(act.negative_slope)
        if not 0.0 <= slope < 1.0:
            raise NotImplementedError(f"activation {act!r}: the HIP path serves LeakyReLU slopes 0 <= negative_slope < 1")
        return L.ActCode(L.ACT_LEAKY, slope)
    if isinstance(act, (nn.Hardswish, A.Hardswish)):
        return L.ACT_HSWISH
    if isinstance(act, (nn.Mish, A.Mish)):
        return L.ACT_MISH
    if isinstance(act, A.AconC):
        return L.ACT_ACON
    if isinstance(act, A.FReLU):
        return L.ACT_FRELU
    if isinstance(act, A.MetaAconC):
        raise NotImplementedError("activation MetaAconC is not implemented on the HIP path (AconC is: its beta is a parameter)")
    raise NotImplementedError(f"activation {act!r} is not supported by the HIP path (SiLU/ReLU/Identity)")


def _pointwise_act_code(act, who: str) -> int:
    code = _act_code(act)
    if code in (L.ACT_ACON, L.ACT_FRELU):
        raise NotImplementedError(f"{who}: the default activation {act!r} is not point-wise; {who} serves the point-wise activations only")
    return code


def _cross_args(c1, c2, k, s, p, g, d):
    """Conv with a tuple kernel or stride.  Equal entries mean the int: -> (k, s, p, None).  A kernel (1, k) / (k, 1) with stride
    (1, s) / (s, 1) (or the int 1) is a cross convolution along W / H: -> (k, s, p, axis) with the axis's own k, s, p.  Everything else
    is refused: the served set is ydl_xconv_supported's."""
    def pair(v, what):
        if isinstance(v, (tuple, list)):
            if len(v) != 2 or not all(isinstance(e, int) and not isinstance(e, bool) for e in v):
                raise TypeError(f"Conv: {what}={v!r} must be an int or a pair of ints")
            return tuple(v)
        if not isinstance(v, int) or isinstance(v, bool):
            raise TypeError(f"Conv: {what}={v!r} must be an int or a pair of ints")
        return None
    kt, st = pair(k, "k"), pair(s, "s")
    got = f"got c1={c1}, c2={c2}, k={k}, s={s}, p={p}, g={g}, d={d}"
    rule = ("cross convolution: the HIP path serves k = (1, k) with s = (1, s) and k = (k, 1) with s = (s, 1) (or the int s = 1), k odd in "
            "3..9, s in {1, 2}, p = None or autopad(k), g = 1, d = 1, c1 and c2 multiples of 8; ")
    if kt is None:
        kt = (k, k)
    if kt[0] == kt[1]:                         # a square kernel written as a pair
        if st is not None and st[0] != st[1]:
            raise NotImplementedError(rule + "a rectangular stride needs a cross kernel; " + got)
        if isinstance(p, (tuple, list)):
            if len(p) != 2 or p[0] != p[1]:
                raise NotImplementedError(rule + "a rectangular padding needs a cross kernel; " + got)
            p = p[0]
        return kt[0], (s if st is None else st[0]), p, None
    if kt[0] != 1 and kt[1] != 1:
        raise NotImplementedError(rule + "general (kh, kw) kernels with both entries > 1 are not implemented; " + got)
    axis = L.AXIS_W if kt[0] == 1 else L.AXIS_H
    kk = kt[1] if axis == L.AXIS_W else kt[0]
    if st is None:
        if s != 1:
            raise NotImplementedError(rule + "an int stride with a cross kernel must be 1; " + got)
        sv = 1
    else:
        sv, other = (st[1], st[0]) if axis == L.AXIS_W else (st[0], st[1])
        if other != 1:
            raise NotImplementedError(rule + "the stride lies along the wrong axis; " + got)
    want = [0, kk // 2] if axis == L.AXIS_W else [kk // 2, 0]
    if not (p is None or (isinstance(p, (tuple, list)) and list(p) == want)):
        raise NotImplementedError(rule + got)
    if g != 1 or d != 1 or c1 % 8 or c2 % 8 or kk % 2 == 0 or not 3 <= kk <= 9 or sv not in (1, 2):
        raise NotImplementedError(rule + got)
    return kk, sv, None, axis


class Conv(_GemmWeights, YdlModule):
    """``Conv(c1, c2, k=1, s=1, p=None, g=1, act=True)`` (seg scripts) and
    ``Conv(c1, c2, k=1, s=1, p=None, g=1, d=1, act=True)`` (models/common.py): the 7th positional argument is taken
    as ``act`` when it is a bool/Module and as the dilation when it is an int > 0 that is not a bool.  ``act=True`` takes the class
    attribute ``default_act`` (models/common.py:49,55), which ``models.default_activation`` sets for the duration of one build."""
    default_act = nn.SiLU()

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, d_or_act=True, act=None):
        super().__init__()
        if act is None:
            if isinstance(d_or_act, bool) or isinstance(d_or_act, nn.Module) or d_or_act is None:
                act, d = d_or_act, 1
            else:
                d, act = int(d_or_act), True
        else:
            d = int(d_or_act) if not isinstance(d_or_act, bool) else 1
        self.cross, self.axis = False, L.AXIS_W
        if isinstance(k, (tuple, list)) or isinstance(s, (tuple, list)):
            k, s, p, axis = _cross_args(c1, c2, k, s, p, g, d)
            if axis is not None:
                self.cross, self.axis = True, axis
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in (c1, c2, k, s, g)):
            raise TypeError(f"Conv arguments must be int: c1={c1}({type(c1)}), c2={c2}({type(c2)})")
        if g <= 0 or c1 % g != 0:
            raise ValueError(f"groups g={g} must be positive and divide c1={c1}")
        self.depthwise = g > 1 and g == c1 == c2
        self.grouped = g > 1 and not self.depthwise
        if self.grouped and not (c2 % g == 0 and (c1 // g) % 16 == 0 and (c2 // g) % 16 == 0 and k in (1, 3) and s == 1
                                 and autopad(k, p) == k // 2 and d == 1):
            raise NotImplementedError(f"the HIP path implements groups=1 (implicit GEMM), groups=c1=c2 (depth-wise, dilation=1) and grouped "
                                      f"convolution with c1/groups and c2/groups multiples of 16, k in {{1,3}}, s=1, p=k//2, d=1; got "
                                      f"c1={c1}, c2={c2}, k={k}, s={s}, p={p}, groups g={g}, d={d}")
        self.groups = g
        if d != 1 and not (g == 1 and d > 1 and s == 1 and k == 3 and p in (None, d)):
            raise NotImplementedError(f"dilated Conv: the HIP path serves g=1, s=1, k=3, d>1 with p=None or p=d (column-form dilated "
                                      f"convolution); got g={g}, s={s}, k={k}, d={d}, p={p}")
        self.d = d
        if self.depthwise and (s not in (1, 2) or k not in (1, 3, 5, 7) or autopad(k, p) != k // 2):
            raise NotImplementedError(f"depth-wise Conv: stride s in {{1,2}}, k in {{1,3,5,7}}, 'same' padding p = k // 2 (got s={s}, k={k}, p={p})")
        self.c1, self.c2, self.k, self.s = c1, c2, k, s
        self.p = autopad(k, p, d)
        if self.cross:                # k taps along one axis: k, s and p are that axis's; (1, k) along W or (k, 1) along H
            kt, st_, pt = ((1, k), (1, s), (0, self.p)) if self.axis == L.AXIS_W else ((k, 1), (s, 1), (self.p, 0))
            self.conv = nn.Conv2d(c1, c2, kt, st_, pt, bias=False)
        else:
            self.conv = nn.Conv2d(c1, c2, k, s, self.p, groups=g, dilation=d, bias=False)
        self.conv.weight.data = self.conv.weight.data.contiguous(memory_format=torch.channels_last)
        self.bn = _BNHolder(c2)
        if act is True:
            dflt = type(self).default_act
            if not type(dflt) is nn.SiLU:
                _pointwise_act_code(dflt, "Conv.default_act")       # a layer with parameters cannot be shared by every Conv
            self.act = nn.SiLU() if type(dflt) is nn.SiLU else dflt
        else:
            self.act = act if isinstance(act, nn.Module) else nn.Identity()
        self.act_code = _act_code(self.act)
        self._wcache = {}
        if d > 1:                     # column form (Tape.dilated_conv): the KRSC master seen as the [c2][9*c1] weight of a 1x1 GEMM
            self.__dict__["_gemm"] = _DeformGemm(self.conv, self.bn)

    # -- parameters in compute layout: _GemmWeights over the KRSC master ``conv.weight`` ---------------------
    @property
    def _wparam(self) -> nn.Parameter:
        return self.conv.weight

    def _gemm_dims(self):
        if self.cross:                # KRSC master [c2][k][c1], the same memory for (1, k) and (k, 1)
            return self.c2, self.k, self.c1
        return self.c2, self.k * self.k, self.c1 // self.groups if self.grouped else self.c1

    def gconv_weights(self, tape: Tape):
        """grouped Conv: compute-dtype copies w [c2][k*k][c1/g] (the master's own shape) and wt [c1][k*k][c2/g] (per-group transpose,
        for the input gradient) from one ydl_gconv_weight_prep launch; cached and invalidated like ``compute_weights``"""
        key = self._wkey(tape)
        c = self._wcache
        if c.get("key") == key:
            return c["w"], c["wt"]
        master = self._master_krsc()
        kk, g = self.k * self.k, self.groups
        w = c.get("w")
        if w is None or c.get("dname") != tape.dname or w.device != master.device:
            c.update(w=torch.empty((self.c2, kk, self.c1 // g), dtype=tape.tdt, device=master.device),
                     wt=torch.empty((self.c1, kk, self.c2 // g), dtype=tape.tdt, device=master.device), dname=tape.dname, key=None)
        L.call("ydl_gconv_weight_prep", tape.dt, _p(master), _p(c["w"]), _p(c["wt"]), self.c2, kk, self.c1, g, _stream())
        c["key"] = key
        return c["w"], c["wt"]

    def trainable(self):
        """(weight, BN weight, BN bias) ``requires_grad`` flags: a frozen parameter (``--freeze``, seg_diceloss_yolov5.py:955-959)
        gets no gradient kernel, is never marked touched and is therefore skipped by the optimizer like torch.optim.SGD skips
        ``grad is None``"""
        return (self.conv.weight.requires_grad, self.bn.weight.requires_grad, self.bn.bias.requires_grad)

    def splittable(self) -> bool:
        """the weight gradient can be written per input-channel block (``wgrad(col0=...)``): dense KRSC storage"""
        return self.c1 % 8 == 0 and self.conv.weight.detach().permute(0, 2, 3, 1).is_contiguous()

    def _place_grad(self, g: torch.Tensor, tmp: torch.Tensor) -> None:
        """exotic gradient layout: let torch place the padded [c2][k*k][cin_p] gradient (cold path)"""
        g.add_(tmp[:, :, :self.c1].view(self.c2, self.k, self.k, self.c1).permute(0, 3, 1, 2))

    # -- depth-wise variant (weight [C,1,k,k]: the KRSC physical layout is [C][k*k]) -------------------------
    def master_dw(self) -> torch.Tensor:
        w = self.conv.weight.detach().permute(0, 2, 3, 1)
        return w if w.is_contiguous() else w.contiguous()

    def grad_dw(self) -> torch.Tensor:
        g = self._grad_of(self.conv.weight).permute(0, 2, 3, 1)
        if not g.is_contiguous():
            raise RuntimeError("Conv weight gradient must be KRSC-contiguous (channels_last storage)")
        return g

    # -- forward ----------------------------------------------------------------------------------------
    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None, res: Optional[Var] = None,
             res_mode: int = L.RES_NONE, act_code: Optional[int] = None) -> Var:
        act = self.act_code if act_code is None else act_code
        if act in (L.ACT_ACON, L.ACT_FRELU):
            # the Conv materialises its BatchNorm output, the layer's own kernels follow; a shortcut is joined behind them
            if res is not None and res_mode != L.RES_AFTER_ACT:
                raise NotImplementedError(f"{type(self.act).__name__}: a residual joined before the activation is not served")
            z = self._fwd(tape, x, act_code=L.ACT_NONE)
            if res is None:
                return self.act._apply_var(tape, z, out=out)
            return tape.add(self.act._apply_var(tape, z), res, out=out)
        if self.d > 1:
            return tape.dilated_conv(x, self.conv, self._gemm, self.d, act, out=out, res=res, res_mode=res_mode)
        self.mark_step(tape)
        if self.depthwise:
            return tape.dw_bn_act(x, self, self.s, act, out=out, res=res, res_mode=res_mode)
        if self.grouped:
            return tape.gconv_bn_act(x, self, act, out=out, res=res, res_mode=res_mode)
        if self.cross:
            return tape.xconv_bn_act(x, self, act, out=out, res=res, res_mode=res_mode)
        if getattr(self, "_fused", None) is not None and not tape.train:
            y = tape.conv_bias_act(x, self, act, res=res, res_mode=res_mode)
            return y if out is None else tape.copy(y, out)
        if (x.ext_src is not None and x.real is None and not x.need and config.stem_s2d() and res is None and self.s > 1
                and self.k % self.s == 0 and self.p % self.s == 0 and self.c1 * self.s * self.s <= 16
                and x.H % self.s == 0 and x.W % self.s == 0):
            # stem on the raw input: conv(k, s, p) == conv(k/s, 1, p/s) over the space-to-depth form (K = 9*16, not 36*8)
            ad = _S2DStem(self)
            return tape.conv_bn_act(tape.input_s2d(x.ext_src, self.s), ad, 1, ad.p, act, out=out)
        return tape.conv_bn_act(x, self, self.s, self.p, act, out=out, res=res, res_mode=res_mode)

    # -- inference-time Conv+BN folding (models/common.py:61-64, utils/torch_utils.py:248-269, models/yolo.py:140-148) --
    def fuse(self) -> "Conv":
        """fold the BatchNorm running statistics into the convolution: eval-mode forward becomes act(conv(x, w') + b')"""
        if self.depthwise:
            raise NotImplementedError("fuse() of a depth-wise Conv")
        if self.grouped:
            raise NotImplementedError("fuse() of a grouped Conv (the folded eval path runs groups=1 convolutions only)")
        if self.cross:
            raise NotImplementedError("fuse() of a cross Conv (the folded eval path runs square convolutions only)")
        if self.d > 1:
            raise NotImplementedError("fuse() of a dilated Conv (the folded eval path runs undilated convolutions only)")
        from .checkpoint import fuse_conv_and_bn
        wf, bf = fuse_conv_and_bn(self.conv, self.bn)
        cp = round_up(self.c2, 8)
        bias = torch.zeros(cp, dtype=torch.float32, device=wf.device)
        bias[:self.c2] = bf
        self._fused = {"w": wf.permute(0, 2, 3, 1).contiguous(), "bias": bias, "ones": torch.ones(cp, dtype=torch.float32, device=wf.device),
                       "cw": {}}
        return self

    def unfuse(self) -> "Conv":
        self._fused = None
        return self

    def forward_fuse(self, x):
        if getattr(self, "_fused", None) is None:
            self.fuse()
        return self.forward(x)

    def _fused_weights(self, tape: Tape):
        f = self._fused
        cw = f["cw"].get(tape.dname)
        if cw is None:
            kk = self.k * self.k
            w = torch.empty((self.c2, kk, round_up(self.c1, 8)), dtype=tape.tdt, device=f["w"].device)
            wt = torch.empty((self.c1, kk, round_up(self.c2, 8)), dtype=tape.tdt, device=f["w"].device)
            L.call("ydl_weight_prep", tape.dt, _p(f["w"]), _p(w), _p(wt), self.c2, kk, self.c1, _stream())
            cw = f["cw"][tape.dname] = (w, wt)
        return cw


class _S2DStem:
    """View of a stem ``Conv`` (k and p multiples of the stride s) as the stride-1 conv it equals over the space-to-depth
    input (ydl_nchw_to_s2d): k/s taps per side, s*s*c1 input channels.  Duck-types the part of ``Conv`` the tape uses;
    weights and gradients go through ydl_weight_prep_s2d / ydl_wgrad_unpack_s2d (same index map as the activation)."""

    def __init__(self, conv: "Conv"):
        self.m = conv
        self.k, self.s, self.p = conv.k // conv.s, 1, conv.p // conv.s
        self.c1, self.c2 = conv.c1 * conv.s * conv.s, conv.c2
        self.bn, self.act_code = conv.bn, conv.act_code

    def splittable(self) -> bool:
        return False

    def compute_weights(self, tape: Tape):
        m = self.m
        key = m._wkey(tape)
        c = m._wcache
        if c.get("s2d_key") != key or c.get("s2d_w") is None:
            if c.get("s2d_w") is None or c["s2d_w"].dtype != tape.tdt:
                c["s2d_w"] = torch.empty((self.c2, self.k * self.k, round_up(self.c1, 8)), dtype=tape.tdt,
                                         device=m.conv.weight.device)
            L.call("ydl_weight_prep_s2d", tape.dt, _p(m._master_krsc()), _p(c["s2d_w"]), m.c2, m.k, m.s, m.c1, _stream())
            c["s2d_key"] = key
        return c["s2d_w"], c["s2d_w"]          # no dgrad: the input is external and needs no gradient

    def coeffs(self, device):
        return self.m.coeffs(device)

    def grad_slot(self, tape: Tape, which: str):
        return self.m.grad_slot(tape, which)

    def touch_bn(self) -> None:
        self.m.touch_bn()

    def trainable(self):
        return self.m.trainable()

    def wgrad(self, tape: Tape, gp, x: Var, dy: Var, st, col0: int = 0, final: bool = True) -> None:
        m = self.m
        p = m.conv.weight
        g = m._grad_of(p)
        gk = g.permute(0, 2, 3, 1)
        tmp = zero_(torch.empty((self.c2, self.k * self.k, round_up(self.c1, 8)), dtype=torch.float32, device=g.device), st)
        _launch_wgrad(tape, gp, _p(x.t), _p(dy.t), _p(tmp), st)
        if gk.is_contiguous():
            L.call("ydl_wgrad_unpack_s2d", _p(tmp), _p(gk), m.c2, m.k, m.s, m.c1, 1, st)
        else:                                           # exotic grad layout: let torch place it (cold path)
            k2, s_ = self.k, m.s
            t6 = tmp[:, :, :self.c1].view(m.c2, k2, k2, s_, s_, m.c1).permute(0, 1, 3, 2, 4, 5).reshape(m.c2, m.k, m.k, m.c1)
            g.add_(t6.permute(0, 3, 1, 2))
        config.mark_touched(p)


class _FusedPair(_GemmWeights):
    """Two 1x1 Convs that read the SAME input (cv1/cv2 of a CSP block) run as ONE convolution with concatenated output
    channels: the input is read once in forward and wgrad, and dgrad writes the input gradient once instead of
    write + read-modify-write.  Possible without any copy when the two modules' parameters, gradients and BN buffers
    are adjacent in memory — which is how yolo_dual_amd.optim.FlatSGDEMA lays the arenas out; otherwise ``make``
    returns None and the block falls back to two convolutions.  Duck-types the part of ``Conv`` the tape uses."""

    def __init__(self, a: "Conv", b: "Conv"):
        self.a, self.b = a, b
        self.c1, self.c2, self.k, self.s, self.p = a.c1, a.c2 + b.c2, a.k, a.s, a.p
        self.act_code = a.act_code
        self._wcache = {}
        self._views = None

    @staticmethod
    def _adjacent(t1: torch.Tensor, t2: torch.Tensor) -> bool:
        return (t1 is not None and t2 is not None and t1.dtype == t2.dtype and
                t1.data_ptr() + t1.numel() * t1.element_size() == t2.data_ptr())

    @classmethod
    def make(cls, a: "Conv", b: "Conv") -> Optional["_FusedPair"]:
        if (a.k, a.s, a.p, a.c1, L.act_key(a.act_code)) != (b.k, b.s, b.p, b.c1, L.act_key(b.act_code)) or a.k != 1:
            return None
        if a.act_code in (L.ACT_ACON, L.ACT_FRELU):      # each half has its own activation parameters behind the BatchNorm
            return None
        if a.c2 % 8 or b.c2 % 8:
            return None
        pairs = [(a.conv.weight, b.conv.weight), (a.bn.weight, b.bn.weight), (a.bn.bias, b.bn.bias),
                 (a.bn.running_mean, b.bn.running_mean), (a.bn.running_var, b.bn.running_var)]
        if not all(cls._adjacent(x.detach(), y.detach()) for x, y in pairs):
            return None
        if not (a.conv.weight.detach().permute(0, 2, 3, 1).is_contiguous() and
                b.conv.weight.detach().permute(0, 2, 3, 1).is_contiguous()):
            return None
        return cls(a, b)

    def still_valid(self) -> bool:
        a, b = self.a, self.b
        key = (a.conv.weight.data_ptr(), b.conv.weight.data_ptr(), a.bn.running_mean.data_ptr())
        if self._views is not None and self._views[0] == key:
            return True
        if _FusedPair.make(a, b) is None:
            return False
        c = self.c2

        def cat1(x, y):
            return torch.as_strided(x.detach(), (c,), (1,))
        w = torch.as_strided(a.conv.weight.detach().permute(0, 2, 3, 1), (c, self.k, self.k, self.c1),
                             (self.k * self.k * self.c1, self.k * self.c1, self.c1, 1))
        bn = _FusedBN()
        bn.weight, bn.bias = cat1(a.bn.weight, b.bn.weight), cat1(a.bn.bias, b.bn.bias)
        bn.running_mean, bn.running_var = cat1(a.bn.running_mean, b.bn.running_mean), cat1(a.bn.running_var, b.bn.running_var)
        bn.eps, bn.momentum = a.bn.eps, a.bn.momentum
        self._views = (key, w, bn)
        return True

    @property
    def bn(self):
        return self._views[2]

    def _master_krsc(self) -> torch.Tensor:
        return self._views[1]

    def _wkey(self, tape: Tape):
        wa, wb = self.a.conv.weight, self.b.conv.weight
        return (tape.dname, wa.data_ptr(), wa._version, wb._version, config.weight_epoch())

    def _gemm_dims(self):
        return self.c2, self.k * self.k, self.c1

    def mark_step(self, tape: Tape) -> None:
        self.a.mark_step(tape)
        self.b.mark_step(tape)

    def _grads(self, which: str):
        if which == "w":
            return self.a.conv.weight, self.b.conv.weight
        return (self.a.bn.weight, self.b.bn.weight) if which == "gamma" else (self.a.bn.bias, self.b.bn.bias)

    def grads_adjacent(self) -> bool:
        for which in ("w", "gamma", "beta"):
            p1, p2 = self._grads(which)
            if p1.grad is None or p2.grad is None or not self._adjacent(p1.grad, p2.grad):
                return False
        g = self.a.conv.weight.grad
        return g.permute(0, 2, 3, 1).is_contiguous() and self.b.conv.weight.grad.permute(0, 2, 3, 1).is_contiguous()

    def grad_slot(self, tape: Tape, which: str):
        p1, p2 = self._grads(which)
        return torch.as_strided(p1.grad, (self.c2,), (1,)), 1

    def touch_bn(self) -> None:
        for which in ("gamma", "beta"):
            for p in self._grads(which):
                if p.requires_grad:
                    config.mark_touched(p)

    def trainable(self):
        return self.a.trainable()

    def uniform_trainable(self) -> bool:
        """both halves frozen or both trainable (one launch writes both halves' gradients)"""
        return self.a.trainable() == self.b.trainable()

    def splittable(self) -> bool:
        return self.c1 % 8 == 0

    def pw_bn_ready(self) -> bool:
        return bool(self.trainable()[0])

    def wgrad(self, tape: Tape, gp, x: Var, dy: Var, st, col0: int = 0, final: bool = True, fuse=None) -> bool:
        p1, p2 = self._grads("w")
        gk = p1.grad.permute(0, 2, 3, 1)
        done = _launch_wgrad(tape, gp, _p(x.t), _p(dy.t) if dy is not None else None, ctypes.c_void_p(gk.data_ptr() + 4 * col0), st, fuse)
        if final:
            config.mark_touched(p1)
            config.mark_touched(p2)
        return done


class _FusedBN:
    pass


def _csp_forward(blk, tape: Tape, x: Var, add: bool) -> Var:
    """shared by C3 / C3Common / C3k2: cv3(cat(m(cv1 x), cv2 x)) (+x) with cv1|cv2 fused when the memory layout allows.
    Buffer T has 3*c_ channels [a | m_out | right]: the fused conv's two halves are activated into T[0:c_] and
    T[2c_:3c_], the last layer of ``m`` writes T[c_:2c_], and cv3 reads the contiguous slice T[c_:3c_] (no copy)."""
    c_, n = blk.c_, len(blk.m)
    pair = getattr(blk, "_pair", None)
    if pair is None:
        pair = blk._pair = _FusedPair(blk.cv1, blk.cv2)
    fused = (config.fuse_siblings() and x.aligned() and not x.lazy and pair.still_valid() and pair.uniform_trainable() and
             (not tape.record or pair.grads_adjacent()))
    if not fused:
        cat = tape.new(x.N, 2 * c_, x.H, x.W)
        left, right = cat.slice(0, c_), cat.slice(c_, 2 * c_)
        a = blk.cv1._fwd(tape, x, out=left if n == 0 else None)
        for i, mm in enumerate(blk.m):
            a = mm._fwd(tape, a, out=left if i == n - 1 else None)
        blk.cv2._fwd(tape, x, out=right)
    else:
        pair.mark_step(tape)
        if n == 0:
            cat = tape.conv_bn_act(x, pair, pair.s, pair.p, pair.act_code)
        else:
            T = tape.new(x.N, 3 * c_, x.H, x.W)
            cat = T.slice(c_, 3 * c_)                 # what cv3 reads: [m_out | right]
            a = T.slice(0, c_)
            mslot, right = cat.slice(0, c_), cat.slice(c_, 2 * c_)   # nested slices: they see cat's gradient state
            tape.conv_bn_act(x, pair, pair.s, pair.p, pair.act_code, out=[a, right])
            for i, mm in enumerate(blk.m):
                a = mm._fwd(tape, a, out=mslot if i == n - 1 else None)
    if add:
        return blk.cv3._fwd(tape, cat, res=x, res_mode=L.RES_AFTER_ACT)
    return blk.cv3._fwd(tape, cat)


# ----------------------------------------------------------------------------------------------------------
# CSP blocks
# ----------------------------------------------------------------------------------------------------------
class C3(YdlModule):
    """Seg-script C3 (seg_diceloss_yolov5.py:416-428): cv3(cat(m(cv1 x), cv2 x)) (+ x), m = n plain 3x3 Convs."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(Conv(c_, c_, 3, 1, g=g) for _ in range(n)))
        self.add = shortcut and c1 == c2
        self.c_ = c_

    def _fwd(self, tape: Tape, x: Var) -> Var:
        return _csp_forward(self, tape, x, self.add)


class C3k2(C3):
    """yolo9 C3k2 (seg_diceloss_yolov9.py:451-472) = script C3; its crop-align branch can never trigger because both
    branches are stride-1 'same' convolutions of the same input."""


class Bottleneck(YdlModule):
    """models/common.py:115-125."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_, c2, 3, 1, g=g)
        self.add = shortcut and c1 == c2

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        h = self.cv1._fwd(tape, x)
        if self.add:
            return self.cv2._fwd(tape, h, out=out, res=x, res_mode=L.RES_AFTER_ACT)
        return self.cv2._fwd(tape, h, out=out)


class C3Common(YdlModule):
    """models/common.py:161-172: m = n Bottlenecks (e=1.0), no outer residual.  Exposed to parse_model as ``C3``."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)))
        self.c_ = c_

    def _fwd(self, tape: Tape, x: Var) -> Var:
        return _csp_forward(self, tape, x, False)


class C2f(YdlModule):
    """yolov8/seg_jaccardloss_yolov8.py:401-414.  cv1 writes the first two chunks of the concat buffer directly."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(Conv(self.c, self.c, 3, 1, g=g) for _ in range(n))
        self.add = shortcut and c1 == c2

    def _fwd(self, tape: Tape, x: Var) -> Var:
        c, n = self.c, len(self.m)
        cat = tape.new(x.N, (2 + n) * c, x.H, x.W)
        self.cv1._fwd(tape, x, out=cat.slice(0, 2 * c))
        last = cat.slice(c, 2 * c)
        for i, mm in enumerate(self.m):
            last = mm._fwd(tape, last, out=cat.slice((2 + i) * c, (3 + i) * c))
        if self.add:
            return self.cv2._fwd(tape, cat, res=x, res_mode=L.RES_AFTER_ACT)
        return self.cv2._fwd(tape, cat)


# ----------------------------------------------------------------------------------------------------------
# space / depth layers, the bare BatchNorm2d row and BottleneckCSP (models/common.py:128-144, 241-250, 282-307; models/yolo.py:330-343)
# ----------------------------------------------------------------------------------------------------------
class Focus(YdlModule):
    """models/common.py:241-250: the four pixel phases of x concatenated on the channels, (::2, ::2), (1::2, ::2), (::2, 1::2),
    (1::2, 1::2), then ``Conv(4 * c1, c2, k, s, p, g, act)``.  The concat is one ydl_space_to_depth launch in ``order`` 1; on the raw
    image it follows the NHWC edge conversion (``Conv``'s own space-to-depth stem, ``_S2DStem``, is a different layer)."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True):
        super().__init__()
        self.conv = Conv(c1 * 4, c2, k, s, p, g, act=act)

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        if x.LH % 2 or x.LW % 2:
            raise ValueError(f"Focus: the {x.LH} x {x.LW} map is not a multiple of 2")
        return self.conv._fwd(tape, tape.space_to_depth(x, 2, order=1), out=out)


def _gain(who: str, gain) -> int:
    if isinstance(gain, bool) or not isinstance(gain, int) or gain < 1:
        raise ValueError(f"{who}: gain={gain!r} must be an int >= 1")
    return gain


class Contract(YdlModule):
    """models/common.py:282-293: (N, C, H, W) -> (N, C * gain^2, H / gain, W / gain), channel (sy * gain + sx) * C + c.  No parameters."""

    def __init__(self, gain=2):
        super().__init__()
        self.gain = _gain("Contract", gain)

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        for what, v in (("height", x.LH), ("width", x.LW)):
            if v % self.gain:
                raise ValueError(f"Contract: the map's {what} {v} is not a multiple of gain={self.gain}")
        return tape.space_to_depth(x, self.gain, order=0, out=out)

    def extra_repr(self):
        return f"gain={self.gain}"


class Expand(YdlModule):
    """models/common.py:296-307: (N, C, H, W) -> (N, C / gain^2, H * gain, W * gain), the inverse of ``Contract``.  No parameters."""

    def __init__(self, gain=2):
        super().__init__()
        self.gain = _gain("Expand", gain)

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        if x.C % self.gain ** 2:
            raise ValueError(f"Expand: {x.C} channels are not a multiple of gain^2={self.gain ** 2}")
        return tape.depth_to_space(x, self.gain, order=0, out=out)

    def extra_repr(self):
        return f"gain={self.gain}"


class BatchNorm2d(_GemmWeights, _BNHolder):
    """The bare ``nn.BatchNorm2d`` row of a yaml (models/yolo.py:330-331): torch's signature and state_dict keys, run by Tape.bn_act with
    no activation.  It is its own ``bn`` and uses the BatchNorm half of ``_GemmWeights`` only (coefficient and gradient rows): there is
    no GEMM in front of it."""
    takes_list = False

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, device=None, dtype=None):
        if not affine or not track_running_stats or momentum is None:
            raise NotImplementedError("BatchNorm2d: the HIP path serves affine=True, track_running_stats=True and a numeric momentum "
                                      f"(got affine={affine}, track_running_stats={track_running_stats}, momentum={momentum})")
        _BNHolder.__init__(self, num_features)
        self.eps, self.momentum = eps, momentum

    @property
    def bn(self):
        return self

    def _gemm_dims(self):
        return self.num_features, 0, 0

    def trainable(self):
        return (False, self.weight.requires_grad, self.bias.requires_grad)

    def forward(self, x):
        if isinstance(x, Var):
            return self._fwd(x.tape, x)
        return run_region(self, [x])

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        self.mark_step(tape)
        return tape.bn_act(x, self, L.ACT_NONE, out=out)


class _BNSlice:
    """channels [c0, c0 + c) of a BatchNorm2d as the tape's launches read them.  The tensors are views taken at the call: the optimizer
    re-homes parameters into its arenas, so a view kept from construction would go stale."""

    def __init__(self, bn: nn.BatchNorm2d, c0: int, c: int):
        self._bn, self._c0, self._c1, self.num_features = bn, c0, c0 + c, c

    eps = property(lambda self: self._bn.eps)
    momentum = property(lambda self: self._bn.momentum)
    weight = property(lambda self: self._bn.weight.detach()[self._c0:self._c1])
    bias = property(lambda self: self._bn.bias.detach()[self._c0:self._c1])
    running_mean = property(lambda self: self._bn.running_mean[self._c0:self._c1])
    running_var = property(lambda self: self._bn.running_var[self._c0:self._c1])


class _CSPConv2d(_GemmWeights, nn.Conv2d):
    """``nn.Conv2d(c1, c2, 1, 1, bias=False)`` of BottleneckCSP (``cv2`` / ``cv3``; state_dict key ``weight``) as Tape.conv_bn_act's
    holder: the launch writes the BatchNorm partial rows of its own output, and its ``bn`` is the view of the block's BatchNorm over the
    half of the concat this convolution fills (BatchNorm is per channel: bn(cat(y1, y2)) = cat(bn[:c_](y1), bn[c_:](y2))).  ``host`` =
    (the block's BatchNorm, first channel, the counter the two halves share)."""
    _wname = "BottleneckCSP.cv2 / cv3"

    def __init__(self, c1, c2):
        super().__init__(c1, c2, 1, 1, bias=False)
        self.c1, self.c2 = c1, c2
        self._wcache = {}

    def attach(self, bn: nn.BatchNorm2d, c0: int, shared: dict) -> None:
        # kept out of the module tree (the BatchNorm belongs to the block, once)
        self.__dict__["_host"] = (bn, c0, shared)

    @property
    def bn(self):
        bn, c0, _shared = self._host
        return _BNSlice(bn, c0, self.c2)

    def _gemm_dims(self):
        return self.c2, 1, self.c1

    def mark_step(self, tape: Tape) -> None:
        pass                     # num_batches_tracked advances once per forward of the block, not once per half

    def trainable(self):
        bn = self._host[0]
        return (self.weight.requires_grad, bn.weight.requires_grad, bn.bias.requires_grad)

    def splittable(self) -> bool:
        return self.c1 % 8 == 0

    def grad_slot(self, tape: Tape, which: str):
        bn, c0, _shared = self._host
        return self._grad_of(bn.weight if which == "gamma" else bn.bias)[c0:c0 + self.c2], 1

    def touch_bn(self) -> None:
        """the block's dgamma / dbeta are complete when BOTH halves have enqueued their backward: only then may the data-parallel hook
        see them"""
        bn, _c0, shared = self._host
        shared["pending"] -= 1
        if shared["pending"] <= 0:
            for p in (bn.weight, bn.bias):
                if p.requires_grad:
                    config.mark_touched(p)


class BottleneckCSP(YdlModule):
    """models/common.py:128-144: cv4(act(bn(cat(cv3(m(cv1 x)), cv2 x)))), ``cv2`` / ``cv3`` bias-free 1x1 convolutions, ``bn`` over the
    2 * c_ concatenated channels, ``act`` the block's own SiLU, m = n Bottlenecks (e = 1.0).  Each of cv3 and cv2 runs as a convolution
    whose launch writes the BatchNorm partial rows of its own output, with a holder that views its half of ``bn``; both activate
    straight into their halves of the one buffer cv4 reads, so the concat and the BatchNorm cost no pass of their own.  ``c_`` must be a
    multiple of 8 (the halves are 16-byte channel groups); other widths are refused."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        if c_ % 8 or c_ < 8:
            raise NotImplementedError(f"BottleneckCSP: c_ = int(c2 * e) = {c_} is not implemented on the HIP path (the two halves of "
                                      "the concat must be multiples of 8 channels)")
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = _CSPConv2d(c1, c_)
        self.cv3 = _CSPConv2d(c_, c_)
        self.cv4 = Conv(2 * c_, c2, 1, 1)
        self.bn = _BNHolder(2 * c_)
        self.act = nn.SiLU()
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)))
        self.c_ = c_
        self._shared = {"pending": 0}
        self.cv3.attach(self.bn, 0, self._shared)
        self.cv2.attach(self.bn, c_, self._shared)

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        c_ = self.c_
        act = _act_code(self.act)
        if tape.train:
            self.bn._nbt_pending += 1
        if tape.record:
            self._shared["pending"] = 2
        cat = tape.new(x.N, 2 * c_, x.H, x.W)
        a = self.cv1._fwd(tape, x)
        for mm in self.m:
            a = mm._fwd(tape, a)
        tape.conv_bn_act(a, self.cv3, 1, 0, act, out=cat.slice(0, c_))
        tape.conv_bn_act(x, self.cv2, 1, 0, act, out=cat.slice(c_, 2 * c_))
        return self.cv4._fwd(tape, cat, out=out)


# ----------------------------------------------------------------------------------------------------------
# Ghost blocks (models/common.py:67-70, 199-204, 253-279)
# ----------------------------------------------------------------------------------------------------------
class DWConv(Conv):
    """models/common.py:67-70: ``Conv`` with g = gcd(c1, c2).  The HIP path serves the depth-wise form g == c1 == c2."""

    def __init__(self, c1, c2, k=1, s=1, d=1, act=True):
        g = math.gcd(c1, c2)
        if not (g == c1 == c2):
            raise NotImplementedError(f"DWConv: c1={c1}, c2={c2} give g = gcd(c1, c2) = {g}; only the depth-wise form g == c1 == c2 is "
                                      "implemented on the HIP path")
        if d != 1:
            raise NotImplementedError(f"DWConv: dilation d={d} is not implemented on the HIP path")
        super().__init__(c1, c2, k, s, None, g, d, act)


class GhostConv(YdlModule):
    """models/common.py:253-263: cat(y, cv2(y)) with y = cv1(x), cv2 a 5x5 depth-wise Conv.  Both halves are written straight into
    one buffer when the half width c_ is a whole number of 8-channel groups (the granularity of the BatchNorm kernels, 16 bytes in
    bf16); other widths go through the concat copies."""

    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        if g != 1:
            raise NotImplementedError(f"GhostConv: groups g={g} is not implemented on the HIP path (g = 1 only)")
        c_ = c2 // 2
        self.cv1 = Conv(c1, c_, k, s, None, g, act=act)
        self.cv2 = Conv(c_, c_, 5, 1, None, c_, act=act)
        self.c_ = c_

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        c_, cv1 = self.c_, self.cv1
        if c_ % 8 == 0 and (out is None or out.aligned()):
            Ho = (x.LH + 2 * cv1.p - cv1.k) // cv1.s + 1
            Wo = (x.LW + 2 * cv1.p - cv1.k) // cv1.s + 1
            cat = out if out is not None else tape.new(x.N, 2 * c_, Ho, Wo)
            a = cv1._fwd(tape, x, out=cat.slice(0, c_))
            self.cv2._fwd(tape, a, out=cat.slice(c_, 2 * c_))
            return cat
        a = cv1._fwd(tape, x)
        cat = tape.concat([a, self.cv2._fwd(tape, a)])
        return cat if out is None else tape.copy(cat, out)


class GhostBottleneck(YdlModule):
    """models/common.py:266-279: conv(x) + shortcut(x)."""

    def __init__(self, c1, c2, k=3, s=1):
        super().__init__()
        c_ = c2 // 2
        self.conv = nn.Sequential(GhostConv(c1, c_, 1, 1),
                                  DWConv(c_, c_, k, s, act=False) if s == 2 else nn.Identity(),
                                  GhostConv(c_, c2, 1, 1, act=False))
        self.shortcut = nn.Sequential(DWConv(c1, c1, k, s, act=False), Conv(c1, c2, 1, 1, act=False)) if s == 2 else nn.Identity()
        self.s = s

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        h = self.conv[0]._fwd(tape, x)
        if self.s == 2:
            h = self.conv[1]._fwd(tape, h)
        h = self.conv[2]._fwd(tape, h)
        if self.s == 2:                                  # the shortcut's linear 1x1 Conv adds the main branch in its BatchNorm apply
            return self.shortcut[1]._fwd(tape, self.shortcut[0]._fwd(tape, x), out=out, res=h, res_mode=L.RES_AFTER_ACT)
        return tape.add(h, x, out=out)


class C3Ghost(C3Common):
    """models/common.py:199-204: C3 whose m is n GhostBottleneck(c_, c_)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.Sequential(*(GhostBottleneck(self.c_, self.c_) for _ in range(n)))


# ----------------------------------------------------------------------------------------------------------
# cross convolutions (models/common.py:147-158, 175-180)
# ----------------------------------------------------------------------------------------------------------
class CrossConv(YdlModule):
    """models/common.py:147-158: cv2(cv1(x)) (+ x) with cv1 = Conv(c1, c_, (1, k), (1, s)) and cv2 = Conv(c_, c2, (k, 1), (s, 1)), both on
    Tape.xconv_bn_act; the shortcut is joined after cv2's activation.  g = 1 only."""

    def __init__(self, c1, c2, k=3, s=1, g=1, e=1.0, shortcut=False):
        super().__init__()
        if g != 1:
            raise NotImplementedError(f"CrossConv: groups g={g} is not implemented on the HIP path (g = 1 only)")
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, (1, k), (1, s))
        self.cv2 = Conv(c_, c2, (k, 1), (s, 1), g=g)
        self.add = shortcut and c1 == c2

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        h = self.cv1._fwd(tape, x)
        if self.add:
            return self.cv2._fwd(tape, h, out=out, res=x, res_mode=L.RES_AFTER_ACT)
        return self.cv2._fwd(tape, h, out=out)


class C3x(C3Common):
    """models/common.py:175-180: C3 whose m is n CrossConv(c_, c_, 3, 1, g, 1.0, shortcut)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        if g != 1:
            raise NotImplementedError(f"C3x: groups g={g} is not implemented on the HIP path (g = 1 only)")
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.Sequential(*(CrossConv(self.c_, self.c_, 3, 1, g, 1.0, shortcut) for _ in range(n)))


# ----------------------------------------------------------------------------------------------------------
# deformable convolution (torchvision.ops.DeformConv2d) and the script blocks built on it
# ----------------------------------------------------------------------------------------------------------
class DeformConv2d(YdlModule):
    """``torchvision.ops.DeformConv2d(in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
    bias=True)`` with ``forward(x, offset, mask=None)``; state_dict ``weight`` [out, in, kh, kw] (+ ``bias``).  Stand-alone
    calls run yolo_dual_amd.deform.deform_conv2d; inside a taped block the op and the BatchNorm that follows it run through
    ``Tape.deform_conv``.  Weight groups > 1 are not implemented."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True):
        super().__init__()
        if groups != 1:
            raise NotImplementedError("DeformConv2d: weight groups > 1 are not implemented on the HIP path (every reference "
                                      "call site uses groups=1)")
        pair = lambda v: (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))
        self.in_channels, self.out_channels, self.groups = in_channels, out_channels, groups
        self.kernel_size, self.stride, self.padding, self.dilation = pair(kernel_size), pair(stride), pair(padding), pair(dilation)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))        # torchvision's reset_parameters
        if self.bias is not None:
            nn.init.uniform_(self.bias, -1 / math.sqrt(in_channels * self.kernel_size[0] * self.kernel_size[1]),
                             1 / math.sqrt(in_channels * self.kernel_size[0] * self.kernel_size[1]))
        self.weight.data = self.weight.data.contiguous(memory_format=torch.channels_last)     # KRSC master

    def forward(self, x, offset, mask=None):
        from .deform import deform_conv2d
        return deform_conv2d(x, offset, self.weight, self.bias, self.stride, self.padding, self.dilation, mask)

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, "
                f"padding={self.padding}, dilation={self.dilation}, bias={self.bias is not None}")


class _DeformGemm(_GemmWeights):
    """parameter holder of the 1x1 GEMM over a deformable column buffer, with Conv's interface for Tape.conv_bn_act: weight
    [Cout][kh*kw*Cin (+1)] = the KRSC weight (+ the bias column), followed by the BatchNorm ``bn``.  Not a module: it only
    points at the DeformConv2d's parameters and the block's BatchNorm.  Its own: the [weight | bias] master and the scatter of
    the padded gradient back into the two parameters; everything else is _GemmWeights."""
    _wname = "DeformConv2d"

    def __init__(self, dc: DeformConv2d, bn: nn.BatchNorm2d):
        self.dc, self.bn = dc, bn
        kh, kw = dc.kernel_size
        self.kk = kh * kw * dc.in_channels
        self.c1 = self.kk + (1 if dc.bias is not None else 0)
        self.c2 = dc.out_channels
        self._wcache = {}

    @property
    def _wparam(self) -> nn.Parameter:
        return self.dc.weight

    def _gemm_dims(self):
        return self.c2, 1, self.c1

    def _wkey(self, tape: Tape):
        w, b = self.dc.weight, self.dc.bias
        return (tape.dname, w.data_ptr(), w._version, b._version if b is not None else -1, config.weight_epoch())

    def _master_krsc(self) -> torch.Tensor:
        wk = super()._master_krsc()
        if self.dc.bias is None:
            return wk
        c, st = self._wcache, _stream()         # [Cout][kk | bias]: two strided copies into a cached f32 buffer
        master = c.get("master")
        if master is None or master.device != wk.device:
            master = c["master"] = torch.empty((self.c2, self.c1), dtype=torch.float32, device=wk.device)
        L.call("ydl_copy2d", L.YDL_F32, _p(wk), self.kk, _p(master), self.c1, self.c2, self.kk, 0, st)
        L.call("ydl_copy2d", L.YDL_F32, _p(self.dc.bias.detach()), 1, ctypes.c_void_p(master.data_ptr() + 4 * self.kk), self.c1,
               self.c2, 1, 0, st)
        return master

    def trainable(self):
        b = self.dc.bias
        return (self.dc.weight.requires_grad or (b is not None and b.requires_grad), self.bn.weight.requires_grad,
                self.bn.bias.requires_grad)

    def splittable(self) -> bool:
        return False

    def pw_bn_ready(self) -> bool:
        return False

    def wgrad(self, tape: Tape, gp, x: Var, dy: Var, st, col0: int = 0, final: bool = True, fuse=None) -> bool:
        w, b = self.dc.weight, self.dc.bias
        if b is None and self.kk % 8 == 0 and w.requires_grad:
            return super().wgrad(tape, gp, x, dy, st, col0, final, fuse)       # the column buffer IS the dense KRSC gradient
        gk = self._grad_of(w).permute(0, 2, 3, 1) if w.requires_grad else None
        if gk is not None and not gk.is_contiguous():
            raise RuntimeError("DeformConv2d weight gradient must be KRSC-contiguous")
        ld = round_up(self.c1, 8)
        tmp = zero_(torch.empty((self.c2, ld), dtype=torch.float32, device=w.device), st)
        _launch_wgrad(tape, gp, _p(x.t), _p(dy.t), _p(tmp), st)
        tape._keep.append(tmp)
        if gk is not None:
            L.call("ydl_copy2d", L.YDL_F32, _p(tmp), ld, _p(gk), self.kk, self.c2, self.kk, 1, st)
            config.mark_touched(w)
        if b is not None and b.requires_grad:
            L.call("ydl_copy2d", L.YDL_F32, ctypes.c_void_p(tmp.data_ptr() + 4 * self.kk), ld, _p(self._grad_of(b)), 1, self.c2, 1, 1, st)
            config.mark_touched(b)
        return False


class _DCNSeq(nn.Sequential):
    """one inner block of the script C3_DCN / C2f_DCN (seg_diceloss_yolov5.py:449-454): Sequential(Conv(c, c, 3, act=False),
    Conv(c, 18, 3) offset branch, DeformConv2d(c, c, 3, padding=1, bias=False), Sequential(BatchNorm2d(c), SiLU))"""
    takes_list = False

    def __init__(self, c, g=1):
        if g != 1:
            raise NotImplementedError("C3_DCN / C2f_DCN: groups g > 1 are not implemented on the HIP path")
        bn = _BNHolder(c)
        super().__init__(Conv(c, c, 3, 1, g=g, d_or_act=False), Conv(c, 2 * 3 * 3, 3, 1, g=g, d_or_act=True),
                         DeformConv2d(c, c, kernel_size=3, padding=1, groups=g, bias=False), nn.Sequential(bn, nn.SiLU(inplace=True)))
        self.__dict__["_gemm"] = _DeformGemm(self[2], bn)

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        x1 = self[0]._fwd(tape, x)
        off = self[1]._fwd(tape, x1)
        return tape.deform_conv(x1, off, None, self[2], self._gemm, L.ACT_SILU, out=out)

    def forward(self, x):
        return run_region(self, [x]) if not isinstance(x, Var) else self._fwd(x.tape, x)


class C3_DCN(C3):
    """Seg-script C3_DCN (unet-lite/yolo5-seg/seg_diceloss_yolov5.py:431-465): C3 wiring (cv3(cat(m(cv1 x), cv2 x)) (+ x)) whose
    inner blocks are 3x3 Conv -> offset Conv(c, 18, 3) -> DeformConv2d(c, c, 3, padding=1) -> BN -> SiLU."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, 0, shortcut, g, e)
        self.m = nn.Sequential(*(_DCNSeq(self.c_, g) for _ in range(n)))


class C2f_DCN(C2f):
    """Seg-script C2f_DCN (yolov8/seg_diceloss_yolov8.py:417-457): C2f wiring (split, chain on the last chunk, concat) with the
    C3_DCN inner blocks."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, 0, shortcut, g, e)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(_DCNSeq(self.c, g) for _ in range(n))


class _BiasConv2d(_GemmWeights, nn.Conv2d):
    """``nn.Conv2d(c1, c2, k, s, p, bias=True)`` run by Tape.conv_bias (no BatchNorm, no activation); weight kept channels_last
    (the KRSC master).  ``_keep_init``: the yaml models' kaiming pass leaves its (zero) initialisation alone."""
    _keep_init = True
    _wname = "conv_offset_mask"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.weight.data = self.weight.data.contiguous(memory_format=torch.channels_last)
        self.k, self.s, self.p = self.kernel_size[0], self.stride[0], self.padding[0]
        self._wcache = {}

    def _gemm_dims(self):
        return self.out_channels, self.k * self.k, self.in_channels


# the stride-2 transposed convolutions that double the map exactly: Ho = (H - 1) * 2 - 2 p + k + output_padding = 2 H
_TCONV_FORMS = ((2, 0, 0), (4, 1, 0), (3, 1, 1))


def _pair_int(v, who: str, what: str) -> int:
    """a square int / (a, a) argument as an int; anything rectangular is refused by name"""
    if isinstance(v, (tuple, list)):
        if len(v) != 2 or v[0] != v[1]:
            raise NotImplementedError(f"{who}: {what}={tuple(v)} must be square on the HIP path")
        v = v[0]
    return int(v)


def _tconv_args(who: str, names, c1, c2, k, s, p, op, groups=1, dilation=1, padding_mode="zeros", depthwise=False):
    """the served set of the two transposed convolutions; ``names`` = the constructor's own names for (kernel, stride, padding,
    output padding).  Everything outside it raises NotImplementedError naming the class and the offending argument."""
    nk, ns, np_, nop = names
    k, s, p, op = _pair_int(k, who, nk), _pair_int(s, who, ns), _pair_int(p, who, np_), _pair_int(op, who, nop)
    d = _pair_int(dilation, who, "dilation")
    if padding_mode != "zeros":
        raise NotImplementedError(f"{who}: padding_mode={padding_mode!r} is not implemented (zeros only)")
    if d != 1:
        raise NotImplementedError(f"{who}: dilation={d} is not implemented on the HIP path (dilation = 1 only)")
    if depthwise:
        if not (c1 == c2 == groups):
            raise NotImplementedError(f"{who}: c1={c1}, c2={c2} give groups = gcd(c1, c2) = {groups}; only the depth-wise form "
                                      f"groups == c1 == c2 is implemented on the HIP path")
    elif groups != 1:
        raise NotImplementedError(f"{who}: groups={groups} is not implemented on the HIP path (groups = 1; the depth-wise form is "
                                  "DWConvTranspose2d)")
    if s != 2:
        raise NotImplementedError(f"{who}: {ns}={s} is not implemented on the HIP path ({ns} = 2 only)")
    if k not in (2, 3, 4):
        raise NotImplementedError(f"{who}: {nk}={k} is not implemented on the HIP path: ({nk}, {np_}, {nop}) must be one of "
                                  f"{_TCONV_FORMS} at {ns} = 2")
    want = {f[0]: f for f in _TCONV_FORMS}[k]
    if p != want[1]:
        raise NotImplementedError(f"{who}: {np_}={p} with {nk}={k} is not implemented on the HIP path: ({nk}, {np_}, {nop}) must be "
                                  f"one of {_TCONV_FORMS}")
    if op != want[2]:
        raise NotImplementedError(f"{who}: {nop}={op} with {nk}={k} is not implemented on the HIP path: ({nk}, {np_}, {nop}) must be "
                                  f"one of {_TCONV_FORMS}")
    if c1 % 8 or c2 % 8:
        bad = ("c1" if depthwise else "in_channels") if c1 % 8 else ("c2" if depthwise else "out_channels")
        raise NotImplementedError(f"{who}: {bad}={c1 if c1 % 8 else c2} is not implemented on the HIP path (channel counts must be "
                                  "multiples of 8)")
    return k, s, p, op


class _TConvBase:
    """stand-alone call / taped call dispatch of the two transposed convolutions (YdlModule.forward for an nn.ConvTranspose2d)"""
    takes_list = False

    def forward(self, x, output_size=None):
        if output_size is not None:
            raise NotImplementedError(f"{self._wname}: output_size is not implemented (the served forms double the map exactly)")
        if isinstance(x, Var):
            return self._fwd(x.tape, x)
        return run_region(self, [x])


class ConvTranspose2d(_TConvBase, _GemmWeights, nn.ConvTranspose2d):
    """``nn.ConvTranspose2d(c1, c2, k, 2, p, output_padding)`` in the three forms that double the map (``_TCONV_FORMS``), groups 1,
    run by Tape.conv_transpose on the implicit-GEMM entry points with the roles of x and dy exchanged: the parameter [c1][c2][k][k]
    kept channels_last is physically [c1][k*k][c2], the KRSC master of the mirrored convolution c2 -> c1."""
    _wname = "ConvTranspose2d"

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, output_padding=0, groups=1, bias=True,
                 dilation=1, padding_mode="zeros", device=None, dtype=None):
        k, s, p, op = _tconv_args("ConvTranspose2d", ("kernel_size", "stride", "padding", "output_padding"), in_channels, out_channels,
                                  kernel_size, stride, padding, output_padding, groups, dilation, padding_mode)
        super().__init__(in_channels, out_channels, k, s, p, op, groups, bias, dilation, padding_mode, device, dtype)
        self.weight.data = self.weight.data.contiguous(memory_format=torch.channels_last)
        self.k, self.s, self.p, self.op = k, s, p, op
        self._wcache = {}

    def _gemm_dims(self):
        return self.in_channels, self.k * self.k, self.out_channels

    def _bias_len(self) -> int:
        return self.out_channels

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        return tape.conv_transpose(x, self, out=out)


class DWConvTranspose2d(_TConvBase, nn.ConvTranspose2d):
    """models/common.py:73-76: ``nn.ConvTranspose2d(c1, c2, k, s, p1, p2, groups=gcd(c1, c2))``; served depth-wise (c1 == c2) at
    s = 2 in the forms of ``_TCONV_FORMS``, by the kernels of csrc/tconv.hip (Tape.dw_conv_transpose).  The weight [C][1][k][k] is
    the f32 master [C][k*k] the kernels read."""
    _wname = "DWConvTranspose2d"

    def __init__(self, c1, c2, k=1, s=1, p1=0, p2=0):
        g = math.gcd(c1, c2)
        k, s, p1, p2 = _tconv_args("DWConvTranspose2d", ("k", "s", "p1", "p2"), c1, c2, k, s, p1, p2, groups=g, depthwise=True)
        super().__init__(c1, c2, k, s, p1, p2, groups=g)
        self.k, self.s, self.p, self.op = k, s, p1, p2

    def master_dw(self) -> torch.Tensor:
        w = self.weight.detach().permute(0, 2, 3, 1)
        return w if w.is_contiguous() else w.contiguous()

    def grad_dw(self) -> torch.Tensor:
        if self.weight.grad is None:
            self.weight.grad = torch.zeros_like(self.weight)
        g = self.weight.grad.permute(0, 2, 3, 1)
        if not g.is_contiguous():
            raise RuntimeError("DWConvTranspose2d weight gradient must be [C][k*k]-contiguous")
        return g

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        return tape.dw_conv_transpose(x, self, out=out)


class DCNv2(YdlModule):
    """models/common.py:1629-1690: ``conv_offset_mask`` (plain biased Conv2d, zero-initialised) -> offsets = channels [0, 2GK),
    mask = sigmoid(channels [2GK, 3GK)) -> deform_conv2d(x, weight, offset, mask, bias) -> BatchNorm -> SiLU.  The sigmoid runs
    inside the gather / backward kernels (the logits are read in place), the bias is one more column of the GEMM (so it reaches
    the output, the BN running mean and its gradient exactly as in the reference)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=1, dilation=1, groups=1, deformable_groups=1):
        super().__init__()
        if groups != 1:
            raise NotImplementedError("DCNv2: weight groups > 1 are not implemented on the HIP path")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = (kernel_size, kernel_size), (stride, stride)
        self.padding, self.dilation = (padding, padding), (dilation, dilation)
        self.groups, self.deformable_groups = groups, deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.conv_offset_mask = _BiasConv2d(in_channels, deformable_groups * 3 * kernel_size * kernel_size, kernel_size, stride,
                                            padding, bias=True)
        self.bn = _BNHolder(out_channels)
        dflt = Conv.default_act                  # models/common.py:1659: DCNv2 follows Conv's default activation
        self.act = nn.SiLU() if type(dflt) is nn.SiLU else dflt
        self.act_code = _pointwise_act_code(self.act, "DCNv2")
        self.reset_parameters()
        self.weight.data = self.weight.data.contiguous(memory_format=torch.channels_last)
        self.__dict__["_gemm"] = _DeformGemm(self, self.bn)

    def reset_parameters(self):
        n = self.in_channels * self.kernel_size[0] * self.kernel_size[1]
        std = 1.0 / math.sqrt(n)
        self.weight.data.uniform_(-std, std)
        self.bias.data.zero_()
        self.conv_offset_mask.weight.data.zero_()
        self.conv_offset_mask.bias.data.zero_()

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None, res: Optional[Var] = None, res_mode: int = L.RES_NONE) -> Var:
        GK = self.deformable_groups * self.kernel_size[0] * self.kernel_size[1]
        om = tape.conv_bias(x, self.conv_offset_mask)
        return tape.deform_conv(x, om.slice(0, 2 * GK), om.slice(2 * GK, 3 * GK), self, self._gemm, self.act_code, mask_sigmoid=True,
                                out=out, res=res, res_mode=res_mode)


class Bottleneck_DCN(YdlModule):
    """models/common.py:1692-1703: x (+) DCNv2(cv1(x))"""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = DCNv2(c_, c2, 3, 1, groups=g)
        self.add = shortcut and c1 == c2

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        h = self.cv1._fwd(tape, x)
        if self.add:
            return self.cv2._fwd(tape, h, out=out, res=x, res_mode=L.RES_AFTER_ACT)
        return self.cv2._fwd(tape, h, out=out)


class C3_DCNCommon(C3Common):
    """models/common.py:1705-1711 ``C3_DCN(C3)``: common.py's C3 wiring (no outer residual) with n Bottleneck_DCN (e=1.0).
    parse_model resolves the yaml name C3_DCN to this class (with ``deformable=True``); the seg-script builders resolve it to
    the script C3_DCN."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, 0, shortcut, g, e)
        self.m = nn.Sequential(*(Bottleneck_DCN(self.c_, self.c_, shortcut, g, e=1.0) for _ in range(n)))


class GAM(YdlModule):
    """yolo9 global-aggregation channel attention (unet-lite/yolo9-seg/seg_diceloss_yolov9.py:475-510):
    x * sigmoid(conv2(avgpool(conv1 x)) + conv3(maxpool(conv1 x))).  conv1 runs twice like the reference (its BN
    running statistics advance twice per step).  Must be built as ``GAM(c)``: the shipped yaml's ``GAM [512]`` binds
    k=512 and cannot be constructed."""

    def __init__(self, c, k=1, s=1, e=0.25):
        super().__init__()
        c_ = int(c * e)
        self.conv1 = Conv(c, c_, k, s)
        self.conv2 = Conv(c_, c, k, s, act=False)
        self.conv3 = Conv(c_, c, k, s, act=False)

    def _fwd(self, tape: Tape, x: Var) -> Var:
        y1 = tape.global_pool(self.conv1._fwd(tape, x), "avg")
        y1 = self.conv2._fwd(tape, y1)
        y2 = tape.global_pool(self.conv1._fwd(tape, x), "max")
        y2 = self.conv3._fwd(tape, y2)
        return tape.gate_mul(x, y1, y2)


class SPPF(YdlModule):
    """seg_diceloss_yolov5.py:468-481 / models/common.py:223-238: three chained 5x5/s1 max-pools written straight into
    the 4-way concat buffer."""

    def __init__(self, c1, c2, k=5):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * 4, c2, 1, 1)
        self.k = k
        self.c_ = c_

    def _fwd(self, tape: Tape, x: Var) -> Var:
        c_ = self.c_
        cat = tape.new(x.N, 4 * c_, x.H, x.W)
        s0 = self.cv1._fwd(tape, x, out=cat.slice(0, c_))
        tape.sppf_pools(s0, self.k, [cat.slice(c_, 2 * c_), cat.slice(2 * c_, 3 * c_), cat.slice(3 * c_, 4 * c_)])
        return self.cv2._fwd(tape, cat)


# ----------------------------------------------------------------------------------------------------------
# SPP pyramid blocks (models/common.py:191-197 C3SPP, :1275-1286 SPP, :1292-1330 SimConv / SimSPPF, :1430-1448 SPPCSPC,
# :1451-1468 SPPCSPC_group, :1473-1492 SimCSPSPPF)
# ----------------------------------------------------------------------------------------------------------
def _odd_windows(name: str, k) -> tuple:
    ks = tuple(int(v) for v in (k if isinstance(k, (tuple, list)) else (k,)))
    if any(v < 1 or v % 2 == 0 for v in ks):
        raise NotImplementedError(f"{name}: max-pool window sizes {ks} are not implemented (odd sizes only: an even k with padding "
                                  "k // 2 changes the output size, and the reference's concat then fails)")
    return ks


class SPP(YdlModule):
    """models/common.py:1275-1286: cv2(cat(y, mp_k1(y), mp_k2(y), ...)) with y = cv1(x); the pools are PARALLEL, every one of y
    (Tape.spp_pools), and write straight into the concat buffer cv1 opened."""

    def __init__(self, c1, c2, k=(5, 9, 13)):
        super().__init__()
        self.k = _odd_windows("SPP", k)
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * (len(self.k) + 1), c2, 1, 1)
        self.c_ = c_

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        c_, n = self.c_, len(self.k)
        cat = tape.new(x.N, (n + 1) * c_, x.LH, x.LW)
        s0 = self.cv1._fwd(tape, x, out=cat.slice(0, c_))
        tape.spp_pools(s0, self.k, [cat.slice((i + 1) * c_, (i + 2) * c_) for i in range(n)])
        return self.cv2._fwd(tape, cat, out=out)


class C3SPP(C3Common):
    """models/common.py:191-197: C3 whose ``m`` is one SPP(c_, c_, k).  Note the argument order: k comes before n."""

    def __init__(self, c1, c2, k=(5, 9, 13), n=1, shortcut=True, g=1, e=0.5):
        if g != 1:
            raise NotImplementedError(f"C3SPP: groups g={g} is not implemented on the HIP path (g = 1 only)")
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = SPP(self.c_, self.c_, k)

    def _fwd(self, tape: Tape, x: Var) -> Var:
        c_ = self.c_
        cat = tape.new(x.N, 2 * c_, x.LH, x.LW)
        self.m._fwd(tape, self.cv1._fwd(tape, x), out=cat.slice(0, c_))
        self.cv2._fwd(tape, x, out=cat.slice(c_, 2 * c_))
        return self.cv3._fwd(tape, cat)


class SimConv(Conv):
    """models/common.py:1292-1313: Conv2d(bias=False, padding kernel_size // 2) -> BatchNorm2d -> ReLU."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, groups=1, bias=False):
        if groups != 1:
            raise NotImplementedError(f"SimConv: groups={groups} is not implemented on the HIP path (groups = 1 only)")
        if bias:
            raise NotImplementedError("SimConv: bias=True is not implemented on the HIP path (the convolution in front of a BatchNorm "
                                      "carries no bias)")
        super().__init__(in_channels, out_channels, kernel_size, stride, kernel_size // 2, 1, act=nn.ReLU())


class SimSPPF(YdlModule):
    """models/common.py:1315-1330: SPPF on SimConv; the pools are SPPF's chain (Tape.sppf_pools)."""

    def __init__(self, in_channels, out_channels, kernel_size=5):
        super().__init__()
        self.k, = _odd_windows("SimSPPF", kernel_size)
        c_ = in_channels // 2
        self.cv1 = SimConv(in_channels, c_, 1, 1)
        self.cv2 = SimConv(c_ * 4, out_channels, 1, 1)
        self.c_ = c_

    _fwd = SPPF._fwd


class _CSPPool(YdlModule):
    """what SPPCSPC and SimCSPSPPF share (models/common.py:1430-1448, :1473-1492): x1 = cv4(cv3(cv1 x)) opens a 4-way concat buffer,
    ``_pools`` fills its other three slices, y1 = cv6(cv5(buffer)) and y2 = cv2(x) are written into the halves of cv7's input.
    ``n``, ``shortcut`` and ``g`` are accepted and unused, as in the reference (which never hands ``g`` to a convolution)."""

    conv_groups = 1        # SPPCSPC_group: 4

    def __init__(self, c1, c2, e):
        super().__init__()
        c_ = int(2 * c2 * e)
        g = self.conv_groups
        self.cv1 = Conv(c1, c_, 1, 1, g=g)
        self.cv2 = Conv(c1, c_, 1, 1, g=g)
        self.cv3 = Conv(c_, c_, 3, 1, g=g)
        self.cv4 = Conv(c_, c_, 1, 1, g=g)
        self.cv5 = Conv(4 * c_, c_, 1, 1, g=g)
        self.cv6 = Conv(c_, c_, 3, 1, g=g)
        self.cv7 = Conv(2 * c_, c2, 1, 1, g=g)
        self.c_ = c_

    def _fwd(self, tape: Tape, x: Var) -> Var:
        c_ = self.c_
        cat = tape.new(x.N, 4 * c_, x.LH, x.LW)
        x1 = self.cv4._fwd(tape, self.cv3._fwd(tape, self.cv1._fwd(tape, x)), out=cat.slice(0, c_))
        self._pools(tape, x1, [cat.slice((i + 1) * c_, (i + 2) * c_) for i in range(3)])
        halves = tape.new(x.N, 2 * c_, x.LH, x.LW)
        self.cv6._fwd(tape, self.cv5._fwd(tape, cat), out=halves.slice(0, c_))
        self.cv2._fwd(tape, x, out=halves.slice(c_, 2 * c_))
        return self.cv7._fwd(tape, halves)


class SPPCSPC(_CSPPool):
    """models/common.py:1430-1448 (YOLOv7): parallel pools of x1 (Tape.spp_pools).  cv5 takes 4 * c_ channels, so ``k`` holds three
    window sizes."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5, k=(5, 9, 13)):
        super().__init__(c1, c2, e)
        self.k = _odd_windows("SPPCSPC", k)
        if len(self.k) != 3:
            raise ValueError(f"SPPCSPC: k={k} must hold three window sizes (cv5 reads 4 * c_ channels)")

    def _pools(self, tape: Tape, x1: Var, outs) -> None:
        tape.spp_pools(x1, self.k, outs)


class SimCSPSPPF(_CSPPool):
    """models/common.py:1473-1492 (YOLOv6 v0.3; SiLU Convs despite the name): SPPF's chain of pools (Tape.sppf_pools)."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5, k=5):
        super().__init__(c1, c2, e)
        self.k, = _odd_windows("SimCSPSPPF", k)

    def _pools(self, tape: Tape, x1: Var, outs) -> None:
        tape.sppf_pools(x1, self.k, outs)


class SPPCSPC_group(SPPCSPC):
    """models/common.py:1451-1468: SPPCSPC whose seven convolutions are all Conv(g=4) (Tape.gconv_bn_act); every one of them must lie
    in the grouped Conv's served set, i.e. c1 / 4 and c_ / 4 and c2 / 4 are multiples of 16."""
    conv_groups = 4


# ----------------------------------------------------------------------------------------------------------
# dilated context blocks (models/common.py:1336-1361 ASPP, :1366-1384 BasicConv, :1386-1425 RFB)
# ----------------------------------------------------------------------------------------------------------
class _Conv2d(_BiasConv2d):
    """a plain ``nn.Conv2d`` of a context block (Tape.conv_bias); unlike DCNv2's conv_offset_mask it takes the yaml models' kaiming pass"""
    _keep_init = False
    _wname = "Conv2d"


class _DilatedConv2d(_Conv2d):
    """``nn.Conv2d(c1, c2, k, 1, padding=d*(k-1)/2, dilation=d)`` as Tape.dilated_conv runs it: the 1x1 layer over the column buffer,
    weight [c2][1][k*k*c1] = the KRSC master as it is"""
    _wname = "dilated Conv2d"

    def __init__(self, c1, c2, k, d, bias=True):
        super().__init__(c1, c2, k, 1, d * (k - 1) // 2, dilation=d, bias=bias)
        self.k, self.s, self.p = 1, 1, 0

    def _gemm_dims(self):
        return self.out_channels, 1, self.kernel_size[0] * self.kernel_size[1] * self.in_channels


def _square(v, what: str) -> int:
    if isinstance(v, (tuple, list)):
        if len(v) != 2 or v[0] != v[1]:
            raise NotImplementedError(f"BasicConv: {what}={v} must be square on the HIP path")
        v = v[0]
    return int(v)


class BasicConv(Conv):
    """models/common.py:1366-1384: Conv2d(bias=False) -> BatchNorm2d(eps=1e-5, momentum=0.01) -> optional ReLU, or with ``bn=False`` a
    biased Conv2d alone.  groups = 1; a dilation d > 1 needs kernel_size 3, stride 1, padding d (Tape.dilated_conv)."""

    def __init__(self, in_planes, out_planes, kernel_size, stride=1, padding=0, dilation=1, groups=1, relu=True, bn=True):
        k, p, d = _square(kernel_size, "kernel_size"), _square(padding, "padding"), _square(dilation, "dilation")
        if groups != 1:
            raise NotImplementedError(f"BasicConv: groups={groups} is not implemented on the HIP path (groups = 1 only)")
        super().__init__(in_planes, out_planes, k, stride, p, 1, d, nn.ReLU(inplace=True) if relu else False)
        self.out_channels = out_planes
        self.relu = self.act if relu else None
        self.bn.eps, self.bn.momentum = 1e-5, 0.01
        if not bn:
            if relu:
                raise NotImplementedError("BasicConv(bn=False, relu=True): the bias form runs without an activation on the HIP path")
            self.bn = None
            self.conv = _DilatedConv2d(in_planes, out_planes, k, d) if d > 1 else _Conv2d(in_planes, out_planes, k, stride, p)

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None, res: Optional[Var] = None,
             res_mode: int = L.RES_NONE, act_code: Optional[int] = None) -> Var:
        if self.bn is not None:
            return super()._fwd(tape, x, out=out, res=res, res_mode=res_mode, act_code=act_code)
        if res is not None or act_code not in (None, L.ACT_NONE):
            raise NotImplementedError("BasicConv(bn=False) takes no residual and no activation")
        if self.d > 1:
            y = tape.dilated_conv(x, self.conv, self.conv, self.d, L.ACT_NONE, out=out if out is None or out.aligned() else None)
        else:
            y = tape.conv_bias(x, self.conv, out=out if out is None or out.aligned() else None)
        return y if out is None or y is out else tape.copy(y, out)

    def fuse(self) -> "Conv":
        if self.bn is None:
            raise NotImplementedError("fuse() of a BasicConv without BatchNorm")
        return super().fuse()


class RFB(YdlModule):
    """models/common.py:1386-1425: three branches ending in 3x3 convolutions of dilation vision+1, vision+2, vision+4, written into
    one concat buffer, ``ConvLinear``, ``shortcut`` and relu(ConvLinear(cat) * scale + shortcut(x)).  ``scale`` multiplies the
    BatchNorm output of ConvLinear as written (Tape.scale), so that layer's gradients carry the factor; the sum and the ReLU run in
    the shortcut's BatchNorm apply.  stride = 1 and groups = 1 only."""

    def __init__(self, in_planes, out_planes, stride=1, scale=0.1, map_reduce=8, vision=1, groups=1):
        super().__init__()
        if stride != 1:
            raise NotImplementedError(f"RFB: stride={stride} is not implemented on the HIP path (stride 1 only)")
        if groups != 1:
            raise NotImplementedError(f"RFB: groups={groups} is not implemented on the HIP path (groups = 1 only)")
        self.scale = scale
        self.out_channels = out_planes
        ip = in_planes // map_reduce
        self.inter_planes = ip

        def tail(d):
            return BasicConv(2 * ip, 2 * ip, kernel_size=3, stride=1, padding=d, dilation=d, relu=False)
        self.branch0 = nn.Sequential(BasicConv(in_planes, ip, kernel_size=1, stride=1, relu=False),
                                     BasicConv(ip, 2 * ip, kernel_size=(3, 3), stride=stride, padding=(1, 1)), tail(vision + 1))
        self.branch1 = nn.Sequential(BasicConv(in_planes, ip, kernel_size=1, stride=1, relu=False),
                                     BasicConv(ip, 2 * ip, kernel_size=(3, 3), stride=stride, padding=(1, 1)), tail(vision + 2))
        self.branch2 = nn.Sequential(BasicConv(in_planes, ip, kernel_size=1, stride=1, relu=False),
                                     BasicConv(ip, (ip // 2) * 3, kernel_size=3, stride=1, padding=1),
                                     BasicConv((ip // 2) * 3, 2 * ip, kernel_size=3, stride=stride, padding=1), tail(vision + 4))
        self.ConvLinear = BasicConv(6 * ip, out_planes, kernel_size=1, stride=1, relu=False)
        self.shortcut = BasicConv(in_planes, out_planes, kernel_size=1, stride=stride, relu=False)
        self.relu = nn.ReLU(inplace=False)

    def _gate(self, device, N: int) -> torch.Tensor:
        """``scale`` as the constant f32 [N][C] operand of ydl_scale_channels (made once: the taped region issues no ATen kernel)"""
        g = self.__dict__.get("_gate_t")
        if g is None or g.device != device or g.shape[0] != N:
            g = self.__dict__["_gate_t"] = torch.full((N, self.out_channels), float(self.scale), dtype=torch.float32, device=device)
        return g

    def _fwd(self, tape: Tape, x: Var) -> Var:
        x = tape._flat(x)
        ip = self.inter_planes
        cat = tape.new(x.N, 6 * ip, x.H, x.W)
        for i, br in enumerate((self.branch0, self.branch1, self.branch2)):
            h = x
            for j, blk in enumerate(br):
                h = blk._fwd(tape, h, out=cat.slice(2 * ip * i, 2 * ip * (i + 1)) if j == len(br) - 1 else None)
        lin = tape.scale(self.ConvLinear._fwd(tape, cat), self._gate(tape.device, x.N))
        return self.shortcut._fwd(tape, x, res=lin, res_mode=L.RES_BEFORE_ACT, act_code=L.ACT_RELU)


class ASPP(YdlModule):
    """models/common.py:1336-1361 (the version without BatchNorm): cat(upsample(conv(avgpool x)), 1x1 conv, three 3x3 convs of
    dilation 6 / 12 / 18) -> conv_1x1_output; every layer a biased ``nn.Conv2d``, no activation.  The bilinear up-sampling of the
    pooled 1x1 map is a broadcast (Tape.resize); each branch writes its channel block of the one concat buffer when the block is a
    whole number of 8-channel groups."""

    def __init__(self, in_channel=512, out_channel=256):
        super().__init__()
        self.mean = nn.AdaptiveAvgPool2d((1, 1))
        self.conv = _Conv2d(in_channel, out_channel, 1, 1)
        self.atrous_block1 = _Conv2d(in_channel, out_channel, 1, 1)
        self.atrous_block6 = _DilatedConv2d(in_channel, out_channel, 3, 6)
        self.atrous_block12 = _DilatedConv2d(in_channel, out_channel, 3, 12)
        self.atrous_block18 = _DilatedConv2d(in_channel, out_channel, 3, 18)
        self.conv_1x1_output = _Conv2d(out_channel * 5, out_channel, 1, 1)
        self.out_channel = out_channel

    def _fwd(self, tape: Tape, x: Var) -> Var:
        x = tape._flat(x)
        c = self.out_channel
        cat = tape.new(x.N, 5 * c, x.H, x.W)
        direct = c % 8 == 0
        pooled = tape.conv_bias(tape.global_pool(x, "avg"), self.conv)
        tape.resize(pooled, x.H, x.W, L.RESIZE_BILINEAR, out=cat.slice(0, c))
        for i, blk in enumerate((self.atrous_block1, self.atrous_block6, self.atrous_block12, self.atrous_block18)):
            sl = cat.slice((i + 1) * c, (i + 2) * c)
            out = sl if direct else None
            y = tape.conv_bias(x, blk, out=out) if i == 0 else tape.dilated_conv(x, blk, blk, blk.dilation[0], L.ACT_NONE, out=out)
            if not direct:
                tape.copy(y, sl)
        return tape.conv_bias(cat, self.conv_1x1_output)


class Concat(YdlModule):
    """Auto-aligning Concat (seg_diceloss_yolov5.py:484-507); with equal sizes it is models/common.py:310-317."""
    takes_list = True

    def __init__(self, dimension=1):
        super().__init__()
        self.d = dimension
        if dimension != 1:
            raise NotImplementedError("Concat along the channel dimension only")

    def _fwd(self, tape: Tape, xs: Sequence[Var]) -> Var:
        if len(xs) == 1:
            return xs[0]
        return tape.concat(xs, align=True)


class Upsample(YdlModule):
    """nn.Upsample restated for the taped path (nearest, or bilinear / bicubic with either align_corners convention).  Bicubic is
    never lazy and runs outside the virtual-concat fusions: materialize + Tape.resize (ydl_bicubic_fwd / ydl_bicubic_bwd)."""

    def __init__(self, size=None, scale_factor=None, mode="nearest", align_corners=None):
        super().__init__()
        self.size = size
        self.scale_factor = scale_factor
        self.mode = mode
        self.align_corners = align_corners
        if mode not in ("nearest", "bilinear", "bicubic"):
            raise NotImplementedError(f"Upsample mode {mode}")

    def _out_size(self, x: Var):
        if self.size is not None:
            return (self.size, self.size) if isinstance(self.size, int) else tuple(self.size)
        sf = self.scale_factor
        sh, sw = (sf, sf) if not isinstance(sf, (tuple, list)) else sf
        return int(math.floor(x.H * sh)), int(math.floor(x.W * sw))

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        if self.mode == "nearest" and self.size is None and out is None and config.lazy_upsample():
            sf = self.scale_factor
            sh, sw = (sf, sf) if not isinstance(sf, (tuple, list)) else sf
            if float(sh).is_integer() and float(sw).is_integer() and sh >= 1 and sw >= 1:
                return tape.upsample_lazy(x, int(sh), int(sw))     # no memory traffic; see tape.Var.rep
        x = tape.materialize(x)
        Ho, Wo = self._out_size(x)
        if self.mode == "nearest":
            # ATen passes 1/scale_factor as the index scale when a scale_factor was given
            if self.size is None:
                sf = self.scale_factor
                sh, sw = (sf, sf) if not isinstance(sf, (tuple, list)) else sf
                return tape.resize(x, Ho, Wo, L.RESIZE_NEAREST, 1.0 / sh, 1.0 / sw, out=out)
            return tape.resize(x, Ho, Wo, L.RESIZE_NEAREST, out=out)
        if self.mode == "bicubic":
            mode = L.RESIZE_BICUBIC_AC if self.align_corners else L.RESIZE_BICUBIC
        else:
            mode = L.RESIZE_BILINEAR_AC if self.align_corners else L.RESIZE_BILINEAR
        if self.size is None and not self.align_corners:
            sf = self.scale_factor
            sh, sw = (sf, sf) if not isinstance(sf, (tuple, list)) else sf
            return tape.resize(x, Ho, Wo, mode, 1.0 / sh, 1.0 / sw, out=out)
        return tape.resize(x, Ho, Wo, mode, out=out)

    def extra_repr(self):
        return f"size={self.size}, scale_factor={self.scale_factor}, mode={self.mode}"


# ----------------------------------------------------------------------------------------------------------
# ResNet blocks + multi-scale SegmentHead (segment/train.py:74-210, Resnet18/seg_diceloss_resnet18.py:216-349)
# ----------------------------------------------------------------------------------------------------------
class BasicBlock(YdlModule):
    expansion = 1

    def __init__(self, in_channels, out_channels, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv(in_channels, out_channels, 3, stride, 1, act=True)
        self.conv2 = Conv(out_channels, out_channels, 3, 1, 1, act=False)
        self.downsample = downsample
        self.act = nn.ReLU(inplace=True)

    def _fwd(self, tape: Tape, x: Var) -> Var:
        out = self.conv1._fwd(tape, x)
        idt = x if self.downsample is None else self.downsample._fwd(tape, x)
        # relu(bn(conv2(out)) + identity) fused into conv2's apply kernel
        return self.conv2._fwd(tape, out, res=idt, res_mode=L.RES_BEFORE_ACT, act_code=L.ACT_RELU)


class BottleneckBlock(YdlModule):
    expansion = 4

    def __init__(self, in_channels, mid_channels, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv(in_channels, mid_channels, 1, 1, 0, act=True)
        self.conv2 = Conv(mid_channels, mid_channels, 3, stride, 1, act=True)
        self.conv3 = Conv(mid_channels, mid_channels * self.expansion, 1, 1, 0, act=False)
        self.downsample = downsample
        self.act = nn.ReLU(inplace=True)

    def _fwd(self, tape: Tape, x: Var) -> Var:
        out = self.conv2._fwd(tape, self.conv1._fwd(tape, x))
        idt = x if self.downsample is None else self.downsample._fwd(tape, x)
        return self.conv3._fwd(tape, out, res=idt, res_mode=L.RES_BEFORE_ACT, act_code=L.ACT_RELU)


class MaxPool2d(YdlModule):
    def __init__(self, kernel_size, stride=None, padding=0):
        super().__init__()
        self.k, self.s, self.p = kernel_size, stride or kernel_size, padding

    def _fwd(self, tape: Tape, x: Var) -> Var:
        return tape.maxpool(x, self.k, self.s, self.p)


class SegmentHead(YdlModule):
    """segment/train.py:159-210: lateral 1x1 -> 128, bilinear(align_corners=True) x2^i, cat, 3x3 -> 256, 1x1 -> nc."""
    takes_list = True

    def __init__(self, num_classes: int = 12, in_channels: List[int] = [256, 512, 1024]):
        super().__init__()
        self.num_classes = num_classes
        self.lateral_convs = nn.ModuleList()
        self.up_samples = nn.ModuleList()
        for i, c in enumerate(in_channels):
            self.lateral_convs.append(Conv(c, 128, 1, 1))
            self.up_samples.append(Upsample(scale_factor=2 ** i, mode="bilinear", align_corners=True))
        self.final_conv = nn.Sequential(Conv(128 * len(in_channels), 256, 3, 1), Conv(256, num_classes, 1, 1, act=False))

    def _fwd(self, tape: Tape, feats: Sequence[Var]) -> Var:
        if len(feats) != len(self.lateral_convs):
            raise ValueError(f"feature count mismatch: expected {len(self.lateral_convs)}, got {len(feats)}")
        feats = [tape.materialize(f) for f in feats]
        H, W = feats[0].H, feats[0].W
        cat = tape.new(feats[0].N, 128 * len(feats), H, W)
        for i, (f, lat, up) in enumerate(zip(feats, self.lateral_convs, self.up_samples)):
            sl = cat.slice(128 * i, 128 * (i + 1))
            if (f.H, f.W) == (H, W):
                lat._fwd(tape, f, out=sl)
                continue
            f = lat._fwd(tape, f)
            Ho, Wo = up._out_size(f)
            if (Ho, Wo) == (H, W):
                up._fwd(tape, f, out=sl)
            else:                                   # F.interpolate(size=target, align_corners=True) fallback
                f = up._fwd(tape, f)
                tape.resize(f, H, W, L.RESIZE_BILINEAR_AC, out=sl)
        return self.final_conv[1]._fwd(tape, self.final_conv[0]._fwd(tape, cat))


# ----------------------------------------------------------------------------------------------------------
# DCNv3 module and its YOLO wiring (models/ops_dcnv3/build/.../modules/dcnv3.py:50-136, "common and yolo.py":2-38)
# ----------------------------------------------------------------------------------------------------------
class _LinearOps(_GemmWeights):
    """a Linear as Tape.conv_bias sees it: the 1x1 case of _GemmWeights over ``self.weight`` [rows, in] and ``self.bias`` [rows] or
    None (the whole parameters: Linear) or over one row block of them (``_rows``: _InProj)"""
    _wname = "Linear"

    def _gemm_dims(self):
        return self.out_features, 1, self.in_features


class Linear(_LinearOps, YdlModule):
    """``nn.Linear`` over the channel dimension of an NHWC tensor (state_dict: weight [out, in], bias [out]) = a 1x1
    convolution with bias on the implicit-GEMM kernels; the bias gradient is a deterministic per-channel sum."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            bound = 1 / math.sqrt(in_features)
            nn.init.uniform_(self.bias, -bound, bound)
        self._wcache = {}

    def _fwd(self, tape: Tape, x: Var) -> Var:
        return tape.conv_bias(x, self)


def _lanes_per_group_channel_block(gc: int) -> int:
    """lanes one (pixel, group) item of the DCNv3 kernels occupies: the next power of two >= the group's channel count, at most a
    wavefront (csrc/dcnv3.hip: fill_args) — the idle share of those lanes is what a non-power-of-two head width costs here"""
    seg = 1
    while seg < gc and seg < 64:
        seg <<= 1
    return seg


class DCNv3(YdlModule):
    """modules/dcnv3.py:50-136.  Input and output are channels-last in the reference ((N, H, W, C)); inside a taped model
    every activation already is, so the permutes of ``DCNV3_YoLo.forward`` vanish.  Stand-alone calls take the
    reference's (N, H, W, C) tensor."""

    def __init__(self, channels=64, kernel_size=3, stride=1, pad=1, dilation=1, group=4, offset_scale=1.0,
                 act_layer="GELU", norm_layer="LN"):
        super().__init__()
        if channels % group != 0:
            raise ValueError(f"channels must be divisible by group, but got {channels} and {group}")
        gc = channels // group
        seg = _lanes_per_group_channel_block(gc)
        lanes = -(-gc // seg) * seg                # lanes x passes an item takes
        if lanes != gc:
            # (the reference warns at the same place, modules/dcnv3.py:75-79, about its own kernel; here the cost is idle lanes)
            import warnings
            warnings.warn(f"DCNv3: {gc} channels per group run as {lanes // seg} pass(es) of {seg}-lane segments in the HIP sampling "
                          f"kernels ({lanes - gc} of {lanes} lane slots idle); a power of two up to 64, or a multiple of 64, wastes none.")
        self.offset_scale = offset_scale
        self.channels = channels
        self.kernel_size = kernel_size
        self.stride = stride
        self.dilation = 1                 # the reference ignores its dilation argument (modules/dcnv3.py:82)
        self.pad = pad
        self.group = group
        self.group_channels = channels // group
        self.dw_conv = Conv(channels, channels, kernel_size, g=channels)
        self.offset = Linear(channels, group * kernel_size * kernel_size * 2)
        self.mask = Linear(channels, group * kernel_size * kernel_size)
        self.input_proj = Linear(channels, channels)
        self.output_proj = Linear(channels, channels)
        self._reset_parameters()

    def _reset_parameters(self):
        with torch.no_grad():
            self.offset.weight.zero_(); self.offset.bias.zero_()
            self.mask.weight.zero_(); self.mask.bias.zero_()
            nn.init.xavier_uniform_(self.input_proj.weight); self.input_proj.bias.zero_()
            nn.init.xavier_uniform_(self.output_proj.weight); self.output_proj.bias.zero_()

    def forward(self, x, *a, **kw):
        if isinstance(x, Var):
            return self._fwd(x.tape, x)
        # stand-alone: (N, H, W, C) in, (N, H, W, C) out like the reference module
        return run_region(self, [x.permute(0, 3, 1, 2)]).permute(0, 2, 3, 1)

    def _fwd(self, tape: Tape, inp: Var) -> Var:
        x = self.input_proj._fwd(tape, inp)
        x1 = self.dw_conv._fwd(tape, inp)
        offset = self.offset._fwd(tape, x1)
        P = self.kernel_size * self.kernel_size
        mask = tape.group_softmax(self.mask._fwd(tape, x1), self.group, P)
        y = tape.dcnv3(x, offset, mask, self.kernel_size, self.stride, self.pad, self.dilation, self.group,
                       self.group_channels, float(self.offset_scale))
        return self.output_proj._fwd(tape, y)


class DCNV3_YoLo(YdlModule):
    """"common and yolo.py":2-14: Conv(inc, ouc, k=1) -> DCNv3(ouc, kernel_size=k, stride=s, group=g, dilation=d)"""

    def __init__(self, inc, ouc, k=1, s=1, p=None, g=1, d=1, act=True):
        super().__init__()
        self.conv = Conv(inc, ouc, k=1)
        self.dcnv3 = DCNv3(ouc, kernel_size=k, stride=s, group=g, dilation=d)

    def _fwd(self, tape: Tape, x: Var) -> Var:
        return self.dcnv3._fwd(tape, self.conv._fwd(tape, x))


class Bottleneck_DCNV3(YdlModule):
    """"common and yolo.py":16-25"""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = DCNV3_YoLo(c_, c2, 3, 1, g=g)
        self.add = shortcut and c1 == c2

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        y = self.cv2._fwd(tape, self.cv1._fwd(tape, x))
        if self.add:
            y = tape.add(x, y)
        return y if out is None else tape.copy(y, out)


class C3_DCNV3(YdlModule):
    """"common and yolo.py":27-38: models/common.py C3 with Bottleneck_DCNV3 inner blocks (no outer residual)"""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(Bottleneck_DCNV3(c_, c_, shortcut, g, e=1.0) for _ in range(n)))
        self.c_ = c_

    def _fwd(self, tape: Tape, x: Var) -> Var:
        return _csp_forward(self, tape, x, False)


# ----------------------------------------------------------------------------------------------------------
# stand-alone local self-attention layers (models/common.py:1509-1627)
# ----------------------------------------------------------------------------------------------------------
class _Proj1x1(_BiasConv2d):
    """bias-free ``nn.Conv2d(c1, c2, kernel_size=1)``: one Q / K / V projection of a self-attention layer (weight [c2, c1, 1, 1], the
    layer's own ``reset_parameters`` initialisation is kept by the yaml models' kaiming pass)"""

    def __init__(self, c1, c2):
        super().__init__(c1, c2, kernel_size=1, bias=False)


class _LocalAttention(YdlModule):
    """what AttentionConv and AttentionStem share: the argument checks and the parameter-side hooks of Tape.local_attention"""

    def _init_common(self, in_channels, out_channels, kernel_size, stride, padding, groups, bias):
        name = type(self).__name__
        assert out_channels % groups == 0, "out_channels should be divided by groups. (example: out_channels: 40, groups: 4)"
        if stride != 1:
            raise NotImplementedError(f"{name}: stride {stride} is not implemented (the reference's forward only works for stride 1: "
                                      "its .view fails otherwise)")
        if kernel_size not in (1, 3, 5, 7):
            raise NotImplementedError(f"{name}: kernel_size {kernel_size} is not implemented (the HIP kernels serve 1, 3, 5 and 7)")
        if 2 * padding != kernel_size - 1:
            raise NotImplementedError(f"{name}: padding {padding} with kernel_size {kernel_size} is not implemented (the reference's "
                                      "forward only works for 2 * padding = kernel_size - 1)")
        if bias:
            raise NotImplementedError(f"{name}: bias=True is not implemented (a bias would make the padded positions non-zero)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.groups = kernel_size, stride, padding, groups

    @staticmethod
    def grad_of(p: nn.Parameter) -> torch.Tensor:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        return p.grad

    def rel(self):
        return None

    def table(self, tape: Tape):
        return None

    def table_trainable(self) -> bool:
        return False

    def _fwd(self, tape: Tape, x: Var) -> Var:
        return tape.local_attention(x, self)

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, "
                f"padding={self.padding}, groups={self.groups}")


class AttentionConv(_LocalAttention):
    """models/common.py:1509-1561.  Per channel and pixel a softmax over the k x k neighbourhood of q * (k + rel), applied to v;
    ``rel_h`` serves the first half of the channels (by window row), ``rel_w`` the second (by window column).  ``groups`` only
    reshapes in the reference and has no arithmetic effect."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=1, groups=1, bias=False):
        super().__init__()
        self._init_common(in_channels, out_channels, kernel_size, stride, padding, groups, bias)
        if out_channels % 2:
            raise NotImplementedError(f"AttentionConv: odd out_channels {out_channels} is not implemented (rel_h and rel_w each "
                                      "serve one half of the channels)")
        self.rel_h = nn.Parameter(torch.randn(out_channels // 2, 1, 1, kernel_size, 1), requires_grad=True)
        self.rel_w = nn.Parameter(torch.randn(out_channels // 2, 1, 1, 1, kernel_size), requires_grad=True)
        self.key_conv = _Proj1x1(in_channels, out_channels)
        self.query_conv = _Proj1x1(in_channels, out_channels)
        self.value_conv = _Proj1x1(in_channels, out_channels)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_normal_(self.key_conv.weight, mode="fan_out", nonlinearity="relu")
        nn.init.kaiming_normal_(self.value_conv.weight, mode="fan_out", nonlinearity="relu")
        nn.init.kaiming_normal_(self.query_conv.weight, mode="fan_out", nonlinearity="relu")
        nn.init.normal_(self.rel_h, 0, 1)
        nn.init.normal_(self.rel_w, 0, 1)

    def projections(self):
        return [self.query_conv, self.key_conv, self.value_conv]

    def rel(self):
        return self.rel_h, self.rel_w


class AttentionStem(_LocalAttention):
    """models/common.py:1563-1627.  ``m`` value projections mixed per window position by E = softmax over m of
    (emb_mix @ emb_a)[m, i] + (emb_mix @ emb_b)[m, j]; no positional term in the logits.  The reference's default ``padding=0``
    is a combination its own forward cannot run; the yaml files always pass ``[c2, 3, 1, 1]``."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, groups=1, m=4, bias=False):
        super().__init__()
        self._init_common(in_channels, out_channels, kernel_size, stride, padding, groups, bias)
        if not 1 <= m <= 8 or m * kernel_size * kernel_size > 196:
            raise NotImplementedError(f"AttentionStem: m={m} with kernel_size {kernel_size} is not implemented (the HIP kernels serve "
                                      "1 <= m <= 8 with m * kernel_size^2 <= 196)")
        self.m = m
        self.emb_a = nn.Parameter(torch.randn(out_channels // groups, kernel_size), requires_grad=True)
        self.emb_b = nn.Parameter(torch.randn(out_channels // groups, kernel_size), requires_grad=True)
        self.emb_mix = nn.Parameter(torch.randn(m, out_channels // groups), requires_grad=True)
        self.key_conv = _Proj1x1(in_channels, out_channels)
        self.query_conv = _Proj1x1(in_channels, out_channels)
        self.value_conv = nn.ModuleList([_Proj1x1(in_channels, out_channels) for _ in range(m)])
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_normal_(self.key_conv.weight, mode="fan_out", nonlinearity="relu")
        nn.init.kaiming_normal_(self.query_conv.weight, mode="fan_out", nonlinearity="relu")
        for v in self.value_conv:
            nn.init.kaiming_normal_(v.weight, mode="fan_out", nonlinearity="relu")
        nn.init.normal_(self.emb_a, 0, 1)
        nn.init.normal_(self.emb_b, 0, 1)
        nn.init.normal_(self.emb_mix, 0, 1)

    def projections(self):
        return [self.query_conv, self.key_conv, *self.value_conv]

    def _embs(self):
        return self.emb_mix, self.emb_a, self.emb_b

    def table(self, tape: Tape):
        """the mixing table E, f32 [m][k*k], recomputed from the parameters by one single-block launch per forward pass"""
        E = self.__dict__.get("_table")
        if E is None or E.device != self.emb_mix.device:
            E = self.__dict__["_table"] = torch.empty((self.m, self.kernel_size ** 2), dtype=torch.float32, device=self.emb_mix.device)
        mix, ea, eb = (p.detach() for p in self._embs())
        L.call("ydl_attn_stem_table_fwd", _p(mix), _p(ea), _p(eb), _p(E), self.m, mix.shape[1], self.kernel_size, _stream())
        return E

    def table_trainable(self) -> bool:
        return any(p.requires_grad for p in self._embs())

    def table_backward(self, tape: Tape, E: torch.Tensor, dE: torch.Tensor, st) -> None:
        mix, ea, eb = self._embs()
        # a frozen parameter's share lands in a scratch row
        gs = [self.grad_of(p) if p.requires_grad else zero_(torch.empty_like(p), st) for p in (mix, ea, eb)]
        L.call("ydl_attn_stem_table_bwd", _p(mix.detach()), _p(ea.detach()), _p(eb.detach()), _p(E), _p(dE), _p(gs[0]), _p(gs[1]), _p(gs[2]),
               self.m, mix.shape[1], self.kernel_size, st)
        tape._keep.extend(gs)
        for p in (mix, ea, eb):
            if p.requires_grad:
                config.mark_touched(p)


# ----------------------------------------------------------------------------------------------------------
# C3TR / TransformerBlock / TransformerLayer (models/common.py:79-112, :183-188): dense multi-head self-attention over the H*W
# positions of a sample (csrc/mha.hip) between Linear layers on the implicit-GEMM kernels
# ----------------------------------------------------------------------------------------------------------
MHA_HEAD_DIM_STEP, MHA_HEAD_DIM_MAX = 8, 128          # ydl_mha_fwd: d a multiple of 8, 8 <= d <= 128


class _InProj(_LinearOps):
    """rows [i*c, (i+1)*c) of ``ma.in_proj_weight`` / ``ma.in_proj_bias`` seen as one Linear by Tape.conv_bias: the compute-layout
    copy is derived from the row block, and the weight and bias gradients are written into the matching contiguous slices of the
    two parameters' gradients.  TransformerLayer runs the blocks in the order Q, K, V, so the backward reaches block 0 last: it
    alone is ``final``."""

    def __init__(self, ma: "_MultiheadAttention", i: int):
        self.ma, self.i = ma, i
        self.in_features = self.out_features = ma.embed_dim
        self._rows = slice(i * ma.embed_dim, (i + 1) * ma.embed_dim)
        self.final = i == 0
        self._wcache = {}

    @property
    def weight(self) -> nn.Parameter:
        return self.ma.in_proj_weight

    @property
    def bias(self) -> nn.Parameter:
        return self.ma.in_proj_bias


class _MultiheadAttention(nn.Module):
    """parameter holder with ``nn.MultiheadAttention``'s names, shapes and initialisation: ``in_proj_weight`` [3c, c] (xavier
    uniform), ``in_proj_bias`` [3c] (zero), ``out_proj`` = Linear(c, c) with a zero bias.  The arithmetic is Tape.mha."""

    def __init__(self, embed_dim: int, num_heads: int):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.out_proj.bias, 0.0)
        self.__dict__["_blocks"] = [_InProj(self, i) for i in range(3)]

    def blocks(self):
        return self.__dict__["_blocks"]

    def forward(self, *a, **kw):  # pragma: no cover - run through TransformerLayer
        raise RuntimeError("_MultiheadAttention holds parameters only; call the TransformerLayer")


class TransformerLayer(YdlModule):
    """models/common.py:79-93: x1 = out_proj(MHA(in_q(q x), in_k(k x), in_v(v x))) + x;  out = fc2(fc1(x1)) + x1 (no LayerNorm).
    The tokens of a sample are its H*W positions."""

    def __init__(self, c, num_heads):
        super().__init__()
        if c % num_heads:
            raise AssertionError("embed_dim must be divisible by num_heads")
        d = c // num_heads
        if d % MHA_HEAD_DIM_STEP or not MHA_HEAD_DIM_STEP <= d <= MHA_HEAD_DIM_MAX:
            raise NotImplementedError(f"TransformerLayer: head dimension {d} (c={c}, num_heads={num_heads}) is not implemented: the "
                                      f"HIP attention kernels serve multiples of {MHA_HEAD_DIM_STEP} between {MHA_HEAD_DIM_STEP} and "
                                      f"{MHA_HEAD_DIM_MAX}")
        self.c, self.num_heads = c, num_heads
        self.q = Linear(c, c, bias=False)
        self.k = Linear(c, c, bias=False)
        self.v = Linear(c, c, bias=False)
        self.ma = _MultiheadAttention(c, num_heads)
        self.fc1 = Linear(c, c, bias=False)
        self.fc2 = Linear(c, c, bias=False)

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        if x.C != self.c:
            raise RuntimeError(f"TransformerLayer input channel mismatch: got {x.C}, weights expect {self.c}")
        x = tape._flat(x)
        c = self.c
        t = tape.new(x.N, 3 * c, x.H, x.W)           # [pix][q x | k x | v x]
        qkv = tape.new(x.N, 3 * c, x.H, x.W)         # [pix][Q | K | V]
        for i, (lin, blk) in enumerate(zip((self.q, self.k, self.v), self.ma.blocks())):
            a = tape.conv_bias(x, lin, out=t.slice(i * c, (i + 1) * c))
            tape.conv_bias(a, blk, out=qkv.slice(i * c, (i + 1) * c))
        att = tape.mha(qkv, self.num_heads)
        x1 = tape.add(tape.conv_bias(att, self.ma.out_proj), x)
        return tape.add(tape.conv_bias(tape.conv_bias(x1, self.fc1), self.fc2), x1, out=out)


class TransformerBlock(YdlModule):
    """models/common.py:96-112: optional Conv(c1, c2), the learnable position embedding p + linear(p), then ``num_layers``
    TransformerLayers."""

    def __init__(self, c1, c2, num_heads, num_layers):
        super().__init__()
        self.conv = None
        if c1 != c2:
            self.conv = Conv(c1, c2)
        self.linear = Linear(c2, c2)
        self.tr = nn.Sequential(*(TransformerLayer(c2, num_heads) for _ in range(num_layers)))
        self.c2 = c2

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        if self.conv is not None:
            x = self.conv._fwd(tape, x)
        n = len(self.tr)
        x = tape.add(x, tape.conv_bias(x, self.linear), out=out if n == 0 else None)
        for i, layer in enumerate(self.tr):
            x = layer._fwd(tape, x, out=out if i == n - 1 else None)
        return x


class C3TR(C3Common):
    """models/common.py:183-188: C3 whose ``m`` is one TransformerBlock(c_, c_, 4, n)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = TransformerBlock(self.c_, self.c_, 4, n)

    def _fwd(self, tape: Tape, x: Var) -> Var:
        c_ = self.c_
        cat = tape.new(x.N, 2 * c_, x.H, x.W)
        left, right = cat.slice(0, c_), cat.slice(c_, 2 * c_)
        self.m._fwd(tape, self.cv1._fwd(tape, x), out=left)
        self.cv2._fwd(tape, x, out=right)
        return self.cv3._fwd(tape, cat)


# ----------------------------------------------------------------------------------------------------------
# ConvNeXt Tiny backbone rows (models/common.py:1241-1269: the slices features[:4], [4:6], [6:8] of torchvision's convnext_tiny).
# torchvision is not a dependency: its definition is restated here with its state_dict keys, so a user's own state_dict loads.
# ----------------------------------------------------------------------------------------------------------
class LayerNorm2d(YdlModule):
    """LayerNorm over the channels of an (N, C, H, W) tensor (torchvision's LayerNorm2d; inside a CNBlock, ``nn.LayerNorm(C)`` between
    the two permutes): parameters ``weight``, ``bias``.  One launch each way on the NHWC rows (Tape.layer_norm), C a multiple of 8 up
    to 1024.  The class name contains "Norm": ``smart_optimizer`` keeps its weight out of the decayed group."""
    _keep_init = True

    def __init__(self, normalized_shape, eps=1e-6):
        super().__init__()
        C = normalized_shape[0] if isinstance(normalized_shape, (list, tuple)) and len(normalized_shape) == 1 else normalized_shape
        if isinstance(C, bool) or not isinstance(C, int) or C < 8 or C > 1024 or C % 8:
            raise ValueError(f"LayerNorm2d: normalized_shape={normalized_shape!r} must be one channel count, a multiple of 8 in 8..1024")
        self.normalized_shape, self.eps = (C,), float(eps)
        self.weight = nn.Parameter(torch.ones(C))
        self.bias = nn.Parameter(torch.zeros(C))

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None, pre_bias=None) -> Var:
        return tape.layer_norm(x, self, pre_bias=pre_bias, out=out)

    def extra_repr(self):
        return f"{self.normalized_shape}, eps={self.eps}"


class _PatchConv2d(_GemmWeights, nn.Conv2d):
    """``nn.Conv2d(c1, c2, k, k, bias=True)``, a patchify convolution: run as space-to-depth and a 1x1 GEMM over k*k*c1 channels
    (Tape.patch_conv).  The weight [c2, c1, k, k] in channels_last storage is that GEMM's [c2][1][k*k*c1] master as it stands."""
    _keep_init = True
    _wname = "patch Conv2d"

    def __init__(self, c1, c2, k):
        super().__init__(c1, c2, k, k)
        self.weight.data = self.weight.data.contiguous(memory_format=torch.channels_last)
        nn.init.trunc_normal_(self.weight, std=0.02)
        nn.init.zeros_(self.bias)
        self.patch = k
        self._wcache = {}

    def _krsc(self, t: torch.Tensor) -> torch.Tensor:
        if t.dim() == 4:
            t = t.permute(0, 2, 3, 1)
            if not t.is_contiguous():
                return t                      # _master_krsc re-homes the parameter; a gradient laid out otherwise is refused by wgrad
            return t.view(t.shape[0], 1, -1)
        return t

    def _gemm_dims(self):
        return self.out_channels, 1, self.patch * self.patch * self.in_channels

    def forward(self, x):
        if isinstance(x, Var):
            return self._fwd(x.tape, x)
        return run_region(self, [x])

    def _fwd(self, tape: Tape, x: Var, out: Optional[Var] = None) -> Var:
        k = self.patch
        if x.LH % k or x.LW % k:
            raise ValueError(f"Conv2d({self.in_channels}, {self.out_channels}, {k}, {k}): the {x.LH} x {x.LW} map is not a multiple of {k}")
        return tape.patch_conv(x, self, out=out)


_PatchConv2d.takes_list = False


class _DWConv2d(nn.Conv2d):
    """``nn.Conv2d(C, C, 7, padding=3, groups=C, bias=True)`` of a CNBlock: the weight [C, 1, k, k] is the [C][k*k] master the depth-wise
    kernels read (Tape.dw_conv); the bias is applied by the LayerNorm behind it."""
    _keep_init = True

    def __init__(self, dim, k=7):
        super().__init__(dim, dim, k, padding=k // 2, groups=dim)
        nn.init.trunc_normal_(self.weight, std=0.02)
        nn.init.zeros_(self.bias)
        self.k = k

    def master_dw(self) -> torch.Tensor:
        w = self.weight.detach().permute(0, 2, 3, 1)
        return w if w.is_contiguous() else w.contiguous()

    def grad_dw(self) -> torch.Tensor:
        if self.weight.grad is None:
            self.weight.grad = torch.zeros_like(self.weight)
        g = self.weight.grad.permute(0, 2, 3, 1)
        if not g.is_contiguous():
            raise RuntimeError("CNBlock depth-wise weight gradient must be [C][k*k]-contiguous")
        return g

    def forward(self, x):  # pragma: no cover - run through CNBlock
        raise RuntimeError("run through CNBlock")


class _CNLinear(Linear):
    """a CNBlock's Linear: torchvision's init (trunc_normal 0.02, zero bias)"""

    def __init__(self, in_features, out_features):
        super().__init__(in_features, out_features)
        nn.init.trunc_normal_(self.weight, std=0.02)
        nn.init.zeros_(self.bias)


class CNBlock(YdlModule):
    """torchvision's CNBlock: ``x + stochastic_depth(layer_scale * fc2(GELU(fc1(LayerNorm(dwconv7x7(x))))))``, stochastic depth in "row"
    mode.  state_dict: block.0 (depth-wise conv, weight [dim,1,7,7] and bias), block.2 (LayerNorm, eps 1e-6), block.3 (Linear dim ->
    4 dim), block.5 (Linear 4 dim -> dim), layer_scale [dim,1,1]; block.1 / .4 / .6 hold no state (the permutes and the GELU).

    Launches: the depth-wise kernel without bias; LayerNorm, which adds that bias on the way in; the fc1 GEMM without bias; bias + erf
    GELU; the fc2 GEMM with bias; the layer-scaled residual, which takes the per-sample keep factors."""
    _keep_init = True

    def __init__(self, dim, layer_scale=1e-6, stochastic_depth_prob=0.0):
        super().__init__()
        if isinstance(dim, bool) or not isinstance(dim, int) or dim < 8 or dim > 1024 or dim % 8:
            raise ValueError(f"CNBlock: dim={dim!r} must be a multiple of 8 in 8..1024")
        p = float(stochastic_depth_prob)
        if not 0.0 <= p < 1.0:
            raise ValueError(f"CNBlock: stochastic_depth_prob={stochastic_depth_prob!r} must be in [0, 1)")
        self.block = nn.Sequential(_DWConv2d(dim), nn.Identity(), LayerNorm2d(dim, eps=1e-6), _CNLinear(dim, 4 * dim), nn.Identity(),
                                   _CNLinear(4 * dim, dim), nn.Identity())
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * layer_scale)
        self.stochastic_depth_prob = p
        self.generator = None             # torch.Generator of the keep draws, or None for the device's default generator

    def draw_keep(self, N: int, device) -> Optional[torch.Tensor]:
        """the per-sample keep factors bernoulli(1 - p) / (1 - p) of this forward as an f32 [N] tensor on the device, or None (eval, p = 0)"""
        p = self.stochastic_depth_prob
        if not self.training or p == 0.0:
            return None
        if L.recorder() is not None:
            raise NotImplementedError(f"stochastic depth ({type(self).__name__} with stochastic_depth_prob > 0 in training) draws its keep factors with "
                                      "torch before the launch: a recorded step cannot replay it; build the rows with stochastic_depth_prob=0")
        keep = torch.empty(N, dtype=torch.float32, device=device).bernoulli_(1.0 - p, generator=self.generator)
        return keep.div_(1.0 - p)

    def _fwd(self, tape: Tape, x: Var) -> Var:
        dw, ln, fc1, fc2 = self.block[0], self.block[2], self.block[3], self.block[5]
        x = tape.materialize(x)
        keep = self.draw_keep(x.N, tape.device)
        t = tape.dw_conv(x, dw)
        t = tape.layer_norm(t, ln, pre_bias=dw.bias)
        t = tape.conv_bias(t, fc1, bias=False)
        t = tape.bias_gelu(t, fc1)
        t = tape.conv_bias(t, fc2)
        return tape.scale_residual(t, self, keep, x)

    def extra_repr(self):
        return f"stochastic_depth_prob={self.stochastic_depth_prob:.4g}"


def refuse_stochastic_depth(model: nn.Module, who: str) -> None:
    """the recorded-step paths re-issue one step's launches: the keep factors of stochastic depth are drawn by torch before the launch,
    every step anew, which a recording cannot repeat"""
    bad = [n for n, m in model.named_modules() if isinstance(m, (CNBlock, MBConv)) and m.training and m.stochastic_depth_prob > 0.0
           and getattr(m, "use_res_connect", True)]
    if bad:
        raise NotImplementedError(f"{who} cannot re-draw the keep factors of stochastic depth: {len(bad)} CNBlock / MBConv block(s) in training mode have "
                                  f"stochastic_depth_prob > 0 (first: {bad[0]}); build the rows with stochastic_depth_prob=0")


_CN_DIMS, _CN_DEPTHS = (96, 192, 384, 768), (3, 3, 9, 3)


def _cn_stage(i: int, sd: float, ls: float) -> nn.Sequential:
    """stage i of convnext_tiny: block j of the 18 (counted over the whole network) gets p = sd * j / 17"""
    first, total = sum(_CN_DEPTHS[:i]), sum(_CN_DEPTHS)
    return nn.Sequential(*(CNBlock(_CN_DIMS[i], ls, sd * (first + j) / (total - 1.0)) for j in range(_CN_DEPTHS[i])))


def _cn_down(i: int) -> nn.Sequential:
    return nn.Sequential(LayerNorm2d(_CN_DIMS[i - 1]), _PatchConv2d(_CN_DIMS[i - 1], _CN_DIMS[i], 2))


class _ConvNeXtRow(YdlModule):
    """one of the three rows: ``self.model`` is the slice of torchvision's ``convnext_tiny().features`` the reference keeps; the row's
    positional argument (the yaml's channel count) is ignored, as in the reference"""
    _keep_init = True
    _first = 0          # index in ``features`` of model.0
    _stride = 2         # the row's total down-sampling

    def __init__(self, ignore=None, *, stochastic_depth_prob=0.1, layer_scale=1e-6):
        super().__init__()
        self.model = nn.Sequential(*self._parts(float(stochastic_depth_prob), float(layer_scale)))

    def _fwd(self, tape: Tape, x: Var) -> Var:
        if x.LH % self._stride or x.LW % self._stride:
            raise ValueError(f"{type(self).__name__}: the {x.LH} x {x.LW} map is not a multiple of {self._stride}, the row's stride")
        for part in self.model:
            for sub in part:
                x = sub._fwd(tape, x)
        return x


class convnext_tiny1(_ConvNeXtRow):
    """models/common.py:1241-1249: features[:4] = stem (Conv2d(3, 96, 4, 4) + LayerNorm2d), 3 x CNBlock(96), LayerNorm2d + Conv2d(96, 192,
    2, 2), 3 x CNBlock(192): 3 -> 192 channels at 1/8 of the input size"""
    _stride = 8

    def _parts(self, sd, ls):
        return [nn.Sequential(_PatchConv2d(3, 96, 4), LayerNorm2d(96)), _cn_stage(0, sd, ls), _cn_down(1), _cn_stage(1, sd, ls)]


class convnext_tiny2(_ConvNeXtRow):
    """models/common.py:1251-1259: features[4:6] = LayerNorm2d + Conv2d(192, 384, 2, 2), 9 x CNBlock(384)"""
    _first = 4

    def _parts(self, sd, ls):
        return [_cn_down(2), _cn_stage(2, sd, ls)]


class convnext_tiny3(_ConvNeXtRow):
    """models/common.py:1261-1269: features[6:8] = LayerNorm2d + Conv2d(384, 768, 2, 2), 3 x CNBlock(768)"""
    _first = 6

    def _parts(self, sd, ls):
        return [_cn_down(3), _cn_stage(3, sd, ls)]


def convnext_key_map(keys=None) -> dict:
    """torchvision ``convnext_tiny`` state_dict key -> (row index 0..2, key inside that row): ``features.N.rest`` belongs to row 0 for
    N < 4, row 1 for N in (4, 5), row 2 for N in (6, 7), as ``model.M.rest`` with M = N, N - 4, N - 6.  ``keys``: the keys to map (the
    classifier's are left out); default: every key of the three rows.  Nothing is downloaded: the state_dict is the user's own."""
    rows = (convnext_tiny1, convnext_tiny2, convnext_tiny3)
    if keys is None:
        keys = [f"features.{r._first + int(k.split('.')[1])}.{k.split('.', 2)[2]}" for r in rows for k in r().state_dict()]
    out = {}
    for k in keys:
        parts = k.split(".", 2)
        if len(parts) != 3 or parts[0] != "features" or not parts[1].isdigit() or int(parts[1]) > 7:
            continue
        n = int(parts[1])
        row = 0 if n < 4 else 1 if n < 6 else 2
        out[k] = (row, f"model.{n - rows[row]._first}.{parts[2]}")
    return out


__all__ += ["LayerNorm2d", "CNBlock", "convnext_tiny1", "convnext_tiny2", "convnext_tiny3", "convnext_key_map"]


# ----------------------------------------------------------------------------------------------------------
# Squeeze-excitation blocks: the MobileNetV3-small and EfficientNet-B0 backbone rows (models/common.py:870-936: slices of torchvision's
# ``mobilenet_v3_small().features`` and ``efficientnet_b0().features``).  torchvision is not a dependency: its definitions are restated
# here with its state_dict keys, so a user's own state_dict loads.  Nothing is downloaded: the reference's ``pretrained=True`` is not
# reproduced, the initialisation is the builder's (torchvision's rule: kaiming fan-out, zero biases, BatchNorm 1 / 0).
# ----------------------------------------------------------------------------------------------------------
_SE_ACTS = {"relu": (nn.ReLU, L.ACT_RELU), "silu": (nn.SiLU, L.ACT_SILU)}
_SE_GATES = {"sigmoid": (nn.Sigmoid, L.SE_GATE_SIGMOID), "hardsigmoid": (nn.Hardsigmoid, L.SE_GATE_HSIGMOID)}


def _se_choice(what: str, v, table: dict):
    """``v``: a name of ``table``, the torch class it stands for, or an instance of that class -> (module, code)"""
    for name, (cls, code) in table.items():
        if v is cls or isinstance(v, cls) or (isinstance(v, str) and v.lower() == name):
            return cls(), code
    raise NotImplementedError(f"SqueezeExcitation: {what}={v!r} is not served (one of {', '.join(sorted(table))})")


class _SEConv2d(nn.Conv2d):
    """fc1 / fc2 of a SqueezeExcitation: a 1x1 ``nn.Conv2d`` with bias; the kernels read its f32 parameters as they stand"""
    _keep_init = True

    def __init__(self, c1, c2):
        super().__init__(c1, c2, 1)
        nn.init.kaiming_normal_(self.weight, mode="fan_out")
        nn.init.zeros_(self.bias)

    def forward(self, x):  # pragma: no cover - run through SqueezeExcitation
        raise RuntimeError("run through SqueezeExcitation")


class SqueezeExcitation(YdlModule):
    """torchvision's SqueezeExcitation: ``x * scale_activation(fc2(activation(fc1(avgpool(x)))))``.  state_dict: fc1.weight
    [squeeze, input, 1, 1], fc1.bias, fc2.weight [input, squeeze, 1, 1], fc2.bias.  ``activation``: "relu" or "silu" (or nn.ReLU /
    nn.SiLU), ``scale_activation``: "sigmoid" or "hardsigmoid" (or the torch classes).  Runs on the kernels of csrc/se.hip
    (Tape.squeeze_excite): input_channels a multiple of 8 in 8..2048, squeeze_channels in 1..512."""

    def __init__(self, input_channels, squeeze_channels, activation="relu", scale_activation="sigmoid"):
        super().__init__()
        C, Cs = input_channels, squeeze_channels
        if any(isinstance(v, bool) or not isinstance(v, int) for v in (C, Cs)) or C < 8 or C > 2048 or C % 8 or not 1 <= Cs <= 512:
            raise ValueError(f"SqueezeExcitation: input_channels={C!r} must be a multiple of 8 in 8..2048 and squeeze_channels={Cs!r} in 1..512")
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = _SEConv2d(C, Cs)
        self.fc2 = _SEConv2d(Cs, C)
        self.activation, self.act_code = _se_choice("activation", activation, _SE_ACTS)
        self.scale_activation, self.gate_code = _se_choice("scale_activation", scale_activation, _SE_GATES)

    def _fwd(self, tape: Tape, x: Var) -> Var:
        return tape.squeeze_excite(x, self)


_CNA_ACTS = {"relu": nn.ReLU, "re": nn.ReLU, "hardswish": nn.Hardswish, "hs": nn.Hardswish, "silu": nn.SiLU}


class Conv2dNormActivation(Conv):
    """torchvision's Conv2dNormActivation: Conv2d without bias, BatchNorm2d, activation, padding (k - 1) / 2.  A ``Conv`` whose
    convolution and BatchNorm sit under torchvision's names: state_dict ``0.weight`` and ``1.{weight, bias, running_mean, running_var,
    num_batches_tracked}`` (the activation, ``2``, holds no state).  ``conv`` / ``bn`` / ``act`` stay readable, so the tape, ``fuse()``,
    the optimizer arenas and the checkpoint code see an ordinary Conv.  ``activation``: "relu", "hardswish", "silu" (or "RE" / "HS", or
    the torch class or an instance), or None for none.  groups: 1, or in_channels == out_channels (depth-wise, k in {1, 3, 5, 7})."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, groups=1, activation="relu", eps=1e-5, momentum=0.1):
        act = activation
        if isinstance(act, str):
            if act.lower() not in _CNA_ACTS:
                raise NotImplementedError(f"Conv2dNormActivation: activation={activation!r} is not served (one of relu, hardswish, silu, None)")
            act = _CNA_ACTS[act.lower()]()
        elif isinstance(act, type):
            act = act()
        super().__init__(in_channels, out_channels, kernel_size, stride, None, groups, 1, act if act is not None else False)
        mods = self._modules
        conv, bn, a = mods.pop("conv"), mods.pop("bn"), mods.pop("act")
        mods["0"], mods["1"], mods["2"] = conv, bn, a
        conv._keep_init = True
        nn.init.kaiming_normal_(conv.weight, mode="fan_out")
        bn.eps, bn.momentum = float(eps), float(momentum)

    def _named(self, new: str, old: str):
        mods = self._modules
        return mods[new] if new in mods else mods[old]

    conv = property(lambda self: self._named("0", "conv"))
    bn = property(lambda self: self._named("1", "bn"))
    act = property(lambda self: self._named("2", "act"))


def _make_divisible_tv(v: float, divisor: int = 8) -> int:
    """torchvision's ``_make_divisible``: the nearest multiple, never below 90 % of ``v``"""
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def _block_ints(who: str, **kw) -> None:
    for k, v in kw.items():
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{who}: {k}={v!r} must be a positive int")


class InvertedResidual(YdlModule):
    """torchvision's MobileNetV3 ``InvertedResidual``: ``block`` = [expand 1x1 Conv+BN+act if expanded != in], depth-wise k x k stride s
    Conv+BN+act, [SqueezeExcitation(expanded, make_divisible(expanded // 4, 8), ReLU, Hardsigmoid)], project 1x1 Conv+BN; the residual
    ``x + block(x)`` where s == 1 and in == out (joined in the projection's BatchNorm apply).  ``activation``: "RE" (ReLU) or "HS"
    (Hardswish).  BatchNorm eps 1e-3, momentum 0.01, as ``mobilenet_v3_small`` builds it."""

    def __init__(self, in_channels, kernel, expanded_channels, out_channels, use_se, activation, stride):
        super().__init__()
        who = "InvertedResidual"
        _block_ints(who, in_channels=in_channels, kernel=kernel, expanded_channels=expanded_channels, out_channels=out_channels, stride=stride)
        if stride not in (1, 2) or kernel not in (1, 3, 5, 7) or str(activation).upper() not in ("RE", "HS"):
            raise NotImplementedError(f"{who}: stride={stride} in {{1, 2}}, kernel={kernel} in {{1, 3, 5, 7}}, activation={activation!r} 'RE' or 'HS'")
        bn = dict(eps=1e-3, momentum=0.01)
        act = str(activation).upper()
        layers = []
        if expanded_channels != in_channels:
            layers.append(Conv2dNormActivation(in_channels, expanded_channels, 1, activation=act, **bn))
        layers.append(Conv2dNormActivation(expanded_channels, expanded_channels, kernel, stride, expanded_channels, activation=act, **bn))
        if use_se:
            layers.append(SqueezeExcitation(expanded_channels, _make_divisible_tv(expanded_channels // 4, 8), "relu", "hardsigmoid"))
        layers.append(Conv2dNormActivation(expanded_channels, out_channels, 1, activation=None, **bn))
        self.block = nn.Sequential(*layers)
        self.use_res_connect = stride == 1 and in_channels == out_channels
        self.out_channels = out_channels

    def _fwd(self, tape: Tape, x: Var) -> Var:
        x = tape.materialize(x)
        h = x
        for sub in self.block[:-1]:
            h = sub._fwd(tape, h)
        if self.use_res_connect:
            return self.block[-1]._fwd(tape, h, res=x, res_mode=L.RES_AFTER_ACT)
        return self.block[-1]._fwd(tape, h)


class MBConv(YdlModule):
    """torchvision's EfficientNet ``MBConv``: ``block`` = [expand 1x1 Conv+BN+SiLU if expand_ratio != 1], depth-wise k x k stride s
    Conv+BN+SiLU, SqueezeExcitation(expanded, max(1, in // 4), SiLU, Sigmoid), project 1x1 Conv+BN; where s == 1 and in == out the
    residual ``x + stochastic_depth(block(x))``, "row" mode.  Without keep factors (eval, p = 0) the projection's BatchNorm apply joins
    the residual; with them the keep-factor kernel of the ConvNeXt blocks does (a sample with keep 0 leaves as it came, bit for bit)."""

    def __init__(self, expand_ratio, kernel, stride, in_channels, out_channels, stochastic_depth_prob=0.0):
        super().__init__()
        who = "MBConv"
        _block_ints(who, expand_ratio=expand_ratio, kernel=kernel, stride=stride, in_channels=in_channels, out_channels=out_channels)
        if stride not in (1, 2) or kernel not in (1, 3, 5, 7):
            raise NotImplementedError(f"{who}: stride={stride} in {{1, 2}}, kernel={kernel} in {{1, 3, 5, 7}}")
        p = float(stochastic_depth_prob)
        if not 0.0 <= p < 1.0:
            raise ValueError(f"{who}: stochastic_depth_prob={stochastic_depth_prob!r} must be in [0, 1)")
        exp = in_channels * expand_ratio
        layers = []
        if exp != in_channels:
            layers.append(Conv2dNormActivation(in_channels, exp, 1, activation="silu"))
        layers.append(Conv2dNormActivation(exp, exp, kernel, stride, exp, activation="silu"))
        layers.append(SqueezeExcitation(exp, max(1, in_channels // 4), "silu", "sigmoid"))
        layers.append(Conv2dNormActivation(exp, out_channels, 1, activation=None))
        self.block = nn.Sequential(*layers)
        self.use_res_connect = stride == 1 and in_channels == out_channels
        self.out_channels = out_channels
        self.stochastic_depth_prob = p
        self.generator = None             # torch.Generator of the keep draws, or None for the device's default generator

    draw_keep = CNBlock.draw_keep

    def _fwd(self, tape: Tape, x: Var) -> Var:
        x = tape.materialize(x)
        keep = self.draw_keep(x.N, tape.device) if self.use_res_connect else None
        h = x
        for sub in self.block[:-1]:
            h = sub._fwd(tape, h)
        if not self.use_res_connect:
            return self.block[-1]._fwd(tape, h)
        if keep is None:
            return self.block[-1]._fwd(tape, h, res=x, res_mode=L.RES_AFTER_ACT)
        ones = self.__dict__.get("_ones")
        if ones is None or ones.device != x.t.device:      # the constant gamma row of the keep-factor kernel, made once
            ones = self.__dict__["_ones"] = torch.ones(self.out_channels, dtype=torch.float32, device=x.t.device)
        return tape.scale_residual(self.block[-1]._fwd(tape, h), None, keep, x, gamma=ones)

    def extra_repr(self):
        return f"stochastic_depth_prob={self.stochastic_depth_prob:.4g}"


# mobilenet_v3_small: features[1..11] as (in, kernel, expanded, out, SE, activation, stride)
_MNV3S = ((16, 3, 16, 16, True, "RE", 2), (16, 3, 72, 24, False, "RE", 2), (24, 3, 88, 24, False, "RE", 1), (24, 5, 96, 40, True, "HS", 2),
          (40, 5, 240, 40, True, "HS", 1), (40, 5, 240, 40, True, "HS", 1), (40, 5, 120, 48, True, "HS", 1), (48, 5, 144, 48, True, "HS", 1),
          (48, 5, 288, 96, True, "HS", 2), (96, 5, 576, 96, True, "HS", 1), (96, 5, 576, 96, True, "HS", 1))
# efficientnet_b0: stages features[1..7] as (expand ratio, kernel, stride of the first block, in, out, repeats)
_EFFB0 = ((1, 3, 1, 32, 16, 1), (6, 3, 2, 16, 24, 2), (6, 5, 2, 24, 40, 2), (6, 3, 2, 40, 80, 3), (6, 5, 1, 80, 112, 3),
          (6, 5, 2, 112, 192, 4), (6, 3, 1, 192, 320, 1))


def _mnv3s_feature(i: int) -> nn.Module:
    bn = dict(eps=1e-3, momentum=0.01)
    if i == 0:
        return Conv2dNormActivation(3, 16, 3, 2, activation="hardswish", **bn)
    if i == 12:
        return Conv2dNormActivation(96, 576, 1, activation="hardswish", **bn)
    return InvertedResidual(*_MNV3S[i - 1])


def _effb0_feature(i: int, sd: float) -> nn.Module:
    """block j of the 16 (counted over the whole network) gets p = sd * j / 16"""
    if i == 0:
        return Conv2dNormActivation(3, 32, 3, 2, activation="silu")
    if i == 8:
        return Conv2dNormActivation(320, 1280, 1, activation="silu")
    ratio, k, s, cin, cout, reps = _EFFB0[i - 1]
    first, total = sum(st[5] for st in _EFFB0[:i - 1]), sum(st[5] for st in _EFFB0)
    return nn.Sequential(*(MBConv(ratio, k, s if j == 0 else 1, cin if j == 0 else cout, cout, sd * (first + j) / total) for j in range(reps)))


class _SERow(YdlModule):
    """one backbone row: ``self.model`` is the slice ``features[_first:_last]`` the reference keeps, so the keys are ``model.<j>. ...``;
    the row's positional argument (the yaml's channel count) is ignored, as in the reference"""
    _first, _last = 0, 0
    _stride = 2         # the row's total down-sampling

    def _fwd(self, tape: Tape, x: Var) -> Var:
        if x.LH % self._stride or x.LW % self._stride:
            raise ValueError(f"{type(self).__name__}: the {x.LH} x {x.LW} map is not a multiple of {self._stride}, the row's stride")
        for part in self.model:
            for sub in (part if isinstance(part, nn.Sequential) else (part,)):
                x = sub._fwd(tape, x)
        return x


class _MobileNetV3sRow(_SERow):
    def __init__(self, ignore=None):
        super().__init__()
        self.model = nn.Sequential(*(_mnv3s_feature(i) for i in range(self._first, self._last)))


class MobileNetV3s1(_MobileNetV3sRow):
    """models/common.py:870-880: features[:4] of mobilenet_v3_small, 3 -> 24 channels at 1/8 of the input size"""
    _first, _last, _stride = 0, 4, 8


class MobileNetV3s2(_MobileNetV3sRow):
    """models/common.py:882-892: features[4:9], 24 -> 48 channels, 1/16"""
    _first, _last = 4, 9


class MobileNetV3s3(_MobileNetV3sRow):
    """models/common.py:894-903: features[9:], 48 -> 576 channels, 1/32"""
    _first, _last = 9, 13


class _EfficientNetB0Row(_SERow):
    def __init__(self, ignore=None, *, stochastic_depth_prob=0.2):
        super().__init__()
        sd = float(stochastic_depth_prob)
        if not 0.0 <= sd < 1.0:
            raise ValueError(f"{type(self).__name__}: stochastic_depth_prob={stochastic_depth_prob!r} must be in [0, 1)")
        self.model = nn.Sequential(*(_effb0_feature(i, sd) for i in range(self._first, self._last)))


class efficientnet_b01(_EfficientNetB0Row):
    """models/common.py:908-916: features[:4] of efficientnet_b0, 3 -> 40 channels at 1/8 of the input size"""
    _first, _last, _stride = 0, 4, 8


class efficientnet_b02(_EfficientNetB0Row):
    """models/common.py:918-926: features[4:6], 40 -> 112 channels, 1/16"""
    _first, _last = 4, 6


class efficientnet_b03(_EfficientNetB0Row):
    """models/common.py:928-936: features[6:], 112 -> 1280 channels, 1/32"""
    _first, _last = 6, 9


def _features_key_map(rows, keys) -> dict:
    """torchvision ``features.N.rest`` -> (row index, ``model.M.rest``) with M = N minus the row's first feature"""
    if keys is None:
        keys = [f"features.{r._first + int(k.split('.')[1])}.{k.split('.', 2)[2]}" for r in rows for k in r().state_dict()]
    out = {}
    for k in keys:
        parts = k.split(".", 2)
        if len(parts) != 3 or parts[0] != "features" or not parts[1].isdigit():
            continue
        n = int(parts[1])
        for i, r in enumerate(rows):
            if r._first <= n < r._last:
                out[k] = (i, f"model.{n - r._first}.{parts[2]}")
    return out


def mobilenet_v3_small_key_map(keys=None) -> dict:
    """torchvision ``mobilenet_v3_small`` state_dict key -> (row index 0..2, key inside that row) for MobileNetV3s1 / 2 / 3.  ``keys``:
    the keys to map (the classifier's are left out); default: every key of the three rows.  Nothing is downloaded."""
    return _features_key_map((MobileNetV3s1, MobileNetV3s2, MobileNetV3s3), keys)


def efficientnet_b0_key_map(keys=None) -> dict:
    """torchvision ``efficientnet_b0`` state_dict key -> (row index 0..2, key inside that row) for efficientnet_b01 / 2 / 3"""
    return _features_key_map((efficientnet_b01, efficientnet_b02, efficientnet_b03), keys)


__all__ += ["SqueezeExcitation", "Conv2dNormActivation", "InvertedResidual", "MBConv", "MobileNetV3s1", "MobileNetV3s2", "MobileNetV3s3",
            "efficientnet_b01", "efficientnet_b02", "efficientnet_b03", "mobilenet_v3_small_key_map", "efficientnet_b0_key_map"]
