"""The MI355X-native runtime under the nn.Module facade: a static reverse-mode *tape* over NHWC device buffers.

One forward pass of a model (or of a single block used on its own) records a list of backward closures; every
primitive launches hand-written HIP kernels through the C ABI (include/ydl.h) on torch's current stream.  torch is
plumbing only (allocator, streams, the autograd edge at the region boundary): there is no ATen compute inside a
taped region.  Gradient fan-in is resolved by accumulate flags on the kernels (first writer overwrites, later
writers add), concatenation is free (producers write channel slices of one buffer), and branches that never
receive a gradient are skipped, which reproduces autograd's "grad is None" for the reference's dead head layers
(SURVEY T4).
"""
from __future__ import annotations

import ctypes
import os
from typing import Callable, List, Optional, Sequence

import torch

from . import _lib as L
from . import config as _cfg

_DT = {"f32": (L.YDL_F32, torch.float32), "bf16": (L.YDL_BF16, torch.bfloat16)}


def round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> ctypes.c_void_p:
    """hipStream_t of torch's current stream (the raw accessor is ~20x cheaper than building a Stream object, and this is
    called once per kernel launch)"""
    if _RAW_STREAM is not None:
        return ctypes.c_void_p(_RAW_STREAM(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_SIDE = {}
_NO_SLAB = os.environ.get("YDL_SLAB", "1") == "0"


def side_stream(device) -> "torch.cuda.Stream":
    """second HIP stream per device: weight-gradient kernels run here, concurrently with the input-gradient chain on
    the main stream (both only read dy; small layers do not fill 256 CUs on their own)"""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    st = _SIDE.get(key)
    if st is None:
        st = _SIDE[key] = torch.cuda.Stream(device=device)
    return st


def _p(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _at(t: torch.Tensor, c0: int) -> ctypes.c_void_p:
    """``t`` from channel ``c0`` on: a per-channel row, or the (N,C,H,W) view of an NHWC buffer (c fastest)"""
    return ctypes.c_void_p(t.data_ptr() + c0 * t.element_size())


def _blocks(t: torch.Tensor, n: int, C: int) -> List[ctypes.c_void_p]:
    """the ``n`` channel blocks of ``C`` channels each that the rows of the NHWC buffer ``t`` hold side by side (Q | K | V ...)"""
    return [_at(t, i * C) for i in range(n)]


def _out_size(n: int, k: int, s: int, p: int, d: int = 1) -> int:
    """output length of a convolution or pool along one axis: ``k`` taps of dilation ``d``, stride ``s``, padding ``p``"""
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def _bn_part(y: "Var", cf, c0: int):
    """what the BatchNorm launches of the channel group from ``c0`` on read: y and the mean, invstd, scale and shift rows there"""
    return [_at(t, c0) for t in (y.t, cf["mean"], cf["invstd"], cf["scale"], cf["shift"])]


def stream_wait(waiter: "torch.cuda.Stream", on: "torch.cuda.Stream") -> None:
    """``waiter`` waits for everything enqueued on ``on`` so far.  Every cross-stream edge of the taped step goes through here so
    that a launch-list recording (yolo_dual_amd.replay) sees it."""
    waiter.wait_stream(on)
    rec = L.recorder()
    if rec is not None:
        rec.edge(on.cuda_stream, waiter.cuda_stream)


_ZDT = {torch.float32: L.YDL_F32, torch.bfloat16: L.YDL_BF16, torch.float16: L.YDL_BF16}


def zero_(t: torch.Tensor, st=None) -> torch.Tensor:
    """t[...] = 0 through the C ABI (ydl_fill_zero / ydl_zero2d) on stream ``st`` (default: torch's current stream): dense
    tensors in any dimension order, or a channel slice of an NHWC buffer seen as (N, C, H, W).  No ATen kernel runs inside a
    taped region — a launch list replays only what went through the C ABI."""
    if t.numel() == 0:
        return t
    if t.device.type != "cuda":         # host-side arenas (the data-parallel rehearsals on CPU): no device work to record
        return t.zero_()
    st = _stream() if st is None else st
    es = t.element_size()
    dense = t.is_contiguous() or (t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous())
    if dense:
        L.call("ydl_fill_zero", _p(t), t.numel() * es, st)
        return t
    if t.dim() == 4 and t.stride(1) == 1 and t.dtype in _ZDT:
        N, C, H, W = t.shape
        ld = t.stride(3)
        if t.stride(2) == W * ld and (N == 1 or t.stride(0) == H * W * ld):
            L.call("ydl_zero2d", _ZDT[t.dtype], _p(t), ld, N * H * W, C, st)
            return t
    raise RuntimeError(f"zero_: unsupported view (shape {tuple(t.shape)}, strides {t.stride()}, {t.dtype})")


class Var:
    """A NHWC activation: ``t`` is a logical (N,C,H,W) torch view whose memory is [N][H][W][ld] with c fastest."""
    __slots__ = ("t", "N", "C", "H", "W", "ld", "g", "gset", "need", "parent", "c0", "children", "tape", "dt", "rep", "alias",
                 "cat_parts", "real", "ext_src", "nuse", "wcount", "bn_src", "bnred")

    def __init__(self, tape: "Tape", t: torch.Tensor, ld: int, need: bool, parent: Optional["Var"] = None, c0: int = 0):
        self.tape = tape
        self.dt = L.YDL_F32 if t.dtype == torch.float32 else L.YDL_BF16
        self.t = t
        self.N, self.C, self.H, self.W = t.shape
        self.ld = ld
        self.g: Optional[torch.Tensor] = None
        self.gset = False
        self.need = need
        self.parent = parent
        self.c0 = c0
        self.children: List["Var"] = []
        # lazy nearest up-sampling: the LOGICAL tensor is this (stored) one replicated rep[0] x rep[1] times.
        # Point-wise ops (1x1 conv, BN, activation, channel softmax) commute with it and run at the stored size;
        # gradients of a lazy Var are kept as the SUM over the replicas, which makes every backward formula of
        # those ops identical to the un-replicated one.
        self.rep = (1, 1)
        self.alias = False      # full-range view of ``parent`` (lazy / materialise views): shares its gradient state
        # virtual channel concat (Tape.concat): no memory behind ``t`` (a zero-stride placeholder of the right shape);
        # cat_parts = [(source Var, first channel, needs bilinear resize)].  A 1x1 convolution consumes the parts
        # directly (conv over a concat = sum of convs over the sources, and a 1x1 conv commutes with the resize);
        # every other consumer goes through Tape.materialize, which builds the real tensor once (``real``).
        self.cat_parts = None
        self.real = None
        # fused BatchNorm-backward reduce (Tape._try_bnred): on the TOP buffer, nuse = pending consumers (a hint) and wcount = the
        # write log (the validation), both as absolute channel ranges; on a conv+BN output, bn_src = what a consumer's dgrad epilogue
        # needs to run this layer's reduce pass, bnred = (sums, length of the write log right after that dgrad's write) once one has
        self.nuse = None          # top buffer: channel ranges of the recorded ops that will still write into its gradient
        self.wcount = None        # top buffer: channel ranges written so far, in order
        self.bn_src = None
        self.bnred = None
        # lazily converted region input: the caller's (N,C,H,W) f32 tensor; the NHWC copy is made by Tape.materialize on
        # first use — or never, when the first layer is a stem conv that reads a space-to-depth conversion instead
        self.ext_src = None

    def root(self) -> "Var":
        v = self
        while v.alias:
            v = v.parent
        return v

    def top(self) -> "Var":
        """the Var that owns the buffer (slices and alias views share their parent's gradient storage)"""
        v = self
        while v.parent is not None:
            v = v.parent
        return v

    def abs_range(self) -> tuple:
        """[c0, c1) of this Var in its top buffer's channels"""
        c0, v = 0, self
        while v.parent is not None:
            if not v.alias:
                c0 += v.c0
            v = v.parent
        return (c0, c0 + self.C)

    @property
    def npix(self) -> int:
        return self.N * self.H * self.W

    @property
    def LH(self) -> int:
        return self.H * self.rep[0]

    @property
    def LW(self) -> int:
        return self.W * self.rep[1]

    @property
    def lazy(self) -> bool:
        return self.rep != (1, 1)

    @property
    def virtual(self) -> bool:
        return self.cat_parts is not None or self.ext_src is not None

    def is_set(self) -> bool:
        v = self.root()
        return v.gset or (v.parent is not None and v.parent.is_set())

    def aligned(self) -> bool:
        """16-byte channel alignment of a slice (whole buffers always are): required by the vector kernels"""
        return self.parent is None or self.alias and self.parent.aligned() or (self.c0 % 8 == 0 and self.C % 8 == 0 and self.parent.aligned())

    def slice(self, c0: int, c1: int) -> "Var":
        assert not self.virtual, "materialize a virtual Var before slicing it"
        v = Var(self.tape, self.t[:, c0:c1], self.ld, self.need, parent=self, c0=c0)
        self.children.append(v)
        return v


def _alloc(N: int, C: int, H: int, W: int, tdtype: torch.dtype, device, zero: bool = False) -> (torch.Tensor, int):
    ld = round_up(C, 8)
    buf = torch.empty((N, H, W, ld), dtype=tdtype, device=device)
    if zero or ld != C:
        zero_(buf)
    return buf.permute(0, 3, 1, 2)[:, :C], ld


class LazyOutput:
    """side channel between a region whose output is a nearest-replicated tensor and SegmentationLoss:
    ``low`` = the (N, C, H, W) tensor the (N, C, H*rh, W*rw) output replicates, ``version`` = the output's version
    counter when it was produced (an in-place edit by the caller invalidates the shortcut), ``dlow`` = replica-summed
    gradient handed back by the loss backward, ``dummy`` = the zero-stride placeholder gradient it returned.

    Fused tail (config.use_fused_seg_tail): the region hands over the stored LOGITS ``x`` instead (a Var: NHWC rows in the compute
    dtype); ``low`` is then computed from them only when something reads it (a second loss on the prediction, the fold into a
    dense gradient).  The loss evaluates ydl_seg_tail_fwd on ``x`` and its backward leaves ``tail`` = [labels, class weights,
    label smoothing, workspace, label counts, loss gradient] for the region, which issues ydl_seg_tail_bwd straight into the
    gradient of ``x`` (or, where the prediction had other consumers, recovers ``dlow`` from it)."""
    __slots__ = ("_low", "x", "rep", "version", "dlow", "dummy", "claimed", "tail")

    def __init__(self, low: Optional[torch.Tensor], rep, x=None):
        self._low, self.x, self.rep, self.version, self.dlow, self.dummy, self.claimed = low, x, tuple(rep), -1, None, None, False
        self.tail = None

    @property
    def low(self) -> torch.Tensor:
        if self._low is None:
            x = self.x
            self._low = torch.empty((x.N, x.C, x.H, x.W), dtype=torch.float32, device=x.t.device)
            sn, sc, sh, sw = self._low.stride()
            L.call("ydl_softmax_fwd", x.dt, _p(x.t), x.ld, _p(self._low), sn, sc, sh, sw, x.N, x.H, x.W, x.C, 1, 1, _stream())
        return self._low

    def tail_dlow(self) -> torch.Tensor:
        """the replica-summed loss gradient of the fused tail as a tensor (``tail`` is consumed)"""
        target, cw, kind, ls, eps, ws, _counts, g = self.tail
        self.tail = None
        low = self.low
        dlow = torch.empty_like(low)
        sn, sc, sh, sw = low.stride()
        N, C, h, w = low.shape
        L.call("ydl_seg_loss_rep_bwd", _p(low), sn, sc, sh, sw, _p(target), _p(cw), kind, ls, eps, N, C, h, w, self.rep[0], self.rep[1],
               _p(ws), _p(g), _p(dlow), _stream())
        return dlow


class Tape:
    def __init__(self, dtype: str, device, train: bool, record: bool):
        self.dname = dtype
        self.dt, self.tdt = _DT[dtype]
        self.V = 4 if dtype == "f32" else 8
        self.device = device
        self.train = train
        self.record = record
        self.bw: List[Callable[[], None]] = []
        self.touched_params: List[torch.nn.Parameter] = []
        self._side_used = False
        self._keep: List[Var] = []
        self._pending_wgrad: List[Callable] = []   # weight-gradient launches waiting for the next fork of the side stream
        self._bw_left = 0
        self.ext = None      # (Var, tensor) of a region whose external output was written directly (softmax head)
        self.labels_out = False   # the caller wants the label map of the output only (yolo_dual_amd.predict): see export_labels
        self._slab = None    # zero-initialised f32 scratch of the region: accumulator rows the kernels add into (BN replica sums)
        self._slab_off = 0
        self._slab_total = 0         # floats handed out so far (the owner module remembers it as next step's slab size)
        self._slab_hint = 0
        self._main = torch.cuda.current_stream() if torch.device(device).type == "cuda" else None

    # ------------------------------------------------------------------ buffers
    def new(self, N: int, C: int, H: int, W: int, need: bool = True, zero: bool = False, f32: bool = False) -> Var:
        t, ld = _alloc(N, C, H, W, torch.float32 if f32 else self.tdt, self.device, zero)
        return Var(self, t, ld, need)

    def zeroed(self, nfloats: int) -> torch.Tensor:
        """``nfloats`` f32 zeros (16-byte aligned) from the region's slab: ONE memset per slab instead of one per accumulator row.
        A slab is cleared when it is created, before any kernel that adds into it is enqueued; rows are handed out once."""
        n = round_up(nfloats, 4)
        if _NO_SLAB:                      # debugging switch: every row its own buffer and memset
            return zero_(torch.empty(nfloats, dtype=torch.float32, device=self.device))
        self._slab_total += n
        if self._slab is None or self._slab_off + n > self._slab.numel():
            cap = max(1 << 18, self._slab_hint, 2 * n, 2 * (self._slab.numel() if self._slab is not None else 0))
            self._slab = zero_(torch.empty(cap, dtype=torch.float32, device=self.device))
            self._slab_off = 0
            # the memset went to the CURRENT stream; rows of this slab may be used on the region's other stream too (dead head
            # branch, deferred work): order it behind the memset.  Normally the slab is sized from the previous step's need and
            # created once, by the first layer, before any fork.
            # (Only when this region has forked the side stream already: waiting on a stream that is not part of the step
            #  would pull it into a HIP-graph capture and leave it unjoined.)
            cur = torch.cuda.current_stream()
            side = _SIDE.get(torch.cuda.current_device())
            if side is not None and (self._side_used or getattr(self, "_side_fwd", False)):
                for other in (self._main, side):
                    if other is not None and other.cuda_stream != cur.cuda_stream:
                        stream_wait(other, cur)
        out = self._slab[self._slab_off:self._slab_off + nfloats]
        self._slab_off += n
        return out

    def new_like(self, v: Var) -> Var:
        return self.new(v.N, v.C, v.H, v.W, v.need, f32=(v.dt == L.YDL_F32))

    def _flat(self, x: Var) -> Var:
        """``x`` as a real tensor with 16-byte aligned rows: materialised, and an odd channel slice staged through a buffer of its own"""
        x = self.materialize(x)
        if not x.aligned():
            x = self.copy(x, self.new_like(x))
        return x

    def _out(self, who: str, shape, out: Optional[Var], need: bool = True, f32: bool = False, aligned: bool = False) -> Var:
        """where the op ``who`` writes its (N, C, H, W) = ``shape`` result: a fresh buffer (``need``, ``f32`` as in ``new``), or the
        caller's ``out`` (typically a concat slice) once its shape has been checked, and its 16-byte alignment where the kernels
        need it (``aligned``)"""
        if out is None:
            return self.new(*shape, need=need, f32=f32)
        if (out.N, out.C, out.H, out.W) != tuple(shape) or (aligned and not out.aligned()):
            raise RuntimeError(f"{who}: the output slice has the wrong shape" + (" or is not 16-byte aligned" if aligned else ""))
        return out

    def _ws(self, nbytes: int, keep: bool = False) -> torch.Tensor:
        """an uninitialised f32 workspace of ``nbytes`` bytes.  The lifetime rule of every scratch buffer of the tape: one used only
        by launches on the stream it was allocated under needs no ``keep``, because the caching allocator orders the reuse of its
        memory on that stream.  Anything a launch on the side stream reads or writes (deferred weight gradients, the dead head
        branch) goes into ``_keep``, which ``run_backward`` clears only after it has joined the streams."""
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        if keep:
            self._keep.append(ws)
        return ws

    def _gbuf(self, v: Var) -> torch.Tensor:
        """gradient buffer of v (a slice shares its parent's buffer)"""
        v = v.root()
        if v.g is None:
            if v.parent is not None:
                pg = self._gbuf(v.parent)
                v.g = pg[:, v.c0:v.c0 + v.C]
            else:
                v.g, _ = _alloc(v.N, v.C, v.H, v.W, v.t.dtype, self.device)
        return v.g

    def _alias_grad(self, v: Var, o: Var, dout: torch.Tensor) -> bool:
        """A residual joined after the activation has d/dv = dout: when v's gradient has no buffer and no writer yet, and both are
        whole buffers of the same layout, v adopts dout's storage (later writers accumulate into it; dout's consumer, the BN
        backward that calls this, reads it before anything else is enqueued).  Saves one write pass over the tensor."""
        v, o = v.root(), o.root()
        if (v.g is not None or v.is_set() or v.parent is not None or o.parent is not None or v.children or o.children
                or v.lazy or o.lazy or v.ld != o.ld or (v.N, v.C, v.H, v.W) != (o.N, o.C, o.H, o.W) or v.t.dtype != o.t.dtype
                or dout.shape != o.t.shape):
            return False
        v.g = dout
        v.gset = True
        self._note_write(v)
        return True

    def _try_bnred(self, x: Var, gp, dy: Var, wt: torch.Tensor, gx: torch.Tensor, acc: int, st) -> bool:
        """the input gradient of a convolution with the BatchNorm-backward REDUCE pass of the layer(s) that produced ``x`` in its
        epilogue (ydl_conv_dgrad_bnred) — when this is, as far as the forward pass could tell, the last write of that gradient
        (no pending consumer on the buffer), the producers are plain conv+BN(+SiLU) outputs covering 8-aligned channel ranges, and
        the geometry runs on a kernel that has the fused epilogue.  The producers find (sums, write count) on their output Var and
        skip their own reduce launch if nothing wrote the buffer in between (Tape.conv_bn_act.bw); a wrong guess only wastes the
        epilogue work."""
        if not _cfg.bn_bwd_fuse() or self.dt != L.YDL_BF16:
            return False
        xr = x.root()
        tp = xr.top()
        pend = tp.nuse or ()

        def last_writer(v: Var) -> bool:
            a, b = v.abs_range()
            return not any(r[0] < b and a < r[1] for r in pend)
        segs = []
        if xr.bn_src is not None:
            if last_writer(xr):
                segs.append((0, xr))
        else:
            for c in xr.children:
                if c.bn_src is not None and not c.alias and last_writer(c):
                    segs.append((c.c0, c))
        if not segs or len(segs) > 2:
            return False
        segs.sort(key=lambda e: e[0])
        if len(segs) == 2 and segs[0][0] + segs[0][1].C > segs[1][0]:
            return False
        if not L.lib().ydl_conv_dgrad_bnred_supported(gp, self.dt):
            return False
        red = L.BnRed()
        red.nseg = len(segs)
        keep = []
        for i, (c0, v) in enumerate(segs):
            yptr, ldy, cf, co, cw, act, ykeep = v.bn_src
            cp = round_up(cw, 8)
            sums = self.zeroed(L.BN_REPLICAS * 2 * cp)
            red.c0[i], red.c1[i], red.ldy[i], red.cp[i], red.act[i] = c0, c0 + cw, ldy, cp, act
            red.y[i] = yptr
            red.scale[i], red.shift[i] = cf["scale"][co:].data_ptr(), cf["shift"][co:].data_ptr()
            red.mean[i], red.invstd[i] = cf["mean"][co:].data_ptr(), cf["invstd"][co:].data_ptr()
            red.sums[i] = sums.data_ptr()
            keep.append((v, sums))
        L.call("ydl_conv_dgrad_bnred", gp, self.dt, _p(dy.t), _p(wt), _p(gx), acc, ctypes.byref(red), st)
        wc = len(tp.wcount)
        for v, sums in keep:
            v.bnred = (sums, wc)
        self._keep.append(red)
        return True

    def _use(self, v: Optional[Var]) -> None:
        """forward-time note: a recorded op will later write d/dv (hint for Tape._try_bnred; a missing note only costs a fallback)"""
        if v is not None and self.record:
            v = v.root()
            tp = v.top()
            if tp.nuse is None:
                tp.nuse = []
            tp.nuse.append(v.abs_range())

    def _unwritten_since(self, o: Var, n: int) -> bool:
        """no gradient write has touched o's channels since the write log of its buffer had n entries"""
        o = o.root()
        a, b = o.abs_range()
        log = o.top().wcount or ()
        return not any(r[0] < b and a < r[1] for r in log[n:])

    def _note_write(self, v: Var) -> None:
        tp = v.top()
        r = v.abs_range()
        if tp.wcount is None:
            tp.wcount = []
        tp.wcount.append(r)
        if tp.nuse:
            try:
                tp.nuse.remove(r)
            except ValueError:
                pass

    def grad_target(self, v: Var) -> (torch.Tensor, int):
        """(buffer, accumulate) for a kernel about to write d/dv; marks v as set."""
        v = v.root()
        self._note_write(v)
        g = self._gbuf(v)
        acc = 1 if v.is_set() else 0
        if not acc and v.children and any(c.gset for c in v.children):
            # a slice already holds a gradient but the whole buffer does not: zero the rest, then accumulate
            for c in v.children:
                if not c.gset:
                    zero_(self._gbuf(c))
            covered = sorted((c.c0, c.c0 + c.C) for c in v.children)
            pos = 0
            for a, b in covered:
                if a > pos:
                    zero_(g[:, pos:a])
                pos = max(pos, b)
            if pos < v.C:
                zero_(g[:, pos:])
            acc = 1
        v.gset = True
        return g, acc

    def _record(self, out: Var, bw: Callable[[], None], uses: Sequence[Optional[Var]] = ()) -> Var:
        """the tail of a taped op, returning ``out``: when the tape records, note the inputs in ``uses`` whose gradient the backward
        will write (``_use``; None and inputs nobody differentiates are skipped) and queue ``bw``, which runs only if ``out`` has
        received a gradient (a dead branch leaves its parameters' grad None)"""
        if self.record:
            for v in uses:
                if v is not None and v.need:
                    self._use(v)

            def run():
                if out.is_set():
                    bw()
            self.bw.append(run)
        return out

    def _grad_via(self, v: Var, launch: Callable[[Var], None], st, aside: Optional[Var] = None) -> None:
        """d/dv from ``launch(dst)``, a pass that can only OVERWRITE its destination: straight into v's gradient when this is its
        first write; otherwise into a buffer of its own (``aside``, or a fresh one), which ydl_copy2d then adds in.  When nobody
        wants d/dv the pass still runs (it forms parameter sums too) and its output is dropped."""
        g, acc = self.grad_target(v) if v.need else (None, 1)
        if not acc:
            launch(Var(self, g, v.ld, False))
            return
        tmp = self.new_like(v) if aside is None else aside
        launch(tmp)
        if v.need:
            L.call("ydl_copy2d", v.dt, _p(tmp.t), tmp.ld, _p(g), v.ld, v.npix, v.C, 1, st)

    def _grad_or_scratch(self, v: Var):
        """(buffer, ld, accumulate) for a launch that always writes d/dv: v's gradient, or a scratch tensor when nobody wants it"""
        if v.need:
            g, acc = self.grad_target(v)
            return g, v.ld, acc
        s = self.new(v.N, v.C, v.H, v.W)
        return s.t, s.ld, 0

    # ------------------------------------------------------------------ per-channel parameters: gradient rows and reporting
    @staticmethod
    def _param_grad(p: torch.nn.Parameter, device) -> torch.Tensor:
        """gradient row of a per-channel parameter; a frozen one gets a scratch row (the launch writes all its rows)"""
        if not p.requires_grad:
            return torch.empty(p.numel(), dtype=torch.float32, device=device)
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        return p.grad

    def _touch(self, *params) -> None:
        """report parameters whose gradient launches are enqueued (the data-parallel hook may now reduce their bucket)"""
        for p in params:
            if p is not None and p.requires_grad:
                _cfg.mark_touched(p)

    # ------------------------------------------------------------------ region boundary
    def input_nchw(self, x: torch.Tensor, lazy: bool = False) -> Var:
        """external (N,C,H,W) f32 tensor (any strides) -> internal NHWC compute dtype, channels zero padded.
        ``lazy``: return a virtual Var and convert on first use (see Var.ext_src)"""
        x = x.detach()
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.contiguous().float()
        N, C, H, W = x.shape
        if lazy:
            ph = torch.empty(1, dtype=self.tdt, device=self.device)
            v = Var(self, ph.expand(N, C, H, W), round_up(C, 8), False)
            v.ext_src = x
            return v
        v = self.new(N, C, H, W, need=False, zero=True)
        L.call("ydl_nchw_to_nhwc", self.dt, _p(x), _p(v.t), v.ld, N, C, H, W, _stream())
        return v

    def input_s2d(self, src: torch.Tensor, s: int) -> Var:
        """space-to-depth conversion of an external (N,C,H,W) tensor: (N, s*s*C, H/s, W/s) NHWC Var (ydl_nchw_to_s2d)"""
        N, C, H, W = src.shape
        v = self.new(N, C * s * s, H // s, W // s, need=False)
        L.call("ydl_nchw_to_s2d", self.dt, _p(src), _p(v.t), v.ld, N, C, H, W, s, _stream())
        return v

    # ------------------------------------------------------------------ lazy nearest up-sampling
    def upsample_lazy(self, x: Var, fh: int, fw: int) -> Var:
        """nearest up-sampling by integer factors without touching memory (see Var.rep)"""
        if x.virtual:
            x = self.materialize(x)
        v = Var(self, x.t, x.ld, x.need, parent=x, c0=0)
        v.alias = True
        v.rep = (x.rep[0] * fh, x.rep[1] * fw)
        return v

    def materialize(self, x: Var, out: Optional[Var] = None) -> Var:
        """turn a lazy Var into a real (LH, LW) tensor (nearest replication kernel; backward sums the replicas);
        a virtual concat becomes the real concatenated tensor"""
        if x.virtual:
            if x.real is None:
                if x.ext_src is not None:
                    x.real = self.input_nchw(x.ext_src)
                else:
                    x.real = self._concat_real([v for (v, _c0, _rs) in x.cat_parts], True)
            x = x.real
        if not x.lazy:
            return x if out is None else self.copy(x, out)
        fh, fw = x.rep
        plain = Var(self, x.t, x.ld, x.need, parent=x, c0=0)
        plain.alias = True
        return self.resize(plain, x.H * fh, x.W * fw, L.RESIZE_NEAREST, 1.0 / fh, 1.0 / fw, out=out)

    def export_nchw(self, v: Var) -> torch.Tensor:
        v = self.materialize(v)
        out = torch.empty((v.N, v.C, v.H, v.W), dtype=torch.float32, device=self.device)
        L.call("ydl_nhwc_to_nchw", v.dt, _p(v.t), v.ld, _p(out), v.N, v.C, v.H, v.W, 0, _stream())
        return out

    def export_labels(self, v: Var) -> torch.Tensor:
        """argmax over the channels of ``v`` as a uint8 (N, LH, LW) label map (ydl_argmax_labels).  The scores are read where they
        are stored, NHWC in the compute dtype and at the resolution before a lazy nearest up-sampling; the replication is folded
        into the store, so neither ydl_nhwc_to_nchw nor the replication kernel runs."""
        if v.virtual:
            v = self.materialize(v)
        out = torch.empty((v.N, v.LH, v.LW), dtype=torch.uint8, device=self.device)
        sn, sc, sh, sw = v.t.stride()
        L.call("ydl_argmax_labels", v.dt, _p(v.t), sn, sc, sh, sw, v.N, v.C, v.H, v.W, v.rep[0], v.rep[1], _p(out), v.LH * v.LW, v.LW,
               _stream())
        return out

    def export_labels_softmax_resized(self, v: Var, Ho: int, Wo: int) -> torch.Tensor:
        """argmax of ``resize(softmax(v), Ho, Wo, bilinear)`` as a uint8 (N, Ho, Wo) label map, in one launch that writes neither
        the probabilities nor their resized copy (ydl_softmax_resize_labels): the labels of softmax + Tape.resize + export_nchw"""
        v = self.materialize(v)           # (a channel slice is fine: the kernel reads a row element by element from its first channel)
        out = torch.empty((v.N, Ho, Wo), dtype=torch.uint8, device=self.device)
        L.call("ydl_softmax_resize_labels", v.dt, _p(v.t), v.ld, v.N, v.C, v.H, v.W, Ho, Wo, _p(out), Ho * Wo, Wo, _stream())
        return out

    def seed_grad_nchw(self, v: Var, g: torch.Tensor) -> None:
        g = g.detach()
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.contiguous().float()
        buf, acc = self.grad_target(v)
        assert acc == 0
        L.call("ydl_nchw_to_nhwc", v.dt, _p(g), _p(buf), v.ld, v.N, v.C, v.H, v.W, _stream())

    def grad_nchw(self, v: Var) -> Optional[torch.Tensor]:
        if not v.is_set():
            return None
        out = torch.empty((v.N, v.C, v.H, v.W), dtype=torch.float32, device=self.device)
        L.call("ydl_nhwc_to_nchw", v.dt, _p(self._gbuf(v)), v.ld, _p(out), v.N, v.C, v.H, v.W, 0, _stream())
        return out

    def _defer_wgrad(self, launch: Callable, keep=()) -> None:
        """queue a weight-gradient launch for the side stream.  One fork (event record + stream wait) per ``wgrad_batch`` launches
        instead of one per layer: forks cost host time in eager mode and a cross-branch edge each in a captured graph.  The last
        layers of the sweep fork at once, so the tail of the backward pass does not wait for a batch to fill."""
        self._pending_wgrad.append(launch)
        self._keep.extend(keep)
        if len(self._pending_wgrad) >= _cfg.wgrad_batch() or self._bw_left <= 2:
            self._flush_wgrads()

    def _flush_wgrads(self) -> None:
        if not self._pending_wgrad:
            return
        side = side_stream(self.device)
        stream_wait(side, torch.cuda.current_stream())
        with torch.cuda.stream(side):
            st = _stream()
            for launch in self._pending_wgrad:
                launch(st)
        self._pending_wgrad.clear()
        self._side_used = True

    def run_backward(self) -> None:
        n = len(self.bw)
        for i, fn in enumerate(reversed(self.bw)):
            self._bw_left = n - 1 - i
            fn()
        self.bw.clear()
        self._flush_wgrads()
        if self._side_used:
            stream_wait(torch.cuda.current_stream(), side_stream(self.device))   # parameter grads complete
            self._side_used = False
        self._keep.clear()

    # ------------------------------------------------------------------ BatchNorm pieces shared by conv_bn_act, _side_bn_act and the bias-only convolutions
    def _bn_coeffs(self, m, cf, C: int, st, part=None) -> None:
        """scale / shift (and in train mode mean / invstd, the running statistics) of ``m.bn`` into ``cf``: from the partial rows
        ``part`` = (ws, rows, block_m, npix, rep) a convolution launch wrote (ydl_bn_finalize), or in eval mode (``part`` None)
        from the running statistics (ydl_bn_eval_coeffs)"""
        bn = m.bn
        if part is None:
            L.call("ydl_bn_eval_coeffs", C, _p(bn.weight), _p(bn.bias), _p(bn.running_mean), _p(bn.running_var), bn.eps,
                   _p(cf["scale"]), _p(cf["shift"]), st)
            return
        ws, rows, block_m, npix, rep = part
        L.call("ydl_bn_finalize", _p(ws), rows, block_m, npix, C, _p(bn.weight), _p(bn.bias), bn.eps, bn.momentum,
               _p(bn.running_mean), _p(bn.running_var), _p(cf["mean"]), _p(cf["invstd"]), _p(cf["scale"]), _p(cf["shift"]), rep, st)

    def _bn_grad_rows(self, m, cp: int):
        """(dgamma row, dbeta row, accumulate flag) of ``m.bn``.  A frozen parameter (requires_grad False) gets a scratch row: the
        sums still exist (dy needs them).  One accumulate flag serves both rows, so a scratch row beside a real one is zeroed."""
        _w, train_g, train_b = m.trainable()
        gw, accw = m.grad_slot(self, "gamma") if train_g else (torch.empty(cp, dtype=torch.float32, device=self.device), 0)
        gb, accb = m.grad_slot(self, "beta") if train_b else (torch.empty(cp, dtype=torch.float32, device=self.device), 0)
        if accb != accw:
            zero_(gw if not train_g else gb)
            accw = 1
        return gw, gb, accw

    def _res_grad(self, res: Optional[Var], res_mode: int, o: Var, dout: torch.Tensor):
        """(buffer, row stride, residual mode) for the BatchNorm-backward pass that also writes (or adds) the gradient of the
        residual operand: dz for a residual joined before the activation, dout itself for one joined after it.  (None, 0, mode)
        when there is nothing to write: no residual, none wanted, or d/dres IS dout and res took dout's buffer (no copy pass)."""
        if res is None or not res.need or res_mode not in (L.RES_BEFORE_ACT, L.RES_AFTER_ACT):
            return None, 0, res_mode
        if res_mode == L.RES_AFTER_ACT and self._alias_grad(res, o, dout):
            return None, 0, res_mode
        gbuf, racc = self.grad_target(res)
        return gbuf, res.ld, (res_mode | L.RES_GRAD_ACCUMULATE) if racc else res_mode

    def _bn_apply(self, y: Var, scale: torch.Tensor, shift: torch.Tensor, act: int, out: Var, npix: int, cp: int, st,
                  res: Optional[Var] = None, res_mode: int = L.RES_NONE, c0: int = 0) -> None:
        """the apply pass: out = act(y * scale + shift) [+ res] over ``cp`` channels (ydl_bn_act_fwd).  ``c0``: the channel group of
        ``y`` and of the coefficient rows that starts there (split outputs).  A bias is the scale-1 case, in place (out is y)."""
        L.call_act("ydl_bn_act_fwd", self.dt, _at(y.t, c0), y.ld, _at(scale, c0), _at(shift, c0), _p(res.t) if res is not None else None,
                   res.ld if res is not None else 0, res_mode, act, _p(out.t), out.ld, npix, cp, st)

    def _bn_bwd_rows(self, m, y: Var, cf, act: int, o: Var, res: Optional[Var], res_mode: int, dy: Var, rows, npix: int, cw: int,
                     cp: int, st, c0: int = 0, touch: bool = True) -> None:
        """the partial-row BatchNorm backward (ydl_bn_act_bwd) of the ``cw`` channels from ``c0`` on whose activated output is ``o``:
        fills that channel group of ``dy``, writes (or adds) the residual's gradient and dgamma / dbeta into ``rows`` =
        _bn_grad_rows(m, .), then reports the BatchNorm parameters (``touch``: a caller with more groups to go does that itself)"""
        gw, gb, accw = rows
        dout = self._gbuf(o)
        dres_t, dres_ld, rmode = self._res_grad(res, res_mode, o, dout)
        ws = self._ws(L.lib().ydl_bn_bwd_ws_bytes(npix, cp))
        L.call_act("ydl_bn_act_bwd", self.dt, _at(y.t, c0), y.ld, _p(dout), o.ld, _p(o.t), o.ld, _at(m.bn.weight, c0),
                   _at(cf["mean"], c0), _at(cf["invstd"], c0), _at(cf["scale"], c0), _at(cf["shift"], c0), rmode, act,
                   _at(dy.t, c0), dy.ld, _p(dres_t), dres_ld, _at(gw, c0), _at(gb, c0), accw, _p(ws), npix, cw, cp, st)
        if touch:
            m.touch_bn()          # dgamma / dbeta kernels are enqueued: the DP hook may now reduce their bucket

    # ------------------------------------------------------------------ conv + BN + act (+ residual)
    def conv_bn_act(self, x: Var, m, s: int, p: int, act: int, out=None,
                    res: Optional[Var] = None, res_mode: int = L.RES_NONE) -> Var:
        """out = act(bn(conv(x))) [+ res].  ``m`` is a yolo_dual_amd.modules.Conv (parameter holder) or a fused sibling
        pair.  ``out`` may be a Var (typically a concat slice) or a LIST of Vars that split the output channels (fused
        siblings: each part is activated into its own destination).
        Reference: Conv.forward seg_diceloss_yolov5.py:403-409."""
        k = m.k
        Cout, Cin = m.c2, m.c1
        if x.C != Cin:
            raise RuntimeError(f"Conv layer input channel mismatch: got {x.C}, weight expects {Cin}")
        outs = list(out) if isinstance(out, (list, tuple)) else None
        rep = 1
        virt = None
        if x.virtual and x.cat_parts is None:
            x = self.materialize(x)
        if x.virtual:
            # conv1x1(cat(a.., bilinear_up(b))) = sum_a conv1x1_a(a) + bilinear_up(conv1x1_b(b)): worth it when the
            # up-sampled source is much wider than the output (the 512-channel 1/16-scale map of the yolov5 head)
            rs = [v for (v, _c0, r_) in x.cat_parts if r_]
            if (k == 1 and s == 1 and p == 0 and res is None and m.splittable() and Cin % 8 == 0
                    and rs[0].C >= 2 * Cout and (outs is None or all(o.aligned() for o in outs))
                    and (outs is not None or out is None or out.aligned())):
                virt = [(self.materialize(v) if (v.lazy or not v.aligned()) else v, c0_, r_) for (v, c0_, r_) in x.cat_parts]
                virt = [(v if v.aligned() else self.copy(v, self.new(v.N, v.C, v.H, v.W, need=v.need)), c0_, r_)
                        for (v, c0_, r_) in virt]
            else:
                x = self.materialize(x)
        if x.lazy:
            if k == 1 and s == 1 and p == 0 and res is None and out is None:
                rep = x.rep[0] * x.rep[1]           # point-wise: run at the stored size, stay lazy
            else:
                x = self.materialize(x)
        if res is not None and (res.lazy or res.virtual):
            res = self.materialize(res)
        if not x.aligned():                       # odd channel split: stage through an aligned buffer (cold path)
            x = self.copy(x, self.new(x.N, x.C, x.H, x.W, need=x.need))
        if res is not None and not res.aligned():
            res = self.copy(res, self.new(res.N, res.C, res.H, res.W, need=res.need))
        if outs is None and out is not None and not out.aligned():
            tmp = self.conv_bn_act(x, m, s, p, act, None, res, res_mode)
            return self.copy(tmp, out)
        Ho, Wo = _out_size(x.H, k, s, p), _out_size(x.W, k, s, p)
        y = self.new(x.N, Cout, Ho, Wo)
        if outs is None:
            fresh = out is None
            out = self._out("conv_bn_act", (x.N, Cout, Ho, Wo), out)
            if fresh:
                out.rep = x.rep
                if virt is None and not x.need and not any(m.trainable()) and (res is None or not res.need):
                    out.need = False      # frozen layer on a prefix that needs no gradient: consumers skip their dgrad into it
            outs = [out]
        else:
            if sum(o.C for o in outs) != Cout or any(o.C % 8 or not o.aligned() for o in outs) or res is not None:
                raise RuntimeError("conv_bn_act: split outputs must be aligned channel groups summing to Cout")
        parts = []                                 # (channel offset, width, destination Var)
        c0 = 0
        for o in outs:
            parts.append((c0, o.C, o))
            c0 += o.C
        st = _stream()
        w, wt = m.compute_weights(self)
        npix = x.N * Ho * Wo
        cf = m.coeffs(self.device)                   # dict of f32 [Cp] tensors: mean, invstd, scale, shift
        Cin_p, Cout_p = round_up(Cin, 8), round_up(Cout, 8)
        if virt is None:
            gkey = (x.N, x.H, x.W, Cin, Cout, k, s, p, x.ld, y.ld, self.dt, L.debug_epoch())
            gc = getattr(m, "_geom_cache", None)
            if gc is None or gc[0] != gkey:
                geom = L.ConvGeom(x.N, x.H, x.W, Cin, Ho, Wo, Cout, k, s, p, x.ld, y.ld, 0)
                gpp = ctypes.byref(geom)
                gc = (gkey, geom, L.lib().ydl_conv_fwd_stats_ws_bytes(gpp, self.dt), L.lib().ydl_conv_fwd_grid_m(gpp, self.dt),
                      L.lib().ydl_conv_fwd_block_m(gpp, self.dt))
                try:
                    m._geom_cache = gc
                except Exception:
                    pass
            geom = gc[1]
            subs = None
        else:
            # one sub-convolution per source, on column block [c0, c0+C) of the weight matrix (row stride = Cin_p)
            subs = []
            for (v, c0_, r_) in virt:
                gv = L.ConvGeom(v.N, v.H, v.W, v.C, v.H, v.W, Cout, 1, 1, 0, v.ld, y.ld, Cin_p)
                subs.append((v, c0_, r_, gv))
            subs.sort(key=lambda e: not e[2])        # the resized source first: it initialises y
            geom = subs[-1][3]                       # the launch that writes the BN partials
        gp = ctypes.byref(geom)

        sums_mode = self.train and _cfg.bn_sums(self.dname)      # replica sums instead of partial rows + finalize / merge launches
        sums = ws = None
        if sums_mode:
            sums = self.zeroed(L.BN_REPLICAS * 2 * Cout_p)
        elif self.train:
            if subs is None:
                nbytes, grid_m, block_m = gc[2], gc[3], gc[4]
            else:
                nbytes = L.lib().ydl_conv_fwd_stats_ws_bytes(gp, self.dt)
                grid_m, block_m = L.lib().ydl_conv_fwd_grid_m(gp, self.dt), L.lib().ydl_conv_fwd_block_m(gp, self.dt)
            ws = self._ws(nbytes)
        ws_ptr = _p(sums if sums_mode else ws) if self.train else None
        fwd_entry = "ydl_conv_fwd_sums" if sums_mode else "ydl_conv_fwd"
        if subs is None:
            L.call(fwd_entry, gp, self.dt, _p(x.t), _p(w), _p(y.t), ws_ptr, 0, st)
        else:
            self._fwd_split(subs, w, y, Cin_p, ws_ptr, fwd_entry, sums_mode, st)
        if not sums_mode:
            self._bn_coeffs(m, cf, Cout, st, (ws, grid_m, block_m, npix, rep) if self.train else None)
        single = len(parts) == 1
        for (co, cw, o) in parts:
            cp = round_up(cw, 8)
            if sums is None:
                self._bn_apply(y, cf["scale"], cf["shift"], act, o, npix, cp, st, res, res_mode, c0=co)
                continue
            # statistics, coefficients (kept for the backward) and running statistics of this channel group in the apply launch
            yp, mean, invstd, scale, shift = _bn_part(y, cf, co)
            bn = m.bn
            L.call_act("ydl_bn_act_fwd_sums", self.dt, yp, y.ld, _at(sums, co), Cout_p, npix, _at(bn.weight, co), _at(bn.bias, co), bn.eps,
                       bn.momentum, _at(bn.running_mean, co), _at(bn.running_var, co), mean, invstd, scale, shift, rep,
                       _p(res.t) if res is not None else None, res.ld if res is not None else 0, res_mode, act,
                       _p(o.t), o.ld, npix, cw, cp, st)
        ret = outs[0] if single else None
        if not self.record:
            return ret
        if not self.train:
            raise RuntimeError("backward through eval-mode BatchNorm is not supported")

        train_w, train_g, train_b = m.trainable()
        if subs is None and x.need:
            self._use(x)
        if res is not None and res.need and res_mode in (L.RES_BEFORE_ACT, L.RES_AFTER_ACT):
            self._use(res)
        if (sums_mode and _cfg.bn_bwd_fuse() and self.dt == L.YDL_BF16 and rep == 1 and act in (L.ACT_NONE, L.ACT_SILU)
                and res_mode in (L.RES_NONE, L.RES_AFTER_ACT)):
            # what the dgrad of this output's LAST consumer needs to run this layer's reduce pass in its epilogue
            es2 = y.t.element_size()
            for (co, cw, o) in parts:
                if cw % 8 == 0 and o.aligned():
                    o.bn_src = (y.t.data_ptr() + co * es2, y.ld, cf, co, cw, act, y)

        def bw():
            if not any(o.is_set() for (_c, _w, o) in parts):
                return                                   # dead branch: parameters keep grad None
            if not (x.need or train_w or train_g or train_b) and subs is None and (res is None or not res.need):
                return                                   # frozen layer on a frozen prefix: nothing upstream wants a gradient
                                                         # (a residual operand that does is served by the BN-backward pass below)
            st2 = _stream()
            if (sums_mode and subs is None and self.dt == L.YDL_BF16 and rep == 1 and act in (L.ACT_NONE, L.ACT_SILU)
                    and train_w and x.need and _cfg.fuse_bn_pw_backward() and _cfg.fuse_pw_backward() and not _cfg.bn_bwd_fuse()
                    and not _cfg.deterministic(self.dname) and all(o.is_set() for (_c, _w, o) in parts)
                    and (single or (len(parts) == 2 and all(cw == 64 for (_c, cw, _o) in parts)))
                    and L.lib().ydl_conv_bwd_pw_bn_supported(gp, self.dt) and getattr(m, "pw_bn_ready", lambda: False)()):
                self._bw_pw_bn(m, x, y, cf, parts, res, res_mode, act, geom, wt, npix, st2)
                return
            dy = self.new(x.N, Cout, Ho, Wo)
            rows = gw, gb, accw = self._bn_grad_rows(m, Cout_p)
            for (co, cw, o) in parts:
                cp = round_up(cw, 8)
                if not o.is_set():                        # this half feeds nothing that reaches the loss
                    zero_(dy.t if single else dy.t[:, co:co + cw])
                    continue
                if not sums_mode:
                    self._bn_bwd_rows(m, y, cf, act, o, res, res_mode, dy, rows, npix, cw, cp, st2, c0=co, touch=False)
                    continue
                dout = self._gbuf(o)
                dres_t, dres_ld, rmode = self._res_grad(res, res_mode, o, dout)
                red = o.bnred
                o.bnred = None
                if red is not None and self._unwritten_since(o, red[1]):
                    # the reduce pass ran in the epilogue of the dgrad that wrote dout last (nothing has written since)
                    entry, sums_b = "ydl_bn_act_bwd_apply_sums", red[0]
                else:
                    entry, sums_b = "ydl_bn_act_bwd_sums", self.zeroed(L.BN_REPLICAS * 2 * cp)
                yp, mean, invstd, scale, shift = _bn_part(y, cf, co)
                L.call_act(entry, self.dt, yp, y.ld, _p(dout), o.ld, _p(o.t), o.ld, mean, invstd, scale, shift, rmode, act,
                           _at(dy.t, co), dy.ld, _p(dres_t), dres_ld, _at(gw, co), _at(gb, co), accw, _p(sums_b), npix, cw, cp, st2)
            m.touch_bn()          # dgamma / dbeta kernels are enqueued: the DP hook may now reduce their bucket
            # weight gradient (f32, KRSC) accumulated into the parameter's grad storage; on the side stream when the
            # input gradient is needed too, so wgrad and dgrad of a layer overlap
            if subs is not None:
                self._bw_split(m, subs, dy, wt, Cout_p, Ho, Wo, st2)
                return
            if (train_w and x.need and not _cfg.bn_bwd_fuse() and _cfg.fuse_pw_backward() and not _cfg.deterministic(self.dname)
                    and L.lib().ydl_conv_bwd_pw_supported(gp, self.dt)):
                # HBM-bound 1x1 layer: input and weight gradient in ONE pass over dy, on the main stream (ydl_conv_bwd_pw)
                gx, acc = self.grad_target(x)
                if m.wgrad(self, gp, x, dy, st2, fuse=(_p(wt), _p(gx), x.ld, acc)):
                    self._keep.append(geom)
                    return
                L.call("ydl_conv_dgrad", gp, self.dt, _p(dy.t), _p(wt), _p(gx), acc, st2)     # (the weight gradient ran alone)
                return
            if not train_w:
                pass                                       # frozen weight: no weight-gradient launch, never marked touched
            elif x.need and _cfg.overlap_wgrad():
                # dy was allocated on the main stream and would die with this closure while the side stream still reads
                # it: park the reference until the streams are joined at the end of run_backward (graph-capture safe,
                # unlike Tensor.record_stream)
                self._defer_wgrad(lambda sst: m.wgrad(self, gp, x, dy, sst), keep=(dy, geom))
            else:
                m.wgrad(self, gp, x, dy, st2)
            if x.need:
                gx, acc = self.grad_target(x)
                if not self._try_bnred(x, gp, dy, wt, gx, acc, st2):
                    L.call("ydl_conv_dgrad", gp, self.dt, _p(dy.t), _p(wt), _p(gx), acc, st2)
            self._keep.append(geom)     # the ctypes struct outlives the enqueue

        self.bw.append(bw)
        return ret

    def conv_bias_act(self, x: Var, m, act: int, res: Optional[Var] = None, res_mode: int = L.RES_NONE) -> Var:
        """eval-only folded Conv (``Conv.forward_fuse``, models/common.py:61-64): act(conv(x, w') + b') [+ res]"""
        if self.record:
            raise RuntimeError("a fused (BN-folded) Conv is inference-only")
        x = self._flat(x)
        if res is not None:
            res = self._flat(res)
        k, s, p = m.k, m.s, m.p
        Ho, Wo = _out_size(x.H, k, s, p), _out_size(x.W, k, s, p)
        out = self.new(x.N, m.c2, Ho, Wo)
        w, _wt = m._fused_weights(self)
        geom = L.ConvGeom(x.N, x.H, x.W, m.c1, Ho, Wo, m.c2, k, s, p, x.ld, out.ld, 0)
        f = m._fused
        self._conv_shift_fwd(ctypes.byref(geom), x, w, out, lambda _dev: (f["ones"], f["bias"]), _stream(), act, res, res_mode)
        return out

    def _fwd_split(self, subs, w: torch.Tensor, y: Var, Cin_p: int, ws_ptr, fwd_entry: str, sums_mode: bool, st) -> None:
        """forward of the commuted conv-over-concat into ``y``: per source one 1x1 convolution on its column block of the weight matrix;
        the resized source runs at its own size and is then resized into y.  Default order: the resize initialises y, the plain
        sub-convolutions accumulate, the last of them with the statistics (``fwd_entry``, ``ws_ptr``).
        ``config.resize_last`` in replica-sums mode: the plain sub-convolutions first (the first one overwrites y, no statistics), the
        resized source LAST through ydl_resize_acc_sums — a streaming read-modify-write that also adds the statistics of the sum.
        (The default order costs a full write of the resized tensor plus the point-wise kernel's register-layout read-modify-write with
        statistics: 42 + 94 us against 48 + ~45 us for the 128-channel 160^2 case of config 2.)"""
        Cout, es = y.C, w.element_size()
        resize_last = sums_mode and ws_ptr is not None and _cfg.resize_last() and sum(1 for e in subs if e[2]) == 1 and len(subs) >= 2
        if resize_last:
            subs = sorted(subs, key=lambda e: e[2])
        first = True
        for i, (v, c0_, r_, gv) in enumerate(subs):
            wv = ctypes.c_void_p(w.data_ptr() + c0_ * es)
            if r_:
                z = self.new(v.N, Cout, v.H, v.W)
                gz = L.ConvGeom(v.N, v.H, v.W, v.C, v.H, v.W, Cout, 1, 1, 0, v.ld, z.ld, Cin_p)
                L.call("ydl_conv_fwd", ctypes.byref(gz), self.dt, _p(v.t), wv, _p(z.t), None, 0, st)
                if resize_last:
                    L.call("ydl_resize_acc_sums", self.dt, L.RESIZE_BILINEAR, _p(z.t), z.ld, _p(y.t), y.ld, v.N, v.H, v.W, y.H, y.W,
                           Cout, 0.0, 0.0, ws_ptr, round_up(Cout, 8), st)
                else:
                    L.call("ydl_resize_fwd", self.dt, L.RESIZE_BILINEAR, _p(z.t), z.ld, _p(y.t), y.ld, v.N, v.H, v.W, y.H, y.W,
                           Cout, 0.0, 0.0, st)
            else:
                stats = ws_ptr is not None and not resize_last and i == len(subs) - 1
                L.call(fwd_entry if stats else "ydl_conv_fwd", ctypes.byref(gv), self.dt, _p(v.t), wv, _p(y.t),
                       ws_ptr if stats else None, 0 if first else 1, st)
            first = False

    def _bw_pw_bn(self, m, x: Var, y: Var, cf, parts, res: Optional[Var], res_mode: int, act: int, geom, wt: torch.Tensor,
                  npix: int, st2) -> None:
        """backward of a 1x1 layer whose dy has ONE reader, the one-pass 1x1 backward: only the reduce pass of the BatchNorm backward is
        launched (it also serves the residual operand), ydl_conv_bwd_pw_bn forms dy from y and dout itself and writes dgamma / dbeta;
        no dy buffer.  ``parts`` = (channel offset, width, destination) of one output or of two 64-channel halves."""
        gw, gb, accw = self._bn_grad_rows(m, round_up(y.C, 8))
        seg = []
        for (co, cw, o) in parts:
            o.bnred = None
            dout = self._gbuf(o)
            dres_t, dres_ld, rmode = self._res_grad(res, res_mode, o, dout)
            sums_b = self.zeroed(L.BN_REPLICAS * 2 * cw)
            yp, mean, invstd, scale, shift = _bn_part(y, cf, co)
            L.call_act("ydl_bn_act_bwd_reduce_sums", self.dt, yp, y.ld, _p(dout), o.ld, _p(o.t), o.ld, mean, invstd, scale, shift,
                       rmode, act, _p(dres_t), dres_ld, _p(sums_b), npix, cw, cw, st2)
            seg.append((dout, o.ld, sums_b))
        if len(parts) == 1:
            seg.append((None, 0, None))
        gx, acc = self.grad_target(x)
        bn = (_p(y.t), y.ld, _p(seg[0][0]), seg[0][1], _p(seg[1][0]), seg[1][1], _p(cf["mean"]), _p(cf["invstd"]),
              _p(cf["scale"]), _p(cf["shift"]), _p(seg[0][2]), _p(seg[1][2]), npix, act, _p(gw), _p(gb), accw, None, 0)
        m.wgrad(self, ctypes.byref(geom), x, None, st2, fuse=(_p(wt), _p(gx), x.ld, acc, bn))
        m.touch_bn()          # after the launch that writes dgamma / dbeta
        self._keep.append((geom, seg))

    def _bw_split(self, m, subs, dy: Var, wt: torch.Tensor, Cout_p: int, Ho: int, Wo: int, st2) -> None:
        """backward of the commuted conv-over-concat: per source one wgrad into its column block of the weight gradient
        and one dgrad with its row block of wt; the resized source sees d z = bilinear_up^T (dy)."""
        es = wt.element_size()
        jobs = []
        for (v, c0_, r_, gv) in subs:
            d = dy
            if r_:
                d = self.new(v.N, dy.C, v.H, v.W)
                L.call("ydl_resize_bwd", self.dt, L.RESIZE_BILINEAR, _p(dy.t), dy.ld, _p(d.t), d.ld, 0,
                       v.N, v.H, v.W, Ho, Wo, dy.C, 0.0, 0.0, st2)
                gv = L.ConvGeom(v.N, v.H, v.W, v.C, v.H, v.W, dy.C, 1, 1, 0, v.ld, d.ld, gv.ldw)
            jobs.append((v, c0_, gv, d))
        overlap = _cfg.overlap_wgrad() and any(v.need for (v, _c, _g, _d) in jobs)
        fused = set()
        if (m.trainable()[0] and not _cfg.bn_bwd_fuse() and _cfg.fuse_pw_backward() and not _cfg.deterministic(self.dname)):
            # sources whose column block is an HBM-bound 128 -> 128 layer of its own: both gradients in one pass (ydl_conv_bwd_pw)
            todo = [i for i, (v, c0_, gv, d) in enumerate(jobs)
                    if v.need and L.lib().ydl_conv_bwd_pw_supported(ctypes.byref(gv), self.dt)]
            rest = [i for i in range(len(jobs)) if i not in todo]
            for i in todo:
                v, c0_, gv, d = jobs[i]
                gx, acc = self.grad_target(v)
                wtv = ctypes.c_void_p(wt.data_ptr() + c0_ * Cout_p * es)
                if m.wgrad(self, ctypes.byref(gv), v, d, st2, col0=c0_, final=(not rest and i == todo[-1]), fuse=(wtv, _p(gx), v.ld, acc)):
                    fused.add(i)
                else:
                    L.call("ydl_conv_dgrad", ctypes.byref(gv), self.dt, _p(d.t), wtv, _p(gx), acc, st2)
                    fused.add(i)
            if fused:
                self._keep.append(tuple(g for (_v, _c, g, _d) in jobs))
                jobs = [jobs[i] for i in rest]
                if not jobs:
                    return
        if not m.trainable()[0]:
            pass                                           # frozen weight
        elif overlap:
            def launch(sst, jobs=jobs):
                for i, (v, c0_, gv, d) in enumerate(jobs):
                    m.wgrad(self, ctypes.byref(gv), v, d, sst, col0=c0_, final=(i == len(jobs) - 1))
            self._defer_wgrad(launch, keep=[d for (_v, _c, _g, d) in jobs] + [dy])
        else:
            for i, (v, c0_, gv, d) in enumerate(jobs):
                m.wgrad(self, ctypes.byref(gv), v, d, st2, col0=c0_, final=(i == len(jobs) - 1))
        for (v, c0_, gv, d) in jobs:
            if v.need:
                gx, acc = self.grad_target(v)
                wtv = ctypes.c_void_p(wt.data_ptr() + c0_ * Cout_p * es)
                L.call("ydl_conv_dgrad", ctypes.byref(gv), self.dt, _p(d.t), wtv, _p(gx), acc, st2)
        self._keep.append(tuple(g for (_v, _c, g, _d) in jobs))      # ctypes structs outlive the enqueue

    # ------------------------------------------------------------------ pooling / resize / copies
    def maxpool(self, x: Var, k: int, s: int, p: int, out: Optional[Var] = None) -> Var:
        x = self._flat(x)
        Ho, Wo = _out_size(x.H, k, s, p), _out_size(x.W, k, s, p)
        if out is not None and not out.aligned():
            return self.copy(self.maxpool(x, k, s, p), out)
        if out is None:
            out = self.new(x.N, x.C, Ho, Wo, f32=(x.dt == L.YDL_F32))
        Cp = round_up(x.C, 4 if x.dt == L.YDL_F32 else 8)
        idx = torch.empty((x.N * Ho * Wo * Cp,), dtype=torch.uint8, device=self.device) if self.record else None
        L.call("ydl_maxpool_fwd", x.dt, _p(x.t), x.ld, _p(out.t), out.ld, _p(idx), x.N, x.H, x.W, Ho, Wo, x.C,
               k, s, p, _stream())
        if self.record:
            self._use(x)              # (noted whether or not x wants a gradient, unlike ``_record``'s notes)

        def bw():
            if x.need:
                gx, acc = self.grad_target(x)
                L.call("ydl_maxpool_bwd", x.dt, _p(self._gbuf(out)), out.ld, _p(idx), _p(gx), x.ld, acc,
                       x.N, x.H, x.W, Ho, Wo, x.C, k, s, p, _stream())
        return self._record(out, bw)

    def sppf_pools(self, x: Var, k: int, outs: Sequence[Var]) -> Sequence[Var]:
        """SPPF's chain y1 = mp(x), y2 = mp(y1), y3 = mp(y2) (k x k, stride 1, pad k//2; seg_diceloss_yolov5.py:468-481) into the
        three given destinations (concat slices): one LDS-resident launch per direction when the plane fits
        (ydl_sppf_pool_fwd / _bwd, bit-identical to the chain), otherwise three ``maxpool`` calls."""
        o1, o2, o3 = outs
        x = self.materialize(x)

        def chain_bw(idx, st):
            # a slice without a gradient (dead consumer): the chain link by link, as three maxpool closures would run it
            for src, dst, ix in ((o2, o3, idx[2]), (o1, o2, idx[1]), (x, o1, idx[0])):
                if not dst.is_set() or not src.need:
                    continue
                gx, acc = self.grad_target(src)
                L.call("ydl_maxpool_bwd", x.dt, _p(self._gbuf(dst)), dst.ld, _p(ix), _p(gx), src.ld, acc,
                       x.N, x.H, x.W, x.H, x.W, x.C, k, 1, k // 2, st)
        idx = self._pools3("ydl_sppf_pool", x, outs, [k], chain_bw) if k % 2 == 1 else None
        if idx is None:
            s1 = self.maxpool(x, k, 1, k // 2, out=o1)
            s2 = self.maxpool(s1, k, 1, k // 2, out=o2)
            s3 = self.maxpool(s2, k, 1, k // 2, out=o3)
            return s1, s2, s3
        hook = _cfg.sppf_argmax_hook()
        if self.record and hook is not None:          # test instrument: read or replace the three arg-max planes the backward will route by
            hook(idx)
        return o1, o2, o3

    def spp_pools(self, x: Var, ks: Sequence[int], outs: Sequence[Var]) -> Sequence[Var]:
        """The parallel pyramid of SPP / SPPCSPC (models/common.py:1282-1286, :1439-1446): outs[i] = max-pool(x; ks[i], stride 1,
        pad ks[i] // 2), every pool of the same x, into the given destinations (concat slices).  Three pools whose plane fits run as
        one LDS-resident launch per direction (ydl_spp_pool_fwd / _bwd, bit-identical to the separate pools); any other tuple
        length, and planes that do not fit, take one ``maxpool`` call per k."""
        ks = [int(k) for k in ks]
        if len(ks) != len(outs):
            raise ValueError(f"spp_pools: {len(ks)} window sizes for {len(outs)} destinations")
        x = self.materialize(x)

        def each_bw(idx, st):
            # a slice without a gradient (dead consumer): pool by pool, in the order the fused kernel sums them
            for k, dst, ix in zip(ks, outs, idx):
                if not dst.is_set() or not x.need:
                    continue
                gx, acc = self.grad_target(x)
                L.call("ydl_maxpool_bwd", x.dt, _p(self._gbuf(dst)), dst.ld, _p(ix), _p(gx), x.ld, acc,
                       x.N, x.H, x.W, x.H, x.W, x.C, k, 1, k // 2, st)
        if len(ks) != 3 or self._pools3("ydl_spp_pool", x, outs, ks, each_bw) is None:
            x = self._flat(x)
            return tuple(self.maxpool(x, k, 1, k // 2, out=o) for k, o in zip(ks, outs))
        return tuple(outs)

    def _pools3(self, entry: str, x: Var, outs: Sequence[Var], ks: Sequence[int], part_bw) -> Optional[list]:
        """what ``sppf_pools`` (``entry`` "ydl_sppf_pool", ks = [k]) and ``spp_pools`` ("ydl_spp_pool", three ks) share, the one-launch
        form of three stride-1 pools into three destinations: None when x, the destinations or the plane do not qualify; otherwise
        the fused forward launch with its three arg-max planes (returned) and a backward that is the one fused launch when every
        destination holds a gradient and x wants one, and else ``part_bw(planes, stream)``, the caller's own pool-wise order"""
        o1 = outs[0]
        if not (x.aligned() and all(o.aligned() and o.ld == o1.ld and o.dt == x.dt for o in outs)
                and all((o.N, o.C, o.H, o.W) == (x.N, x.C, x.H, x.W) for o in outs)
                and getattr(L.lib(), entry + "_supported")(x.dt, x.H, x.W, x.C, *ks)):
            return None
        Cp = round_up(x.C, 4 if x.dt == L.YDL_F32 else 8)
        n = x.N * x.H * x.W * Cp
        idx = [torch.empty((n,), dtype=torch.uint8, device=self.device) for _ in range(3)] if self.record else [None] * 3
        L.call(entry + "_fwd", x.dt, _p(x.t), x.ld, *[_p(o.t) for o in outs], o1.ld, *[_p(i) for i in idx], x.N, x.H, x.W, x.C, *ks,
               _stream())
        if self.record:
            self._use(x)

            def bw():
                st = _stream()
                if not (all(o.is_set() for o in outs) and x.need):
                    return part_bw(idx, st)
                gs = [_p(self._gbuf(o)) for o in outs]
                gx, acc = self.grad_target(x)
                L.call(entry + "_bwd", x.dt, *gs, o1.ld, *[_p(i) for i in idx], _p(gx), x.ld, acc, x.N, x.H, x.W, x.C, *ks, st)
            self.bw.append(bw)
        return idx

    def resize(self, x: Var, Ho: int, Wo: int, mode: int, scale_h: float = 0.0, scale_w: float = 0.0,
               out: Optional[Var] = None) -> Var:
        """mode: L.RESIZE_NEAREST / RESIZE_BILINEAR (align_corners=False) / RESIZE_BILINEAR_AC (True) / RESIZE_BICUBIC (False) /
        RESIZE_BICUBIC_AC (True)."""
        x = self._flat(x)
        if out is not None and not out.aligned():
            return self.copy(self.resize(x, Ho, Wo, mode, scale_h, scale_w), out)
        if out is None:
            out = self.new(x.N, x.C, Ho, Wo, f32=(x.dt == L.YDL_F32))
        # bicubic has entry points of its own (their second argument is align_corners); ydl_resize_* serve modes 0..2
        cubic = mode in (L.RESIZE_BICUBIC, L.RESIZE_BICUBIC_AC)
        fwd, bwd, arg = ("ydl_bicubic_fwd", "ydl_bicubic_bwd", int(mode == L.RESIZE_BICUBIC_AC)) if cubic else ("ydl_resize_fwd", "ydl_resize_bwd", mode)
        L.call(fwd, x.dt, arg, _p(x.t), x.ld, _p(out.t), out.ld, x.N, x.H, x.W, Ho, Wo, x.C,
               scale_h, scale_w, _stream())

        def bw():
            if x.need:
                gx, acc = self.grad_target(x)
                L.call(bwd, x.dt, arg, _p(self._gbuf(out)), out.ld, _p(gx), x.ld, acc,
                       x.N, x.H, x.W, Ho, Wo, x.C, scale_h, scale_w, _stream())
        return self._record(out, bw)

    def copy(self, x: Var, out: Var) -> Var:
        """out[:] = x (channel-slice aware); backward adds d(out) into d(x)."""
        if x.lazy or x.virtual:
            return self.materialize(x, out=out)
        L.call("ydl_copy2d", x.dt, _p(x.t), x.ld, _p(out.t), out.ld, x.npix, x.C, 0, _stream())

        def bw():
            if x.need:
                gx, acc = self.grad_target(x)
                L.call("ydl_copy2d", x.dt, _p(self._gbuf(out)), out.ld, _p(gx), x.ld, x.npix, x.C, acc, _stream())
        return self._record(out, bw)

    def add(self, a: Var, b: Var, out: Optional[Var] = None) -> Var:
        """out = a + b (element-wise, same shape); backward hands d(out) to both.  ``out`` may be a concat slice."""
        a, b = self._flat(a) if (a.lazy or a.virtual) else a, self._flat(b) if (b.lazy or b.virtual) else b
        out = self._out("add", (a.N, a.C, a.H, a.W), out, f32=(a.dt == L.YDL_F32))
        st = _stream()
        L.call("ydl_copy2d", a.dt, _p(a.t), a.ld, _p(out.t), out.ld, a.npix, a.C, 0, st)
        L.call("ydl_copy2d", b.dt, _p(b.t), b.ld, _p(out.t), out.ld, b.npix, b.C, 1, st)

        def bw():
            for v in (a, b):
                if v.need:
                    gv, acc = self.grad_target(v)
                    L.call("ydl_copy2d", v.dt, _p(self._gbuf(out)), out.ld, _p(gv), v.ld, v.npix, v.C, acc, _stream())
        return self._record(out, bw)

    # ------------------------------------------------------------------ space-to-depth / depth-to-space (csrc/s2d.hip)
    def _block_permute(self, x: Var, s: int, order: int, out: Optional[Var], down: bool) -> Var:
        """the body of ``space_to_depth`` (``down``) and ``depth_to_space``: one launch each way, the backward is the opposite entry
        point into x's gradient with its accumulate flag.  The launcher picks the 16-byte or the element-granular kernel from the raw
        pointers and strides, so an odd channel slice on either side needs no staging copy."""
        who = "space_to_depth" if down else "depth_to_space"
        x = self.materialize(x)
        s, ss = int(s), int(s) * int(s)
        if s < 1 or order not in (0, 1):
            raise RuntimeError(f"{who}: s={s} must be >= 1 and order={order} 0 or 1")
        if down:
            if x.H % s or x.W % s:
                raise RuntimeError(f"{who}: the {x.H} x {x.W} map is not a multiple of s={s}")
            C, shape = x.C, (x.N, x.C * ss, x.H // s, x.W // s)
        else:
            if x.C % ss:
                raise RuntimeError(f"{who}: {x.C} channels are not a multiple of s*s={ss}")
            C, shape = x.C // ss, (x.N, x.C // ss, x.H * s, x.W * s)
        out = self._out(who, shape, out, need=x.need, f32=(x.dt == L.YDL_F32))
        if out.dt != x.dt:
            raise RuntimeError(f"{who}: the output slice has the wrong dtype")
        fwd, bwd = ("ydl_space_to_depth", "ydl_depth_to_space") if down else ("ydl_depth_to_space", "ydl_space_to_depth")
        L.call(fwd, x.dt, _p(x.t), x.ld, _p(out.t), out.ld, x.N, x.H, x.W, C, s, order, 0, _stream())
        if not x.need:                                # the external image: nothing upstream wants a gradient
            return out

        def bw():
            gx, acc = self.grad_target(x)
            L.call(bwd, x.dt, _p(self._gbuf(out)), out.ld, _p(gx), x.ld, out.N, out.H, out.W, C, s, order, acc, _stream())
        return self._record(out, bw, uses=(x,))

    def space_to_depth(self, x: Var, s: int, order: int = 0, out: Optional[Var] = None) -> Var:
        """(N, C, H, W) -> (N, s*s*C, H/s, W/s): out channel blk*C + c of pixel (ho, wo) is x's channel c at (ho*s + sy, wo*s + sx), with
        blk = sy*s + sx (``order`` 0: Contract, models/common.py:282-293) or sx*s + sy (``order`` 1: Focus's concat, :241-250).  ``out`` may
        be a concat slice."""
        return self._block_permute(x, s, order, out, True)

    def depth_to_space(self, x: Var, s: int, order: int = 0, out: Optional[Var] = None) -> Var:
        """(N, s*s*C, H, W) -> (N, C, H*s, W*s), the inverse of ``space_to_depth`` (``order`` 0: Expand, models/common.py:296-307)"""
        return self._block_permute(x, s, order, out, False)

    def bn_act(self, x: Var, m, act: int, out: Optional[Var] = None) -> Var:
        """out = act(bn(x)) of an existing tensor: BatchNorm that is not the epilogue of its own convolution (a bare nn.BatchNorm2d
        row).  ``m`` holds ``m.bn`` like a Conv.  Train mode: ydl_bn_stats -> ydl_bn_finalize -> ydl_bn_act_fwd; eval mode:
        ydl_bn_eval_coeffs -> ydl_bn_act_fwd.  The backward is ydl_bn_act_bwd straight into x's gradient, or through a buffer that is
        added to it when x has other consumers."""
        x = self._flat(x)
        if out is not None and not out.aligned():        # the BatchNorm kernels work on 8-channel groups: stage an odd slice
            return self.copy(self.bn_act(x, m, act), out)
        C, cp, npix = x.C, round_up(x.C, 8), x.npix
        if C != m.bn.num_features:
            raise RuntimeError(f"BatchNorm2d input channel mismatch: got {C}, the layer has {m.bn.num_features}")
        out = self._out("bn_act", (x.N, C, x.H, x.W), out)
        st = _stream()
        cf = m.coeffs(self.device)
        if self.train:
            lib = L.lib()
            bm = lib.ydl_bn_stats_block_m()
            ws = self._ws(lib.ydl_bn_stats_ws_bytes(npix, C))
            L.call("ydl_bn_stats", self.dt, _p(x.t), x.ld, _p(ws), npix, C, st)
            self._bn_coeffs(m, cf, C, st, (ws, (npix + bm - 1) // bm, bm, npix, 1))
        else:
            self._bn_coeffs(m, cf, C, st)
        self._bn_apply(x, cf["scale"], cf["shift"], act, out, npix, cp, st)
        if not self.record:
            return out
        if not self.train:
            raise RuntimeError("backward through eval-mode BatchNorm is not supported")

        def bw():
            if not (x.need or any(m.trainable()[1:])):
                return
            st2 = _stream()
            # first writer of d/dx: the pass writes it in place; otherwise (or when nobody wants it) into a buffer of its own
            self._grad_via(x, lambda dy: self._bn_bwd_rows(m, x, cf, act, out, None, L.RES_NONE, dy, self._bn_grad_rows(m, cp), npix, C,
                                                           cp, st2), st2)
        return self._record(out, bw, uses=(x,))

    # ------------------------------------------------------------------ learnable activations (csrc/act.hip)
    def acon(self, z: Var, m, out: Optional[Var] = None) -> Var:
        """AconC behind a materialised BatchNorm output: out = d * sigmoid(beta * d) + p2 * z, d = (p1 - p2) * z, with ``m.p1``,
        ``m.p2``, ``m.beta`` of shape (1, C, 1, 1) (utils/activations.py).  The backward is one pass (ydl_acon_bwd): dz and the three
        per-channel sums, added into the parameters' gradient rows."""
        z = self._flat(z)
        if out is not None and not out.aligned():
            return self.copy(self.acon(z, m), out)
        C, cp, hw = z.C, round_up(z.C, 8), z.H * z.W
        out = self._out("acon", (z.N, C, z.H, z.W), out)
        ps = (m.p1, m.p2, m.beta)
        if any(p.numel() != C or not p.is_contiguous() or p.dtype != torch.float32 for p in ps):
            raise RuntimeError(f"acon: p1 / p2 / beta must be contiguous f32 rows of {C} channels")
        L.call("ydl_acon_fwd", self.dt, _p(z.t), z.ld, _p(ps[0]), _p(ps[1]), _p(ps[2]), 0, _p(out.t), out.ld, z.npix, hw, C, cp, _stream())

        def bw():
            st = _stream()
            g1, g2, gb = (self._param_grad(p, self.device) for p in ps)
            ws = self._ws(L.lib().ydl_acon_bwd_ws_bytes(z.npix, hw, 0, cp))
            gz, ldz, acc = self._grad_or_scratch(z)   # (nothing upstream wants dz: the pass still forms the parameter sums)
            L.call("ydl_acon_bwd", self.dt, _p(z.t), z.ld, _p(self._gbuf(out)), out.ld, _p(ps[0]), _p(ps[1]), _p(ps[2]), 0,
                   _p(gz), ldz, acc, _p(g1), _p(g2), _p(gb), 1, _p(ws), z.npix, hw, C, cp, st)
            self._touch(*ps)
        return self._record(out, bw, uses=(z,))

    def max2(self, a: Var, b: Var, out: Optional[Var] = None) -> Var:
        """out = max(a, b) element-wise (FReLU's merge); the backward routes d(out) to the larger operand, half to each on a tie"""
        a, b = self._flat(a), self._flat(b)
        if (a.N, a.C, a.H, a.W) != (b.N, b.C, b.H, b.W):
            raise RuntimeError("max2: operands differ in shape")
        if out is not None and not out.aligned():
            return self.copy(self.max2(a, b), out)
        cp = round_up(a.C, 8)
        out = self._out("max2", (a.N, a.C, a.H, a.W), out)
        L.call("ydl_max2_fwd", self.dt, _p(a.t), a.ld, _p(b.t), b.ld, _p(out.t), out.ld, a.npix, cp, _stream())

        def bw():
            if not (a.need or b.need):
                return
            ga, acca = self.grad_target(a) if a.need else (None, 0)
            gb, accb = self.grad_target(b) if b.need else (None, 0)
            L.call("ydl_max2_bwd", self.dt, _p(a.t), a.ld, _p(b.t), b.ld, _p(self._gbuf(out)), out.ld, _p(ga), a.ld, acca,
                   _p(gb), b.ld, accb, a.npix, cp, _stream())
        return self._record(out, bw, uses=(a, b))

    # ------------------------------------------------------------------ ConvNeXt pieces (csrc/convnext.hip)
    def dw_conv(self, x: Var, m) -> Var:
        """plain depth-wise k x k convolution, stride 1, padding k // 2, no BatchNorm: ydl_dwconv2_fwd without its statistics rows.
        ``m`` holds the [C][k*k] master (``master_dw`` / ``grad_dw``); its bias, if any, belongs to the consumer
        (``layer_norm(pre_bias=...)``)."""
        x = self._flat(x)
        C, k = x.C, m.k
        y = self.new(x.N, C, x.H, x.W)
        L.call("ydl_dwconv2_fwd", self.dt, _p(x.t), x.ld, _p(m.master_dw()), _p(y.t), y.ld, None, x.N, x.H, x.W, C, k, 1, _stream())

        def bw():
            st = _stream()
            dy = self._gbuf(y)
            if m.weight.requires_grad:
                ws = self._ws(L.lib().ydl_dwconv2_wgrad_ws_bytes(C, k))
                L.call("ydl_dwconv2_wgrad", self.dt, _p(x.t), x.ld, _p(dy), y.ld, _p(m.grad_dw()), _p(ws), x.N, x.H, x.W, C, k, 1, st)
                self._touch(m.weight)
            if x.need:
                gx, acc = self.grad_target(x)
                L.call("ydl_dwconv2_dgrad", self.dt, _p(dy), y.ld, _p(m.master_dw()), _p(gx), x.ld, acc, x.N, x.H, x.W, C, k, 1, st)
        return self._record(y, bw, uses=(x,))

    def layer_norm(self, x: Var, m, pre_bias=None, out: Optional[Var] = None) -> Var:
        """LayerNorm over the channels of every pixel: out = (u - mean_c u) / sqrt(var_c u + m.eps) * m.weight + m.bias with
        u = x + pre_bias (``pre_bias``: an f32 [C] parameter, the bias of the depth-wise convolution in front, or None).  One launch
        each way (ydl_ln_fwd / ydl_ln_bwd); the backward adds the three per-channel sums into the parameters' gradients."""
        x = self._flat(x)
        C = x.C
        if not L.lib().ydl_ln_supported(C):
            raise RuntimeError(f"layer_norm: {C} channels are outside the served set (a multiple of 8 in 8..1024)")
        ps = (m.weight, m.bias) + ((pre_bias,) if pre_bias is not None else ())
        if any(p.numel() != C or not p.is_contiguous() or p.dtype != torch.float32 for p in ps):
            raise RuntimeError(f"layer_norm: weight / bias / pre_bias must be contiguous f32 rows of {C} channels")
        out = self._out("layer_norm", (x.N, C, x.H, x.W), out, aligned=True)
        stats = torch.empty((x.npix, 2), dtype=torch.float32, device=self.device) if self.record else None
        L.call("ydl_ln_fwd", self.dt, _p(x.t), x.ld, _p(pre_bias), _p(m.weight), _p(m.bias), float(m.eps), _p(out.t), out.ld, _p(stats),
               x.npix, C, _stream())

        def bw():
            gg, gb = self._param_grad(m.weight, self.device), self._param_grad(m.bias, self.device)
            gp = self._param_grad(pre_bias, self.device) if pre_bias is not None else None
            ws = self._ws(L.lib().ydl_ln_bwd_ws_bytes(x.npix, C))
            gx, ldx, acc = self._grad_or_scratch(x)
            L.call("ydl_ln_bwd", self.dt, _p(x.t), x.ld, _p(pre_bias), _p(m.weight), _p(stats), _p(self._gbuf(out)), out.ld, _p(gx), ldx,
                   acc, _p(gg), _p(gb), _p(gp), _p(ws), x.npix, C, _stream())
            self._touch(*ps)
        return self._record(out, bw, uses=(x,))

    def bias_gelu(self, z: Var, m) -> Var:
        """out = GELU(z + m.bias), the exact (erf) form; ``z`` is the output of the bias-free GEMM in front.  Backward: one pass
        (ydl_bias_gelu_bwd) gives dz and adds the bias gradient into ``m.bias.grad``."""
        z = self._flat(z)
        C, b = z.C, m.bias
        if C % 8 or b.numel() != C or not b.is_contiguous() or b.dtype != torch.float32:
            raise RuntimeError(f"bias_gelu: the bias must be a contiguous f32 row of {C} channels, a multiple of 8")
        out = self.new(z.N, C, z.H, z.W)
        L.call("ydl_bias_gelu_fwd", self.dt, _p(z.t), z.ld, _p(b), _p(out.t), out.ld, z.npix, C, _stream())

        def bw():
            st = _stream()
            dy = Var(self, self._gbuf(out), out.ld, False)
            ws = self._ws(L.lib().ydl_bias_gelu_bwd_ws_bytes(z.npix, C))
            # first writer of d/dz: straight into it; otherwise in place over dy, then added (or dropped when nobody wants it)
            self._grad_via(z, lambda dz: L.call("ydl_bias_gelu_bwd", self.dt, _p(z.t), z.ld, _p(b), _p(dy.t), dy.ld, _p(dz.t), dz.ld,
                                                _p(self._param_grad(b, self.device)), _p(ws), z.npix, C, st), st, aside=dy)
            self._touch(b)
        return self._record(out, bw, uses=(z,))

    def scale_residual(self, y: Var, m, keep: Optional[torch.Tensor], x: Var, gamma: Optional[torch.Tensor] = None) -> Var:
        """out = x + keep[n] * m.layer_scale[c] * y: the layer-scaled residual of a ConvNeXt block with the per-sample keep factors of
        stochastic depth (``keep``: f32 [N] on the device, or None for 1).  Backward: d/dy, the layer-scale gradient, and d/dx = d/dout,
        which x adopts without a pass where it can (``_alias_grad``).  ``gamma``: a constant f32 [C] row in place of ``m.layer_scale``
        (MBConv: ones; ``m`` is not read then and the row's gradient goes to a scratch row)."""
        y, x = self._flat(y), self._flat(x)
        C, hw, g = y.C, y.H * y.W, m.layer_scale if gamma is None else gamma
        if C % 8 or (x.N, x.C, x.H, x.W) != (y.N, C, y.H, y.W):
            raise RuntimeError(f"scale_residual: the branch ({C} channels, a multiple of 8) and the residual differ in shape")
        if g.numel() != C or not g.is_contiguous() or g.dtype != torch.float32:
            raise RuntimeError(f"scale_residual: layer_scale must be a contiguous f32 row of {C} channels")
        if keep is not None and (keep.numel() != y.N or keep.dtype != torch.float32 or not keep.is_contiguous()):
            raise RuntimeError(f"scale_residual: keep must hold {y.N} f32 factors")
        out = self.new(y.N, C, y.H, y.W)
        L.call("ydl_scale_res_fwd", self.dt, _p(y.t), y.ld, _p(g), _p(keep), _p(x.t), x.ld, _p(out.t), out.ld, y.N, hw, C, _stream())

        def bw():
            st = _stream()
            dout = self._gbuf(out)
            ws = self._ws(L.lib().ydl_scale_res_bwd_ws_bytes(y.N, hw, C))

            def launch(dy: Var):
                gx, accx = None, 0
                if x.need and not self._alias_grad(x, out, dout):
                    gx, accx = self.grad_target(x)
                dg = self._param_grad(g, self.device) if gamma is None else torch.empty(C, dtype=torch.float32, device=self.device)
                L.call("ydl_scale_res_bwd", self.dt, _p(dout), out.ld, _p(y.t), y.ld, _p(g), _p(keep), _p(dy.t), dy.ld, _p(gx), x.ld, accx,
                       _p(dg), _p(ws), y.N, hw, C, st)
            self._grad_via(y, launch, st)                # (another consumer wrote d/dy first: ours is formed aside, then added)
            if keep is not None:
                self._keep.append(keep)
            if gamma is None:
                self._touch(g)
        return self._record(out, bw, uses=(y, x))

    # ------------------------------------------------------------------ squeeze-and-excitation (csrc/se.hip)
    def squeeze_excite(self, x: Var, m) -> Var:
        """out = x * scale(fc2(act(fc1(mean_hw x))))[n, c], torchvision's SqueezeExcitation: ``m.fc1`` / ``m.fc2`` are the 1x1
        ``nn.Conv2d(C, Cs)`` / ``(Cs, C)`` with bias whose f32 parameters the kernels read as they stand, ``m.act_code`` is ACT_RELU or
        ACT_SILU and ``m.gate_code`` SE_GATE_SIGMOID or SE_GATE_HSIGMOID.  Forward: ydl_se_pool_fwd (partial sums), ydl_se_excite_fwd
        (one launch from the partial rows to the gate; pooled, h and z are kept), ydl_scale_channels.  Backward: the gate gradient
        sum_hw dout * x through ydl_se_pool_fwd's product form, ydl_se_excite_bwd (dpooled and the four parameter gradients), and
        ydl_se_scale_bwd: dx (+)= dout * gate + dpooled / HW, two reads and one write of the tensor."""
        x = self._flat(x)
        N, C, HW = x.N, x.C, x.H * x.W
        fc1, fc2 = m.fc1, m.fc2
        Cs = fc1.out_channels
        lib = L.lib()
        if not lib.ydl_se_supported(C, Cs):
            raise RuntimeError(f"squeeze_excite: C={C}, Cs={Cs} are outside the served set (C a multiple of 8 in 8..2048, Cs in 1..512)")
        ps = (fc1.weight, fc1.bias, fc2.weight, fc2.bias)
        if (fc1.in_channels, fc2.in_channels, fc2.out_channels) != (C, Cs, C) or any(
                p is None or p.dtype != torch.float32 or not p.is_contiguous() for p in ps):
            raise RuntimeError(f"squeeze_excite: fc1 / fc2 must be 1x1 convolutions {C} -> {Cs} -> {C} with contiguous f32 weights and biases")
        f32 = dict(dtype=torch.float32, device=self.device)
        S = lib.ydl_se_pool_splits(N, HW)
        part = self._ws(lib.ydl_se_pool_ws_bytes(N, HW, C))
        pooled, z, gate = torch.empty((3, N, C), **f32).unbind(0)
        h = torch.empty((N, Cs), **f32)
        st = _stream()
        L.call("ydl_se_pool_fwd", self.dt, _p(x.t), x.ld, None, 0, _p(part), N, HW, C, st)
        L.call("ydl_se_excite_fwd", _p(part), S, _p(ps[0]), _p(ps[1]), _p(ps[2]), _p(ps[3]), m.act_code, m.gate_code, _p(pooled), _p(h),
               _p(z), _p(gate), N, HW, C, Cs, st)
        out = self.scale_channels(x, gate)

        def bw():
            if not (x.need or any(p.requires_grad for p in ps)):
                return
            st2 = _stream()
            dout = self._gbuf(out)
            dgate = torch.empty(N * S * C, **f32)
            L.call("ydl_se_pool_fwd", self.dt, _p(dout), out.ld, _p(x.t), x.ld, _p(dgate), N, HW, C, st2)
            grads = [self._param_grad(p, self.device) if p.requires_grad else None for p in ps]
            dpooled = torch.empty((N, C), **f32)
            ws = self._ws(lib.ydl_se_excite_bwd_ws_bytes(N, C, Cs))
            L.call("ydl_se_excite_bwd", _p(dgate), S, _p(pooled), _p(h), _p(z), _p(ps[0]), _p(ps[2]), m.act_code, m.gate_code, _p(dpooled),
                   _p(grads[0]), _p(grads[1]), _p(grads[2]), _p(grads[3]), _p(ws), N, C, Cs, st2)
            self._touch(*ps)
            if x.need:
                gx, acc = self.grad_target(x)
                L.call("ydl_se_scale_bwd", self.dt, _p(dout), out.ld, _p(gate), _p(dpooled), _p(gx), x.ld, acc, N, HW, C, st2)
        return self._record(out, bw, uses=(x,))

    def patch_conv(self, x: Var, m, out: Optional[Var] = None) -> Var:
        """patchify convolution, kernel = stride = ``m.patch``, no padding: ``space_to_depth(x, k, order=0)`` and the 1x1 ``conv_bias``
        over k*k*Cin channels.  The parameter [Cout, Cin, k, k] in channels_last storage IS the [Cout][1][k*k*Cin] master of that 1x1
        (channel (dy*k + dx)*Cin + c): no weight copy, no gradient re-layout.  The model's NCHW image takes the edge conversion
        ``input_s2d`` instead of an interior pass."""
        k = m.patch
        if x.LH % k or x.LW % k:
            raise ValueError(f"{m._wname}: the {x.LH} x {x.LW} map is not a multiple of the patch size {k}")
        if x.ext_src is not None and x.real is None and not x.need:
            xs = self.input_s2d(x.ext_src, k)
        else:
            xs = self.space_to_depth(x, k, order=0)
        return self.conv_bias(xs, m, out=out)

    def concat(self, xs: Sequence[Var], align: bool = True) -> Var:
        """Concat along channels with the reference's auto-align (bilinear, align_corners=False, to the first
        input's size) — seg_diceloss_yolov5.py:484-507.
        When exactly one source has to be up-sampled and everything is 16-byte aligned the result is VIRTUAL (see
        Var.cat_parts): the typical consumer is a 1x1 convolution, which then never needs the up-sampled tensor."""
        xs = [self.materialize(v) if (v.virtual and v.ext_src is not None) else v for v in xs]
        H, W = xs[0].LH, xs[0].LW
        ups = [v for v in xs if (v.LH, v.LW) != (H, W)]
        if (_cfg.commute_concat() and align and len(ups) == 1 and ups[0].LH < H and ups[0].LW < W
                and all(v.C % 8 == 0 and not v.virtual for v in xs) and len({v.dt for v in xs}) == 1):
            Ct = sum(v.C for v in xs)
            ph = torch.empty(1, dtype=self.tdt if xs[0].dt != L.YDL_F32 else torch.float32, device=self.device)
            cat = Var(self, ph.expand(xs[0].N, Ct, H, W), round_up(Ct, 8), any(v.need for v in xs))
            parts, c0 = [], 0
            for v in xs:
                parts.append((v, c0, (v.LH, v.LW) != (H, W)))
                c0 += v.C
            cat.cat_parts = parts
            return cat
        return self._concat_real(xs, align)

    def _concat_real(self, xs: Sequence[Var], align: bool) -> Var:
        """each source is written (copied / bilinearly resized) straight into its channel slice"""
        H, W = xs[0].LH, xs[0].LW
        Ct = sum(v.C for v in xs)
        cat = self.new(xs[0].N, Ct, H, W, f32=(xs[0].dt == L.YDL_F32))
        c0 = 0
        for v in xs:
            sl = cat.slice(c0, c0 + v.C)
            if (v.LH, v.LW) == (H, W):
                self.copy(v, sl)
            elif align:
                self.resize(v, H, W, L.RESIZE_BILINEAR, out=sl)
            else:
                raise RuntimeError("Concat: spatial sizes differ")
            c0 += v.C
        return cat

    # ------------------------------------------------------------------ softmax head
    def softmax(self, x: Var) -> Var:
        """nn.Softmax(1) into an f32 NHWC Var (probabilities stay f32 even in bf16 mode)."""
        if x.virtual:
            x = self.materialize(x)
        out = self.new(x.N, x.C, x.H, x.W, zero=True, f32=True)
        out.rep = x.rep                                   # point-wise: stays lazy
        sn, sc, sh, sw = out.t.stride()
        L.call("ydl_softmax_fwd", x.dt, _p(x.t), x.ld, _p(out.t), sn, sc, sh, sw, x.N, x.H, x.W, x.C, 1, 1, _stream())

        def bw():
            if not x.need:
                return
            dp = self._gbuf(out)
            gx, acc = self.grad_target(x)
            assert acc == 0, "softmax input must have a single consumer"
            L.call("ydl_softmax_bwd", x.dt, _p(out.t), _p(dp), sn, sc, sh, sw, _p(gx), x.ld, x.N, x.H, x.W, x.C, 1, 1,
                   _stream())
        return self._record(out, bw)

    def softmax_nchw(self, x: Var) -> torch.Tensor:
        """nn.Softmax(1) producing the region's external output directly: f32 NCHW contiguous (no extra pass).
        The region owner must call softmax_nchw_backward with the incoming gradient.
        When x is a lazily up-sampled tensor the stored-resolution probabilities are kept as well (``self.lazy_out``):
        SegmentationLoss uses them to evaluate the loss and its gradient per stored pixel (ydl_seg_loss_rep_*).  With
        config.use_fused_seg_tail the stored logits are handed over instead and the probabilities are computed on demand only
        (LazyOutput)."""
        assert not x.virtual
        p = torch.empty((x.N, x.C, x.LH, x.LW), dtype=torch.float32, device=self.device)
        sn, sc, sh, sw = p.stride()
        L.call("ydl_softmax_fwd", x.dt, _p(x.t), x.ld, _p(p), sn, sc, sh, sw, x.N, x.H, x.W, x.C, x.rep[0], x.rep[1],
               _stream())
        self.lazy_out = None
        if x.rep != (1, 1) and self.record:
            if _cfg.use_fused_seg_tail(x.N * x.H * x.W):
                self.lazy_out = LazyOutput(None, x.rep, x)
            else:
                plow = torch.empty((x.N, x.C, x.H, x.W), dtype=torch.float32, device=self.device)
                sn, sc, sh, sw = plow.stride()
                L.call("ydl_softmax_fwd", x.dt, _p(x.t), x.ld, _p(plow), sn, sc, sh, sw, x.N, x.H, x.W, x.C, 1, 1, _stream())
                self.lazy_out = LazyOutput(plow, x.rep)
        return p

    def softmax_nchw_backward(self, x: Var, p: torch.Tensor, dp: torch.Tensor) -> None:
        dp = dp.detach()
        gx, acc = self.grad_target(x)
        assert acc == 0
        lazy = getattr(self, "lazy_out", None)
        dlow = None
        if lazy is not None:
            dlow, lazy.dlow = lazy.dlow, None
            if lazy.tail is not None:
                if all(s == 0 for s in dp.stride()) and getattr(lazy, "dummy", None) is not None:
                    # the loss is the prediction's only consumer: its backward and the soft-max backward in one pass from the logits
                    lazy.dummy = None
                    target, cw, _kind, ls, _eps, ws, counts, g = lazy.tail
                    lazy.tail = None
                    L.call("ydl_seg_tail_bwd", x.dt, _p(x.t), x.ld, _p(counts), _p(target), _p(cw), ls, x.N, x.C, x.H, x.W,
                           x.rep[0], x.rep[1], _p(ws), _p(g), _p(gx), x.ld, _stream())
                    return
                dlow = lazy.tail_dlow()
        if dlow is not None:
            if all(s == 0 for s in dp.stride()) and getattr(lazy, "dummy", None) is not None:
                # the loss already summed its gradient over the replicas: soft-max backward at the stored resolution
                lazy.dummy = None
                sn, sc, sh, sw = lazy.low.stride()
                L.call("ydl_softmax_bwd", x.dt, _p(lazy.low), _p(dlow), sn, sc, sh, sw, _p(gx), x.ld, x.N, x.H, x.W, x.C,
                       1, 1, _stream())
                return
            # pred had other consumers besides the loss: fold the summed part into one replica of the dense gradient
            dp = dp.float().contiguous().clone()
            dp.view(x.N, x.C, x.H, x.rep[0], x.W, x.rep[1])[:, :, :, 0, :, 0] += dlow
        if dp.dtype != torch.float32 or dp.stride() != p.stride():
            dp = dp.float().contiguous()
        sn, sc, sh, sw = p.stride()
        L.call("ydl_softmax_bwd", x.dt, _p(p), _p(dp), sn, sc, sh, sw, _p(gx), x.ld, x.N, x.H, x.W, x.C, x.rep[0], x.rep[1],
               _stream())

    # ------------------------------------------------------------------ GAM pieces
    def global_pool(self, x: Var, kind: str) -> Var:
        """AdaptiveAvgPool2d(1) / AdaptiveMaxPool2d(1) -> (N, C, 1, 1)"""
        x = self.materialize(x)
        avg = self.new(x.N, x.C, 1, 1, zero=True)
        mx = self.new(x.N, x.C, 1, 1, zero=True)
        amax = torch.empty((x.N, round_up(x.C, 8)), dtype=torch.int32, device=self.device)
        HW = x.H * x.W
        L.call("ydl_global_pool_fwd", x.dt, _p(x.t), x.ld, _p(avg.t), avg.ld, _p(mx.t), mx.ld, _p(amax), x.N, HW, x.C,
               _stream())
        out = avg if kind == "avg" else mx

        def bw():
            if not x.need:
                return
            g = self._gbuf(out)
            gx, acc = self.grad_target(x)
            L.call("ydl_global_pool_bwd", x.dt, _p(g) if kind == "avg" else None, out.ld,
                   _p(g) if kind == "max" else None, out.ld, _p(amax), _p(gx), x.ld, acc, x.N, HW, x.C, _stream())
        return self._record(out, bw)

    def _scale_channels_bwd(self, x: Var, out: Var, gate: torch.Tensor, st) -> None:
        """d x (+)= d out * gate[n, c], the backward of ``out = scale_channels(x, gate)`` for x (ydl_scale_channels has no accumulate
        flag: ``_grad_via``)"""
        self._grad_via(x, lambda dx: L.call("ydl_scale_channels", x.dt, _p(self._gbuf(out)), out.ld, _p(gate), _p(dx.t), dx.ld, x.N,
                                            x.H * x.W, x.C, st), st)

    def gate_mul(self, x: Var, a: Var, b: Var) -> Var:
        """out = x * sigmoid(a + b) with a, b of shape (N, C, 1, 1) (GAM: the bilinear expansion of a 1x1 map is constant)"""
        x = self.materialize(x)
        gate = torch.empty((x.N, x.C), dtype=torch.float32, device=self.device)
        L.call("ydl_gate_fwd", x.dt, _p(a.t), a.ld, _p(b.t), b.ld, _p(gate), x.N, x.C, _stream())
        out = self.scale_channels(x, gate)

        def bw():
            st = _stream()
            dgate = torch.empty((x.N, x.C), dtype=torch.float32, device=self.device)
            L.call("ydl_channel_dot", x.dt, _p(self._gbuf(out)), out.ld, _p(x.t), x.ld, _p(dgate), x.N, x.H * x.W, x.C, st)
            ga, acca = self.grad_target(a)
            gb, accb = self.grad_target(b)
            L.call("ydl_gate_bwd", x.dt, _p(gate), _p(dgate), _p(ga), a.ld, acca, _p(gb), b.ld, accb, x.N, x.C, st)
            if x.need:
                self._scale_channels_bwd(x, out, gate, st)
        return self._record(out, bw)

    # ------------------------------------------------------------------ depth-wise, grouped and cross Conv + BN + act
    def _side_bn_act(self, fam, x: Var, m, act: int, out: Optional[Var], res: Optional[Var], res_mode: int) -> Var:
        """the body that ``dw_bn_act``, ``gconv_bn_act`` and ``xconv_bn_act`` share: out = act(bn(conv(x))) [+ res].  The convolution launch
        writes the BatchNorm partial rows of its own output, so train mode goes conv -> ydl_bn_finalize -> ydl_bn_act_fwd; the backward
        is ydl_bn_act_bwd, then the weight and the input gradient on the main stream.  ``fam`` says what differs between the families:
          who, kind             the method's name and the layer's, for messages
          Cout, k, s            output channels, taps and stride of the geometry (padding k // 2)
          size(x) -> Ho, Wo     the output's size
          weights() -> w, wt    the operands of the forward and of the input gradient
          refuse(gp)            None, or: false when the kernels do not take the geometry (ydl_last_error says why)
          stats(gp, npix)       bytes of the statistics workspace and the block height of its partial rows
          fwd(gp, x, w, y, ws, st), wgrad(gp, x, dy, gk, st), dgrad(gp, x, dy, wt, gx, acc, st)      the three launches
        ``gp`` is the ConvGeom of the layer by reference (the depth-wise kernels take their sizes as plain arguments instead)."""
        who, kind, Cout, k, s, size, weights, refuse, stats, fwd, wgrad, dgrad = fam
        x = self._flat(x)
        if res is not None:
            res = self._flat(res)
        if out is not None and not out.aligned():       # the BatchNorm kernels work on 8-channel groups: stage an odd slice
            return self.copy(self._side_bn_act(fam, x, m, act, None, res, res_mode), out)
        if x.C != m.c1:
            raise RuntimeError(f"{kind} input channel mismatch: got {x.C}, weight expects {m.c1}")
        Ho, Wo = size(x)
        y = self.new(x.N, Cout, Ho, Wo)
        out = self._out(who, (x.N, Cout, Ho, Wo), out)
        st = _stream()
        w, wt = weights()
        cf = m.coeffs(self.device)
        npix = x.N * Ho * Wo
        cp = round_up(Cout, 8)
        geom = L.ConvGeom(x.N, x.H, x.W, m.c1, Ho, Wo, Cout, k, s, k // 2, x.ld, y.ld, 0)
        gp = ctypes.byref(geom)
        if refuse is not None and not refuse(gp):
            raise RuntimeError(f"{who}: " + (L.lib().ydl_last_error() or b"?").decode())
        if self.train:
            nbytes, bm = stats(gp, npix)
            ws = self._ws(nbytes)
            fwd(gp, x, w, y, _p(ws), st)
            self._bn_coeffs(m, cf, Cout, st, (ws, (npix + bm - 1) // bm, bm, npix, 1))
        else:
            fwd(gp, x, w, y, None, st)
            self._bn_coeffs(m, cf, Cout, st)
        self._bn_apply(y, cf["scale"], cf["shift"], act, out, npix, cp, st, res, res_mode)
        if not self.record:
            return out
        if not self.train:
            raise RuntimeError("backward through eval-mode BatchNorm is not supported")
        self._keep.append(geom)         # the ctypes struct outlives the enqueue

        def bw():
            st2 = _stream()
            dy = self.new(x.N, Cout, Ho, Wo)
            self._bn_bwd_rows(m, y, cf, act, out, res, res_mode, dy, self._bn_grad_rows(m, cp), npix, Cout, cp, st2)
            gb_ = L.ConvGeom(x.N, x.H, x.W, m.c1, Ho, Wo, Cout, k, s, k // 2, x.ld, dy.ld, 0)     # the same geometry on dy's rows
            gpb = ctypes.byref(gb_)
            self._keep.append(gb_)
            if m.trainable()[0]:
                wgrad(gpb, x, dy, m.grad_dw(), st2)
                self._touch(m.conv.weight)
            if x.need:
                gx, acc = self.grad_target(x)
                dgrad(gpb, x, dy, wt, gx, acc, st2)
        return self._record(out, bw, uses=(x, res if res_mode in (L.RES_BEFORE_ACT, L.RES_AFTER_ACT) else None))

    def _geom_family(self, entry: str, arg: int):
        """refuse, stats, fwd, wgrad, dgrad of ``_side_bn_act`` for the kernels that take a ConvGeom and one more integer (``entry`` =
        "ydl_gconv" with the group count, "ydl_xconv" with the axis).  They use no atomics: the same launches serve throughput mode and
        deterministic mode."""
        lib = L.lib()

        def refuse(gp):
            return getattr(lib, entry + "_supported")(gp, arg, self.dt)

        def stats(gp, npix):
            return getattr(lib, entry + "_fwd_stats_ws_bytes")(gp, arg, self.dt), getattr(lib, entry + "_fwd_block_m")(gp, arg, self.dt)

        def fwd(gp, x, w, y, ws, st):
            L.call(entry + "_fwd", gp, arg, self.dt, _p(x.t), _p(w), _p(y.t), ws, st)

        def wgrad(gp, x, dy, gk, st):                        # gk: KRSC [Cout][taps][Cin / groups], the kernel's dw layout
            ws = self._ws(max(getattr(lib, entry + "_wgrad_ws_bytes")(gp, arg, self.dt), 16))
            L.call(entry + "_wgrad", gp, arg, self.dt, _p(x.t), _p(dy.t), _p(gk), _p(ws), st)

        def dgrad(gp, x, dy, wt, gx, acc, st):
            L.call(entry + "_dgrad", gp, arg, self.dt, _p(dy.t), _p(wt), _p(gx), acc, st)
        return refuse, stats, fwd, wgrad, dgrad

    def dw_bn_act(self, x: Var, m, s: int, act: int, out: Optional[Var] = None, res: Optional[Var] = None,
                  res_mode: int = L.RES_NONE) -> Var:
        """depth-wise Conv+BN+act: out = act(bn(dwconv(x))) [+ res], stride 1 or 2 — the Ghost blocks (models/common.py:67-70,
        253-279) and the ``dw_conv`` branch of DCNv3 (modules/dcnv3.py:89, :35-39).  The convolution launch writes the BatchNorm
        partial rows of its own output (ydl_dwconv2_fwd), so train mode goes conv -> ydl_bn_finalize -> ydl_bn_act_fwd with no
        statistics pass over y.  ``out`` may be a concat slice."""
        C, k, lib = m.c1, m.k, L.lib()

        def size(x):
            return _out_size(x.H, k, s, k // 2), _out_size(x.W, k, s, k // 2)

        def weights():
            wm = m.master_dw()                                  # f32 [C][k*k]: both directions read the master
            return wm, wm

        def stats(gp, npix):
            return lib.ydl_bn_stats_ws_bytes(npix, C), lib.ydl_bn_stats_block_m()

        def fwd(gp, x, w, y, ws, st):
            L.call("ydl_dwconv2_fwd", self.dt, _p(x.t), x.ld, _p(w), _p(y.t), y.ld, ws, x.N, x.H, x.W, C, k, s, st)

        def wgrad(gp, x, dy, gk, st):
            # k = 3 at stride 1 (DCNv3's dw_conv) stays on the stride-1 entry point and its vectorised kernel until
            # ydl_dwconv2_wgrad has been measured against it at those shapes; its last argument is the padding, 1 like s
            wg = "ydl_dwconv_wgrad" if (k == 3 and s == 1) else "ydl_dwconv2_wgrad"
            ws = self._ws(getattr(lib, wg + "_ws_bytes")(C, k))
            L.call(wg, self.dt, _p(x.t), x.ld, _p(dy.t), dy.ld, _p(gk), _p(ws), x.N, x.H, x.W, C, k, s, st)

        def dgrad(gp, x, dy, wt, gx, acc, st):
            L.call("ydl_dwconv2_dgrad", self.dt, _p(dy.t), dy.ld, _p(wt), _p(gx), x.ld, acc, x.N, x.H, x.W, C, k, s, st)
        fam = ("dw_bn_act", "depth-wise Conv", C, k, s, size, weights, None, stats, fwd, wgrad, dgrad)
        return self._side_bn_act(fam, x, m, act, out, res, res_mode)

    def gconv_bn_act(self, x: Var, m, act: int, out: Optional[Var] = None, res: Optional[Var] = None,
                     res_mode: int = L.RES_NONE) -> Var:
        """grouped Conv+BN+act, 1 < groups < channels: out = act(bn(gconv(x))) [+ res] — models/common.py:1451-1468 (SPPCSPC_group) and
        every Conv / Bottleneck / C3 / C2f with g > 1.  One ydl_gconv_fwd launch serves all groups and writes the BatchNorm partial rows
        of its output, so train mode goes conv -> ydl_bn_finalize -> ydl_bn_act_fwd.  The kernels use no atomics: the same launches
        serve throughput mode and deterministic mode.  ``out`` may be a concat slice."""
        fam = ("gconv_bn_act", "grouped Conv", m.c2, m.k, 1, lambda x: (x.H, x.W), lambda: m.gconv_weights(self))
        return self._side_bn_act(fam + self._geom_family("ydl_gconv", m.groups), x, m, act, out, res, res_mode)

    def xconv_bn_act(self, x: Var, m, act: int, out: Optional[Var] = None, res: Optional[Var] = None,
                     res_mode: int = L.RES_NONE) -> Var:
        """cross Conv+BN+act, a kernel of m.k taps along the axis m.axis with stride m.s along it: out = act(bn(xconv(x))) [+ res] — the
        two convolutions of CrossConv (models/common.py:147-158).  ydl_xconv_fwd writes the BatchNorm partial rows of its output, so
        train mode goes conv -> ydl_bn_finalize -> ydl_bn_act_fwd.  The kernels use no atomics: the same launches serve throughput
        mode and deterministic mode.  ``out`` may be a concat slice."""
        k, s, ax = m.k, m.s, m.axis

        def size(x):
            return (_out_size(x.H, k, s, k // 2) if ax == L.AXIS_H else x.H), (_out_size(x.W, k, s, k // 2) if ax == L.AXIS_W else x.W)
        # weights: [Cout][k][Cin] and [Cin][k][Cout], ydl_weight_prep with kk = k
        fam = ("xconv_bn_act", "cross Conv", m.c2, k, s, size, lambda: m.compute_weights(self))
        return self._side_bn_act(fam + self._geom_family("ydl_xconv", ax), x, m, act, out, res, res_mode)

    def group_softmax(self, x: Var, G: int, P: int) -> Var:
        """softmax over the P sampling points of each group (modules/dcnv3.py:122-123)"""
        x = self._flat(x)
        assert x.C == G * P
        out = self.new(x.N, x.C, x.H, x.W)
        L.call("ydl_group_softmax_fwd", self.dt, _p(x.t), x.ld, _p(out.t), out.ld, x.npix, G, P, _stream())

        def bw():
            if x.need:
                gx, acc = self.grad_target(x)
                L.call("ydl_group_softmax_bwd", self.dt, _p(out.t), out.ld, _p(self._gbuf(out)), out.ld, _p(gx), x.ld, acc,
                       x.npix, G, P, _stream())
        return self._record(out, bw)

    def _cast_grads(self, pairs, st) -> None:
        """the tail of a backward whose kernel forms f32 gradients: (v, its dense f32 gradient or None) -> ydl_cast_f32 into (or added
        to) d/dv in the compute dtype, for every v that wants one"""
        for v, g32 in pairs:
            if g32 is not None and v.need:
                gv, acc = self.grad_target(v)
                L.call("ydl_cast_f32", v.dt, _p(g32), g32.shape[-1], _p(gv), v.ld, v.npix, v.C, acc, st)

    def dcnv3(self, x: Var, offset: Var, mask: Var, k: int, s: int, pad: int, dil: int, G: int, Gc: int, scale: float) -> Var:
        """the deformable sampling op itself (ydl_dcnv3_fwd / _bwd; functions/dcnv3_func.py:19-61).  The op wants dense
        rows: channel counts that are not multiples of 8 (offset 18*G, mask 9*G) are packed first."""
        def dense(v: Var) -> torch.Tensor:
            v = self.materialize(v)
            if v.ld == v.C and v.parent is None:
                return v.t.permute(0, 2, 3, 1)
            buf = torch.empty((v.N, v.H, v.W, v.C), dtype=v.t.dtype, device=self.device)
            L.call("ydl_copy2d", v.dt, _p(v.t), v.ld, _p(buf), v.C, v.npix, v.C, 0, _stream())
            return buf
        xd, od, md = dense(x), dense(offset), dense(mask)
        N, H, W, C = xd.shape
        Ho, Wo = _out_size(H, k, s, pad, dil), _out_size(W, k, s, pad, dil)
        out = self.new(N, C, Ho, Wo)
        assert out.ld == C, "DCNv3: channels must be a multiple of 8"
        L.call("ydl_dcnv3_fwd", self.dt, _p(xd), _p(od), _p(md), _p(out.t), k, k, s, s, pad, pad, dil, dil, G, Gc,
               ctypes.c_float(scale), N, H, W, Ho, Wo, _stream())

        def bw():
            st2 = _stream()
            gin = zero_(torch.empty(xd.shape, dtype=torch.float32, device=self.device))
            goff = torch.empty(od.shape, dtype=torch.float32, device=self.device)
            gmsk = torch.empty(md.shape, dtype=torch.float32, device=self.device)
            L.call("ydl_dcnv3_bwd", self.dt, _p(xd), _p(od), _p(md), _p(self._gbuf(out)), _p(gin), _p(goff), _p(gmsk),
                   k, k, s, s, pad, pad, dil, dil, G, Gc, ctypes.c_float(scale), N, H, W, Ho, Wo, st2)
            self._cast_grads(((x, gin), (offset, goff), (mask, gmsk)), st2)
        return self._record(out, bw)

    def _conv_shift_fwd(self, gp, x: Var, w: torch.Tensor, out: Var, shift, st, act: int = L.ACT_NONE, res: Optional[Var] = None,
                        res_mode: int = L.RES_NONE) -> None:
        """out = act(conv(x, w) + b) [+ res]: the implicit-GEMM launch, then — unless ``shift`` is None — ydl_bn_act_fwd in place
        with scale 1; ``shift(device)`` = (ones, b), asked for after the convolution is enqueued (it may launch a copy)"""
        L.call("ydl_conv_fwd", gp, self.dt, _p(x.t), _p(w), _p(out.t), None, 0, st)
        if shift is not None:
            ones, bias = shift(self.device)
            self._bn_apply(out, ones, bias, act, out, out.npix, round_up(out.C, 8), st, res, res_mode)

    def _conv_bias_bwd(self, m, gp, x: Var, dy: Var, wt: torch.Tensor, st, bias: bool = True) -> None:
        """backward of out = conv(x, m.weight) + m.bias from dy = d out: the bias gradient (ydl_channel_sum), the weight gradient,
        and the input gradient added into d x"""
        if bias and m.bias is not None and m.bias.requires_grad:
            # a row block of a shared parameter reports it once, after its last writer
            self._channel_sum_grad(dy, m._grad_of(m.bias), m.bias if m.final else None, st)
        m.wgrad(self, gp, x, dy, st)
        if x.need:
            gx, acc = self.grad_target(x)
            L.call("ydl_conv_dgrad", gp, self.dt, _p(dy.t), _p(wt), _p(gx), acc, st)

    def conv_bias(self, x: Var, m, out: Optional[Var] = None, bias: bool = True) -> Var:
        """convolution + optional bias with no BatchNorm and no activation: ``nn.Conv2d`` (DCNv2's conv_offset_mask,
        models/common.py:1652-1659) and ``nn.Linear`` on the channel dimension of an NHWC tensor (modules/dcnv3.py:92-100), which is
        its 1x1 case.  ``m`` is a yolo_dual_amd.modules._GemmWeights holder: weight [out][taps][in] in KRSC order, ``bias`` [out] or
        None.  ``out`` may be an 8-aligned channel slice of a wider buffer (the Q | K | V blocks of Tape.mha).  Backward: bias
        gradient by ydl_channel_sum, weight and input gradient by the conv kernels.  ``bias`` False leaves ``m.bias`` and its gradient
        to the consumer (``bias_gelu``)."""
        x = self._flat(x)
        Cout, _taps, Cin = m._gemm_dims()
        k, s, p = m.k, m.s, m.p
        if x.C != Cin:
            raise RuntimeError(f"{m._wname} input channel mismatch: got {x.C}, weight expects {Cin}")
        Ho, Wo = _out_size(x.H, k, s, p), _out_size(x.W, k, s, p)
        w, wt = m.compute_weights(self)
        out = self._out("conv_bias", (x.N, Cout, Ho, Wo), out, aligned=True)
        geom =L.ConvGeom(x.N, x.H, x.W, Cin, Ho, Wo, Cout, k, s, p, x.ld, out.ld, 0)
        gp = ctypes.byref(geom)
        self._conv_shift_fwd(gp, x, w, out, m.bias_coeffs if (bias and m.bias is not None) else None, _stream())
        if self.record:
            if x.need:
                self._use(x)

            def bw():
                # consumers may have written channel slices of this buffer's gradient only (DCNv2: the offset and mask slices)
                if not (out.is_set() or any(c.gset for c in out.children)):
                    return
                self._conv_bias_bwd(m, gp, x, Var(self, self._gbuf(out), out.ld, False), wt, _stream(), bias)
                self._keep.append(geom)
            self.bw.append(bw)
        return out

    def _bias_grad(self, m, dy: Var, st) -> None:
        """bias gradient of a transposed convolution: ydl_channel_sum over dy, added into ``m.bias.grad``"""
        if m.bias is not None and m.bias.requires_grad:
            self._channel_sum_grad(dy, self._param_grad(m.bias, self.device), m.bias, st)

    def _channel_sum_grad(self, dy: Var, grad: torch.Tensor, param, st) -> None:
        """grad += the per-channel sums of dy (ydl_channel_sum); ``param``: the parameter to report as written, or None"""
        ws = self._ws(L.lib().ydl_channel_sum_ws_bytes(dy.C), keep=True)
        L.call("ydl_channel_sum", self.dt, _p(dy.t), dy.ld, _p(grad), _p(ws), dy.npix, dy.C, 1, st)
        self._touch(param)

    def conv_transpose(self, x: Var, m, out: Optional[Var] = None) -> Var:
        """``nn.ConvTranspose2d(c1, c2, k, 2, p, output_padding)`` in the forms that double the map (modules._TCONV_FORMS), with no new
        kernel: a transposed convolution is the input gradient of the MIRRORED convolution c2 -> c1 on the (2H, 2W) map, and
        ydl_conv_dgrad already evaluates that in sub-pixel form (one dense convolution per output-parity class).  ``m`` is a
        modules.ConvTranspose2d: its channels_last parameter [c1][c2][k][k] is the KRSC master [c1][k*k][c2] of the mirrored layer.
          forward          ydl_conv_dgrad(g, dy := x, wt, dx := y), then the bias by ydl_bn_act_fwd in place with scale 1
          bias gradient    ydl_channel_sum over dy
          weight gradient  the holder's wgrad with x := dy, dy := x
          input gradient   ydl_conv_fwd(g, x := dy, w, y := dx, accumulate)"""
        x = self._flat(x)
        c1, _taps, c2 = m._gemm_dims()
        if x.C != c1:
            raise RuntimeError(f"ConvTranspose2d input channel mismatch: got {x.C}, weight expects {c1}")
        w, wt = m.compute_weights(self)
        out = self._out("conv_transpose", (x.N, c2, 2 * x.H, 2 * x.W), out, aligned=True)
        geom = L.ConvGeom(x.N, out.H, out.W, c2, x.H, x.W, c1, m.k, 2, m.p, out.ld, x.ld, 0)
        gp = ctypes.byref(geom)
        st = _stream()
        L.call("ydl_conv_dgrad", gp, self.dt, _p(x.t), _p(wt), _p(out.t), 0, st)
        if m.bias is not None:
            ones, bias = m.bias_coeffs(self.device)
            self._bn_apply(out, ones, bias, L.ACT_NONE, out, out.npix, round_up(out.C, 8), st)

        def bw():
            st2 = _stream()
            dy = Var(self, self._gbuf(out), out.ld, False)
            self._bias_grad(m, dy, st2)
            m.wgrad(self, gp, dy, x, st2)
            if x.need:
                gx, acc = self.grad_target(x)
                L.call("ydl_conv_fwd", gp, self.dt, _p(dy.t), _p(w), _p(gx), None, acc, st2)
            self._keep.append(geom)
        return self._record(out, bw, uses=(x,))

    def dw_conv_transpose(self, x: Var, m, out: Optional[Var] = None) -> Var:
        """``DWConvTranspose2d`` (models/common.py:73-76), depth-wise at stride 2 in the forms that double the map: the kernels of
        csrc/tconv.hip read the f32 master [C][k*k] directly and fuse the bias; the weight gradient is deterministic (per-CTA
        partials merged in a fixed order), the bias gradient comes from ydl_channel_sum."""
        x = self._flat(x)
        C, k, p, op = m.in_channels, m.k, m.p, m.op
        if x.C != C:
            raise RuntimeError(f"DWConvTranspose2d input channel mismatch: got {x.C}, weight expects {C}")
        out = self._out("dw_conv_transpose", (x.N, C, 2 * x.H, 2 * x.W), out, aligned=True)
        wm = m.master_dw()
        st = _stream()
        L.call("ydl_dwtconv_fwd", self.dt, _p(x.t), x.ld, _p(wm), _p(m.bias.detach()) if m.bias is not None else None, _p(out.t), out.ld,
               x.N, x.H, x.W, C, k, p, op, st)

        def bw():
            st2 = _stream()
            dy = Var(self, self._gbuf(out), out.ld, False)
            self._bias_grad(m, dy, st2)
            if m.weight.requires_grad:
                gk = m.grad_dw()
                ws = self._ws(L.lib().ydl_dwtconv_wgrad_ws_bytes(C, k), keep=True)
                L.call("ydl_dwtconv_wgrad", self.dt, _p(x.t), x.ld, _p(dy.t), dy.ld, _p(gk), _p(ws), x.N, x.H, x.W, C, k, p, op, st2)
                self._touch(m.weight)
            if x.need:
                gx, acc = self.grad_target(x)
                L.call("ydl_dwtconv_dgrad", self.dt, _p(dy.t), dy.ld, _p(wm), _p(gx), x.ld, acc, x.N, x.H, x.W, C, k, p, op, st2)
        return self._record(out, bw, uses=(x,))

    def deform_conv(self, x: Var, offset: Var, mask: Optional[Var], m, gm, act: int, mask_sigmoid: bool = False,
                    out: Optional[Var] = None, res: Optional[Var] = None, res_mode: int = L.RES_NONE) -> Var:
        """act(bn(deform_conv2d(x, offset, m.weight, m.bias, mask))) (torchvision.ops.deform_conv2d followed by the block's
        BatchNorm): ydl_deform_gather writes the column buffer, the 1x1 GEMM over it is an ordinary ``conv_bn_act`` with the
        parameter holder ``gm`` (yolo_dual_amd.modules._DeformGemm: weight [Cout][kh*kw*Cin] = the KRSC weight, the bias as one more column), so the BN
        statistics, the deferred weight gradient and d col come from the existing conv path; the backward of the gather turns
        d col into the input, offset and mask gradients.  ``offset`` / ``mask`` are read with their own row strides (channel
        slices of one buffer are fine); ``mask_sigmoid``: ``mask`` holds logits and the kernels apply the sigmoid."""
        x = self._flat(x)
        offset = self.materialize(offset)
        mask = self.materialize(mask) if mask is not None else None
        kh, kw = m.kernel_size
        (sh, sw), (ph, pw), (dh, dw) = m.stride, m.padding, m.dilation
        K = kh * kw
        if x.C != m.in_channels:
            raise RuntimeError(f"DeformConv2d input channel mismatch: got {x.C}, weight expects {m.in_channels}")
        G = offset.C // (2 * K)
        if G < 1 or offset.C != 2 * G * K or x.C % G or (mask is not None and mask.C != G * K):
            raise RuntimeError(f"DeformConv2d: offset has {offset.C} channels (2*G*{K} expected), mask "
                               f"{mask.C if mask is not None else None}")
        Ho, Wo = _out_size(x.H, kh, sh, ph, dh), _out_size(x.W, kw, sw, pw, dw)
        if (offset.H, offset.W) != (Ho, Wo) or (mask is not None and (mask.H, mask.W) != (Ho, Wo)):
            raise RuntimeError("DeformConv2d: offset / mask resolution does not match the output")
        kc = gm.c1
        ld = round_up(kc, 8)
        buf = torch.empty((x.N, Ho, Wo, ld), dtype=self.tdt, device=self.device)
        need = x.need or offset.need or (mask is not None and mask.need)
        col = Var(self, buf.permute(0, 3, 1, 2)[:, :kc], ld, need)
        L.call("ydl_deform_gather", self.dt, _p(x.t), x.ld, _p(offset.t), offset.ld, _p(mask.t) if mask is not None else None,
               mask.ld if mask is not None else 0, int(mask_sigmoid), _p(col.t), ld, int(m.bias is not None),
               x.N, x.H, x.W, x.C, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, G, _stream())
        if self.record and need:
            self._keep.append(buf)      # the deferred weight gradient reads col on the side stream: alive until the streams join
            if x.need:
                self._use(x)

            def bw():
                if not col.is_set():
                    return
                st2 = _stream()
                npix = x.N * Ho * Wo
                gin = zero_(torch.empty((x.N, x.H, x.W, x.C), dtype=torch.float32, device=self.device)) if x.need else None
                goff = torch.empty((npix, 2 * G * K), dtype=torch.float32, device=self.device) if offset.need else None
                gmsk = (torch.empty((npix, G * K), dtype=torch.float32, device=self.device)
                        if mask is not None and mask.need else None)
                L.call("ydl_deform_bwd", self.dt, _p(x.t), x.ld, _p(offset.t), offset.ld, _p(mask.t) if mask is not None else None,
                       mask.ld if mask is not None else 0, int(mask_sigmoid), _p(self._gbuf(col)), ld, _p(gin), _p(goff), _p(gmsk),
                       x.N, x.H, x.W, x.C, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, G, st2)
                self._cast_grads(((x, gin), (offset, goff), (mask, gmsk)), st2)
            self.bw.append(bw)
        gm.mark_step(self)
        return self.conv_bn_act(col, gm, 1, 0, act, out=out, res=res, res_mode=res_mode)

    def dilated_conv(self, x: Var, m, gm, d: int, act: int, out: Optional[Var] = None, res: Optional[Var] = None,
                     res_mode: int = L.RES_NONE) -> Var:
        """k x k convolution with dilation ``d``, stride 1 and padding d*(k-1)/2, in column form like ``deform_conv``:
        ydl_dilated_cols copies the taps into col[pix][tap*Cin + c] (a channel slice of a wider buffer is read in place), and the 1x1
        GEMM over col is an ordinary ``conv_bn_act`` (``gm`` holds a BatchNorm: Conv + BN + act) or ``conv_bias`` (``gm.bn`` is None:
        a plain ``nn.Conv2d``, bias or not, no activation), so the statistics, the weight gradient and d col come from the existing
        conv path; ydl_dilated_cols_bwd gathers d col into d x (no atomics).  ``m`` is the ``nn.Conv2d`` that owns the weight
        [Cout, Cin, k, k] (KRSC storage: the 1x1 weight as it is); ``gm`` its _GemmWeights view [Cout][1][k*k*Cin]."""
        x = self.materialize(x)
        k = m.kernel_size[0]
        if x.C != m.in_channels:
            raise RuntimeError(f"dilated Conv2d input channel mismatch: got {x.C}, weight expects {m.in_channels}")
        kc = k * k * x.C
        ld = round_up(kc, 8)
        buf = torch.empty((x.N, x.H, x.W, ld), dtype=self.tdt, device=self.device)
        col = Var(self, buf.permute(0, 3, 1, 2)[:, :kc], ld, x.need)
        L.call("ydl_dilated_cols", self.dt, _p(x.t), x.ld, _p(col.t), ld, 0, x.N, x.H, x.W, x.C, k, d, _stream())
        if self.record and x.need:
            self._keep.append(buf)      # the deferred weight gradient reads col on the side stream: alive until the streams join
            self._use(x)

            def bw():
                if not col.is_set():
                    return
                gx, acc = self.grad_target(x)
                L.call("ydl_dilated_cols_bwd", self.dt, _p(self._gbuf(col)), ld, _p(gx), x.ld, acc, x.N, x.H, x.W, x.C, k, d, _stream())
            self.bw.append(bw)
        if getattr(gm, "bn", None) is None:
            if act != L.ACT_NONE or res is not None:
                raise NotImplementedError("dilated_conv: a convolution without BatchNorm takes no activation and no residual")
            return self.conv_bias(col, gm, out=out)
        gm.mark_step(self)
        return self.conv_bn_act(col, gm, 1, 0, act, out=out, res=res, res_mode=res_mode)

    def scale(self, x: Var, gate: torch.Tensor) -> Var:
        """out = x * gate[n, c] with a constant ``gate`` (f32 [N][C], e.g. RFB's ``scale``); backward d x += d out * gate"""
        x = self.materialize(x)
        out = self.scale_channels(x, gate)
        return self._record(out, lambda: self._scale_channels_bwd(x, out, gate, _stream())) if x.need else out

    def local_attention(self, x: Var, mod) -> Var:
        """AttentionConv / AttentionStem (models/common.py:1509-1627): the bias-free 1x1 projections Q, K, V^0..V^{m-1} of x as
        implicit-GEMM launches into channel blocks of ONE buffer, then the windowed softmax-and-sum (ydl_local_attn_fwd).  ``mod`` is
        a yolo_dual_amd.modules._LocalAttention: ``projections()`` = [query, key, value...] weight holders, ``rel()`` = (rel_h, rel_w)
        or None, ``table(tape)`` = the AttentionStem mixing table E (f32 [m][k*k], ydl_attn_stem_table_fwd) or None.  Backward: the
        gather-form kernels write dQ | dK | dV^m into one buffer of the same layout, d rel_* and the table's three gradients are
        deterministic reductions, and every projection gets its weight gradient and adds its input gradient."""
        x = self._flat(x)
        projs = mod.projections()
        C, ks, m = mod.out_channels, mod.kernel_size, len(projs) - 2
        Cin = mod.in_channels
        if x.C != Cin:
            raise RuntimeError(f"{type(mod).__name__} input channel mismatch: got {x.C}, weights expect {Cin}")
        N, H, W = x.N, x.H, x.W
        Cp = round_up(C, 8)
        st = _stream()
        qkv = self.new(N, len(projs) * Cp, H, W, zero=(Cp != C))
        geom = L.ConvGeom(N, H, W, Cin, H, W, C, 1, 1, 0, x.ld, qkv.ld, 0)
        gp = ctypes.byref(geom)
        blk = _blocks(qkv.t, len(projs), Cp)
        wts = []
        for i, pr in enumerate(projs):
            w, wt = pr.compute_weights(self)
            wts.append(wt)
            self._conv_shift_fwd(gp, x, w, Var(self, qkv.t[:, i * Cp:i * Cp + C], qkv.ld, False), None, st)
        rel = mod.rel()
        emb = mod.table(self)
        rh, rw = (_p(rel[0].detach()), _p(rel[1].detach())) if rel is not None else (None, None)
        out = self.new(N, C, H, W)
        lse = torch.empty((x.npix, Cp), dtype=torch.float32, device=self.device) if self.record else None
        L.call("ydl_local_attn_fwd", self.dt, blk[0], qkv.ld, blk[1], qkv.ld, blk[2], qkv.ld, Cp, m, rh, rw, _p(emb), _p(out.t), out.ld,
               _p(lse), N, H, W, C, ks, st)

        def bw():
            st2 = _stream()
            dqkv = self.new(N, len(projs) * Cp, H, W, need=False, zero=(Cp != C))
            dblk = _blocks(dqkv.t, len(projs), Cp)
            drh = drw = demb = ws = None
            want_rel = rel is not None and (rel[0].requires_grad or rel[1].requires_grad)
            want_tab = emb is not None and mod.table_trainable()
            if want_rel:
                drh, drw = self._param_grad(rel[0], self.device), self._param_grad(rel[1], self.device)
            if want_tab:
                demb = torch.empty_like(emb)
            if want_rel or want_tab:
                ws = self._ws(L.lib().ydl_local_attn_bwd_ws_bytes(C, ks, m))
            L.call("ydl_local_attn_bwd", self.dt, blk[0], qkv.ld, blk[1], qkv.ld, blk[2], qkv.ld, Cp, m, rh, rw, _p(emb),
                   _p(out.t), out.ld, _p(lse), _p(self._gbuf(out)), out.ld, dblk[0], dblk[1], dblk[2], dqkv.ld, Cp, 0,
                   _p(drh), _p(drw), _p(demb), _p(ws), N, H, W, C, ks, st2)
            if want_rel:
                self._touch(*rel)
            if want_tab:
                mod.table_backward(self, emb, demb, st2)
            for i, pr in enumerate(projs):
                self._conv_bias_bwd(pr, gp, x, Var(self, dqkv.t[:, i * Cp:i * Cp + C], dqkv.ld, False), wts[i], st2)
            self._keep.extend((geom, qkv, dqkv, ws, demb))
        return self._record(out, bw, uses=(x,))

    def mha(self, qkv: Var, heads: int) -> Var:
        """dense multi-head self-attention over the H*W positions of each sample (nn.MultiheadAttention's core, no mask, no
        dropout): ``qkv`` is ONE buffer of rows [pix][Q | K | V] whose three channel blocks were written by Tape.conv_bias; head h is
        channels [h*d, (h+1)*d) of a block, scale = d^-0.5.  ydl_mha_fwd keeps the f32 log-sum of every softmax row; the backward
        (ydl_mha_bwd, gather form, bitwise reproducible) writes dQ | dK | dV into the gradient of ``qkv`` in the same layout."""
        if qkv.parent is not None or qkv.lazy or qkv.virtual or qkv.C % 3:
            raise RuntimeError("mha: qkv must be a whole [pix][Q | K | V] buffer")
        C = qkv.C // 3
        d = C // heads
        if C % heads or d % 8 or not 8 <= d <= 128:
            raise NotImplementedError(f"mha: head dimension {C}/{heads} is not implemented (multiples of 8 between 8 and 128)")
        N, S = qkv.N, qkv.H * qkv.W
        scale = float(d) ** -0.5
        blk = _blocks(qkv.t, 3, C)
        out = self.new(N, C, qkv.H, qkv.W)
        lse = torch.empty(N * heads * S, dtype=torch.float32, device=self.device) if self.record else None
        L.call("ydl_mha_fwd", self.dt, blk[0], qkv.ld, blk[1], qkv.ld, blk[2], qkv.ld, _p(out.t), out.ld, _p(lse),
               N, S, heads, d, scale, _stream())
        if self.record and qkv.need:
            def bw():
                if not out.is_set():
                    return
                st2 = _stream()
                ws = self._ws(L.lib().ydl_mha_bwd_ws_bytes(N, S, heads), keep=True)
                g, acc = self.grad_target(qkv)
                dblk = _blocks(g, 3, C)
                L.call("ydl_mha_bwd", self.dt, blk[0], qkv.ld, blk[1], qkv.ld, blk[2], qkv.ld, _p(out.t), out.ld, _p(lse),
                       _p(self._gbuf(out)), out.ld, dblk[0], dblk[1], dblk[2], qkv.ld, acc, _p(ws), N, S, heads, d, scale, st2)
                self._keep.append(lse)
            self.bw.append(bw)
        return out

    def scale_channels(self, x: Var, gate: torch.Tensor) -> Var:
        x = self.materialize(x)
        out = self.new_like(x)
        L.call("ydl_scale_channels", x.dt, _p(x.t), x.ld, _p(gate), _p(out.t), out.ld, x.N, x.H * x.W, x.C, _stream())
        return out
