"""Flat-arena optimizers + EMA: the optimizer step of the hot path as ONE fused HIP kernel per parameter run.  ``FlatSGDEMA`` is
the scripts' SGD(nesterov); ``FlatAdamEMA`` / ``FlatAdamWEMA`` / ``FlatRMSPropEMA`` are the other names ``smart_optimizer`` takes.
All share the arenas, the slots, the EMA shadow and the run tables of ``FlatArenaOptimizer``.

Semantics restate ``smart_optimizer(model, 'SGD', lr, momentum, decay)`` (utils/torch_utils.py:318-346: three groups —
biases / BN weights without decay, other weights with decay; torch.optim.SGD(nesterov=True)) and ``ModelEMA``
(utils/torch_utils.py:404-428: every float entry of the state_dict, decay ``d = 0.9999 (1 - exp(-n/2000))``).

MI355X-first layout: parameters, gradients, momentum and the EMA shadow each live in one contiguous f32 arena
``[weights with decay | BN weights | biases | float buffers]``.  ``p.data`` / ``p.grad`` of every parameter are views
of the arenas (conv weights keep their KRSC physical layout), so
  * the wgrad / BN-backward kernels write gradients straight into the arena,
  * ``zero_grad`` is one memset, the step is one streaming kernel per run, and
  * data-parallel all-reduce works on a few large contiguous ranges (yolo_dual_amd.parallel).
Parameters whose gradient was not produced in the current step (the reference's dead head layers) are
skipped exactly like torch.optim.SGD skips ``grad is None``: no weight decay, no momentum update."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from . import config
from .tape import _p, _stream, zero_


def _is_bn(m: nn.Module) -> bool:
    return "Norm" in type(m).__name__ or isinstance(m, nn.modules.batchnorm._BatchNorm)


class FlatArenaOptimizer(torch.optim.Optimizer):
    """what every flat-arena optimizer shares: the arenas ``[weights with decay | BN weights | biases | float buffers]``, the slots,
    the EMA shadow, the device hyper-parameter vector with its pinned ring, and the cache of device run tables.  A rule adds its
    state arenas (``n_state`` of them, allocated once between the gradient arena and the EMA shadow), its param_groups, its
    checkpoint format and the hooks of the step driver"""

    def _init_arenas(self, model: nn.Module, n_state: int, ema: bool, ema_decay: float, ema_tau: float, ema_updates: int):
        """lay the model out in the arenas; returns (decay weights, BN weights, biases, device)"""
        g0, g1, g2 = [], [], []          # decay weights, BN weights, biases   (names kept for the arena order)
        seen = set()
        for mod in model.modules():
            for pname, p in mod.named_parameters(recurse=False):
                if id(p) in seen:
                    continue
                seen.add(id(p))
                if pname == "bias":
                    g2.append(p)
                elif pname == "weight" and _is_bn(mod):
                    g1.append(p)
                else:
                    g0.append(p)
        # float buffers, all running means first, then all running variances (module order inside each): sibling
        # convolutions keep adjacent statistics, which lets CSP blocks run cv1|cv2 as one fused conv
        named = [(k, b) for k, b in model.named_buffers() if b.dtype.is_floating_point]
        bufs = ([b for k, b in named if k.endswith("running_mean")] + [b for k, b in named if k.endswith("running_var")] +
                [b for k, b in named if not (k.endswith("running_mean") or k.endswith("running_var"))])
        self.model = model
        self._groups3 = (g0, g1, g2)
        self._bufs = bufs
        dev = next(model.parameters()).device
        sizes = [sum(p.numel() for p in g) for g in (g0, g1, g2)]
        self.n_params = sum(sizes)
        self.n_total = self.n_params + sum(b.numel() for b in bufs)
        self.params_arena = torch.empty(self.n_total, dtype=torch.float32, device=dev)
        self.grads_arena = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
        self._state_arenas = [torch.zeros(self.n_params, dtype=torch.float32, device=dev) for _ in range(n_state)]
        self.ema_arena = torch.empty(self.n_total, dtype=torch.float32, device=dev) if ema else None
        self._slots: List[Tuple[nn.Parameter, int, int, int]] = []      # (param, offset, numel, group)
        off = 0
        for gi, g in enumerate((g0, g1, g2)):
            for p in g:
                n = p.numel()
                self._rehome(p, off, n)
                self._slots.append((p, off, n, gi))
                off += n
        self._buf_slots = []
        for b in bufs:
            n = b.numel()
            view = self.params_arena[off:off + n].view(b.shape)
            view.copy_(b.data)
            b.data = view
            self._buf_slots.append((b, off, n))
            off += n
        if ema:
            self.ema_arena.copy_(self.params_arena)
        self.ema_decay, self.ema_tau, self.updates = ema_decay, ema_tau, ema_updates
        return g0, g1, g2, dev

    def _init_groups(self, g0, g1, g2, dev, defaults: dict, weight_decay: float) -> None:
        """torch.optim.Optimizer plumbing (lr schedulers read/write param_groups[*]['lr']); group order follows
        smart_optimizer: biases, decay weights, BN weights"""
        torch.optim.Optimizer.__init__(self, [{"params": g2 or [torch.nn.Parameter(torch.zeros(0, device=dev))]},
                                              {"params": g0, "weight_decay": weight_decay},
                                              {"params": g1, "weight_decay": 0.0}], defaults)
        config.bump_weight_epoch()

    # ------------------------------------------------------------------
    @staticmethod
    def _view(arena: torch.Tensor, off: int, n: int, shape) -> torch.Tensor:
        """``arena[off:off + n]`` in the logical ``shape``; conv weights are KRSC physical, OIHW logical"""
        flat = arena[off:off + n]
        if len(shape) == 4:
            O, I, kh, kw = shape
            return flat.view(O, kh, kw, I).permute(0, 3, 1, 2)
        return flat.view(shape)

    def _slot_of_ptr(self) -> Dict[int, Tuple[int, int]]:
        """data pointer of every parameter and float buffer -> (offset, numel) in the arenas"""
        return {t.data_ptr(): (off, n) for t, off, n, *_g in self._slots + self._buf_slots}

    def _rehome(self, p: nn.Parameter, off: int, n: int) -> None:
        view = self._view(self.params_arena, off, n, p.shape)
        view.copy_(p.data)
        p.data = view
        p.grad = self._view(self.grads_arena, off, n, p.shape)
        p._ydl_touched = False

    def reattach(self) -> None:
        """(re)bind ``p.grad`` to the arena (needed if foreign code set grads to None)"""
        for p, off, n, _g in self._slots:
            if p.grad is None or p.grad.data_ptr() != self.grads_arena.data_ptr() + 4 * off:
                p.grad = self._view(self.grads_arena, off, n, p.shape)

    def zero_grad(self, set_to_none: bool = False) -> None:   # grads stay attached to the arena
        zero_(self.grads_arena)
        self.reattach()
        for p, *_ in self._slots:
            p._ydl_touched = False

    def live_ranges(self) -> List[Tuple[int, int]]:
        """contiguous arena ranges [a, b) of parameters that received a gradient this step"""
        out: List[Tuple[int, int]] = []
        for p, off, n, _g in self._slots:
            if getattr(p, "_ydl_touched", False):
                if out and out[-1][1] == off:
                    out[-1] = (out[-1][0], off + n)
                else:
                    out.append((off, off + n))
        return out

    # ------------------------------------------------------------------ graph-capturable step
    def ensure_hyper(self) -> None:
        """create the device hyper-parameter vector and its pinned staging ring.  Callers that route allocations to a private pool
        (HIP-graph capture, launch-list recording) call this BEFORE they do: a persistent tensor must not land on an address the
        captured / recorded step uses as scratch"""
        if getattr(self, "_hyper_ring", None) is None:
            # ring of pinned staging buffers, each guarded by the event of its last H2D copy: the host never rewrites a
            # buffer whose copy may still be queued behind a graph replay (one reused buffer raced with the next step's write)
            self._hyper_ring = [(torch.zeros(self._HYPER_FLOATS, dtype=torch.float32).pin_memory(), torch.cuda.Event()) for _ in range(8)]
            self._hyper_slot = 0
            self._hyper_used = [False] * 8
            self._hyper_dev = torch.zeros(self._HYPER_FLOATS, dtype=torch.float32, device=self.params_arena.device)

    def ensure_runs_table(self) -> None:
        """device table of the CURRENT run structure (as the last backward left the touched flags), created now: call after the
        warm-up steps and before entering a private pool, next to ``ensure_hyper``"""
        sig = self._run_rows(self._runs(commit=False))
        if sig:
            self._runs_dev = self._runs_table(sig)

    def _runs_table(self, sig: tuple) -> tuple:
        """(signature, device table) for a run structure.  Tables are cached per signature and never freed: a recorded launch list or
        a captured graph holds the raw device pointer of the table it was recorded with, and a later eager step with another
        structure (a freeze change, a different touched set) must not hand that block back to the allocator"""
        cache = self.__dict__.setdefault("_runs_cache", {})
        tab = cache.get(sig)
        if tab is None:
            n_tot = self.n_total
            for row in sig:                             # rows index the arenas unchecked in the kernel: validate them here
                off, n = row[0], row[3]
                if off < 0 or n < 0 or off + n > n_tot:
                    raise RuntimeError(f"optimizer run table row ({off}, {n}) outside the arenas ({n_tot})")
            tab = (sig, torch.tensor(sig, dtype=torch.int64).to(self.params_arena.device))
            cache[sig] = tab
        return tab

    # ------------------------------------------------------------------ the step driver; a rule supplies the hooks below it
    def _ema_d(self, off: float) -> float:
        """advance the EMA counter; the decay of this step, or ``off`` without an EMA"""
        if self.ema_arena is None:
            return off
        self.updates += 1
        return self.ema_decay * (1.0 - math.exp(-self.updates / self.ema_tau))

    def _runs(self, commit: bool = False) -> List[List]:
        """maximal runs of consecutive slots with identical (touched, group, rule state) key; ``commit`` tells the rule that the
        touched parameters are being stepped with that state"""
        runs: List[List] = []
        for i, (p, off, n, gi) in enumerate(self._slots):
            touched = bool(getattr(p, "_ydl_touched", False))
            key = (touched, gi, self._run_state(i, p, touched))
            if runs and runs[-1][0] == key and runs[-1][2] == off:
                runs[-1][2] = off + n
            else:
                runs.append([key, off, off + n])
            if touched and commit:
                self._commit(p)
        return runs

    def _spans(self, runs):
        """(offset, length, group, rule state) of every launch of a step: the touched runs and, with an EMA, the untouched runs and
        the float buffers behind the parameters (group None: EMA only, gradients and state are not read)"""
        for (touched, gi, state), a, b in runs:
            if touched:
                yield a, b - a, gi, state
            elif self.ema_arena is not None:
                yield a, b - a, None, 0
        if self.ema_arena is not None and self.n_total > self.n_params:
            yield self.n_params, self.n_total - self.n_params, None, 0

    def _run_rows(self, runs) -> tuple:
        """rows {offset, n_decay, n_params, n_total, lr index, flags (bit 0 weight decay), rule columns} of the ``_multi`` entry"""
        cls = self._classes()
        return tuple((a, 0, 0, n) + (0,) * (self._ROW_COLS - 4) if gi is None else
                     (a, n if gi == 0 else 0, n, n, gi) + self._row_tail(gi, state, cls) for a, n, gi, state in self._spans(runs))

    def _ptrs(self, a: int = 0, live: bool = True) -> list:
        """the array arguments of a launch that starts at element ``a``; an EMA-only launch (``live`` false) gets the gradient and
        state arenas as they are: they end at ``n_params`` and are not read"""
        ea = self.ema_arena
        return [_p(self.params_arena[a:])] + [_p(t[a:] if live else t) for t in [self.grads_arena] + self._state_arenas] + \
            [_p(ea[a:]) if ea is not None else None]

    def _hyper(self, grad_scale: float, d: float) -> List[float]:
        """the head of the hyper vector (ydl.h): lr of {weights, BN weights, biases}, the rule's values, grad_scale and EMA decay in
        their places, in double precision"""
        lr_bias, lr_w, lr_bn = (float(g["lr"]) for g in self.param_groups)
        return self._hyper_vals([lr_w, lr_bn, lr_bias], float(self.param_groups[1]["weight_decay"]), grad_scale, d)

    def prepare_step(self, grad_scale: float = 1.0) -> None:
        """host half of a step: advance the EMA counter and the rule's counters, and push the hyper-parameters and the EMA decay to
        the device vector the captured kernels read (call OUTSIDE the graph, before replaying it; layout: ydl.h)"""
        d = self._ema_d(0.0)
        self._advance()
        vals = self._hyper(grad_scale, d)
        vals += self._class_vals(vals)
        self.ensure_hyper()
        i = self._hyper_slot
        self._hyper_slot = (i + 1) % len(self._hyper_ring)
        h, ev = self._hyper_ring[i]
        if self._hyper_used[i]:
            ev.synchronize()              # normally long complete (8 steps ago)
        h.copy_(torch.tensor(vals, dtype=torch.float64))         # one rounding, double -> f32
        self._hyper_dev.copy_(h, non_blocking=True)
        ev.record()
        self._hyper_used[i] = True

    @torch.no_grad()
    def step_device_hyper(self) -> None:
        """device half: the same kernels as ``step`` but reading hyper-parameters from ``_hyper_dev`` (capturable)"""
        st = _stream()
        use_ema = 1 if self.ema_arena is not None else 0
        hp = _p(self._hyper_dev)
        rows = self._run_rows(self._runs(commit=True))
        # one launch for all runs.  The table is a persistent device tensor keyed by the run structure (constant while the same
        # parameters stay live); inside a recording / capture pass a NEW table must not be allocated (private pool), so a miss
        # there takes the per-run launches below
        tab = getattr(self, "_runs_dev", None)
        if (tab is None or tab[0] != rows) and rows and L.recorder() is None and not torch.cuda.is_current_stream_capturing():
            tab = self._runs_table(rows)
            self._runs_dev = tab
        if tab is not None and tab[0] == rows:
            if rows:
                L.call(self._ENTRY + "_multi", *self._rule_args(), *self._ptrs(), _p(tab[1]), len(rows), max(r[3] for r in rows),
                       hp, use_ema, st)
        else:
            for row in rows:
                L.call(self._ENTRY + "_dev", *self._rule_args(), *self._ptrs(row[0], row[2] > 0), *row[1:4], hp,
                       *self._dev_args(row), use_ema, st)
        config.bump_weight_epoch()

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        d = self._ema_d(-1.0)
        self._advance()
        hv = self._hyper(grad_scale, d)
        st = _stream()
        for a, n, gi, state in self._spans(self._runs(commit=True)):
            L.call(self._ENTRY, *self._rule_args(), *self._ptrs(a, gi is not None), n if gi == 0 else 0, 0 if gi is None else n, n,
                   *self._host_args(gi, state, hv), st)
        config.bump_weight_epoch()
        return None

    # ------------------------------------------------------------------ what a rule supplies
    # _ENTRY (name of its host-scalar entry point; "_dev" / "_multi" are the other two), _ROW_COLS and _HYPER_FLOATS (widths of
    # its run-table row and hyper vector), the number of state arenas (``_init_arenas``), _run_state (third component of a run
    # key), _row_tail (columns of a row after the lr index), _hyper_vals (head of the hyper vector), _dev_args / _host_args (the
    # scalars of the per-run entry points between n_total | hyper_dev and use_ema | stream), and where it needs them:
    RULE = 0                 # the ``rule`` argument of the family's entry points; SGD has entry points of its own and none

    def _rule_args(self) -> tuple:
        return (self.RULE,) if self.RULE else ()

    def _advance(self) -> None:
        """counters that move once per step, before the runs are formed (``step`` and ``prepare_step``)"""

    def _commit(self, p: nn.Parameter) -> None:
        """``p`` is being stepped (``step`` and ``step_device_hyper``)"""

    def _classes(self) -> Dict[int, int]:
        return {}

    def _class_vals(self, vals: List[float]) -> List[float]:
        """what follows the head of the hyper vector"""
        return []

    def load_ema_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """restore the EMA shadow from a ``state_dict`` (smart_resume: ``ema.ema.load_state_dict(ckpt['ema']...)``)"""
        if self.ema_arena is None:
            raise RuntimeError("EMA disabled")
        cur = self.ema_state_dict()
        by_ptr = self._slot_of_ptr()
        for k, v in self.model.state_dict().items():
            slot = by_ptr.get(v.data_ptr())
            if slot is None or not v.dtype.is_floating_point or k not in sd or tuple(sd[k].shape) != tuple(cur[k].shape):
                continue
            off, n = slot
            src = sd[k].float().to(self.ema_arena.device)
            if v.dim() == 4:
                src = src.permute(0, 2, 3, 1).contiguous()
            self.ema_arena[off:off + n].copy_(src.reshape(-1))

    # ------------------------------------------------------------------ EMA access (ModelEMA.ema equivalent)
    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """state_dict of the EMA shadow (same keys as model.state_dict(); integer buffers are copied as is)."""
        if self.ema_arena is None:
            raise RuntimeError("EMA disabled")
        by_ptr = self._slot_of_ptr()
        out = {}
        for k, v in self.model.state_dict().items():
            slot = by_ptr.get(v.data_ptr())
            if slot is None or not v.dtype.is_floating_point:
                out[k] = v.clone()
            else:
                out[k] = self._view(self.ema_arena, *slot, v.shape).clone()
        return out


class FlatSGDEMA(FlatArenaOptimizer):
    _ENTRY, _ROW_COLS, _HYPER_FLOATS = "ydl_sgd_ema_step", 6, 7

    def __init__(self, model: nn.Module, lr: float = 0.01, momentum: float = 0.937, weight_decay: float = 5e-4,
                 ema: bool = True, ema_decay: float = 0.9999, ema_tau: float = 2000.0, ema_updates: int = 0):
        g0, g1, g2, dev = self._init_arenas(model, 1, ema, ema_decay, ema_tau, ema_updates)
        self.mom_arena = self._state_arenas[0]
        self._has_buf: Dict[int, bool] = {}
        self._init_groups(g0, g1, g2, dev, dict(lr=lr, momentum=momentum, nesterov=True, weight_decay=0.0), weight_decay)

    def _run_state(self, i: int, p: nn.Parameter, touched: bool) -> bool:
        """first step of this parameter: its momentum buffer is initialised with the gradient"""
        return touched and not self._has_buf.get(id(p), False)

    def _commit(self, p: nn.Parameter) -> None:
        self._has_buf[id(p)] = True

    def _row_tail(self, gi: int, first: bool, cls) -> tuple:
        return ((1 if gi == 0 else 0) | (2 if first else 0),)

    def _hyper_vals(self, lrs, wd, grad_scale, d) -> List[float]:
        return lrs + [float(self.param_groups[1]["momentum"]), wd, grad_scale, d]

    def _dev_args(self, row) -> tuple:
        """lr index, weight decay, first step"""
        return row[4], row[5] & 1, row[5] >> 1

    def _host_args(self, gi, first, hv) -> tuple:
        """lr of the decay and of the no-decay part, momentum, weight decay, grad_scale, first step, EMA decay"""
        if gi is None:
            return 0.0, 0.0, hv[3], 0.0, 1.0, 0, hv[6]
        return hv[gi], hv[gi], hv[3], hv[4] if gi == 0 else 0.0, hv[5], 1 if first else 0, hv[6]

    # ------------------------------------------------------------------ checkpoint state (seg_diceloss_yolov5.py:1204-1212)
    def state_dict(self):
        """what ``'optimizer': optimizer.state_dict()`` of a checkpoint holds here: hyper-parameters per group, the momentum
        arena, which parameters already own a momentum buffer, and the EMA update counter (plain tensors / numbers only, so
        the file loads with ``torch.load(..., weights_only=True)``)"""
        return {"format": "ydl-flat-sgd-ema-1",
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups],
                "momentum": self.mom_arena.detach().cpu().clone(),
                "has_momentum": torch.tensor([bool(self._has_buf.get(id(p), False)) for p, *_ in self._slots]),
                "updates": int(self.updates)}

    def load_state_dict(self, sd) -> None:
        if sd.get("format") != "ydl-flat-sgd-ema-1":
            raise ValueError("optimizer state was not written by yolo_dual_amd.FlatSGDEMA")
        if sd["momentum"].numel() != self.mom_arena.numel():
            raise ValueError("optimizer state belongs to a different model (arena size differs)")
        for g, gs in zip(self.param_groups, sd["param_groups"]):
            g.update(gs)
        self.mom_arena.copy_(sd["momentum"].to(self.mom_arena.device))
        for (p, *_), h in zip(self._slots, sd["has_momentum"].tolist()):
            self._has_buf[id(p)] = bool(h)
        self.updates = int(sd.get("updates", 0))


class _FlatAdaptiveEMA(FlatArenaOptimizer):
    """Adam / AdamW / RMSProp over the arenas: torch.optim's single-tensor update per element (csrc/optim.hip), two state arenas
    (``state1_arena``: exp_avg | momentum buffer, ``state2_arena``: exp_avg_sq | square_avg), a step count per slot.

    Like torch, a parameter without a gradient this step is skipped entirely (no decay, no state update, its step count ``t`` does not
    advance), so parameters can sit at different ``t``.  Everything torch derives from ``t`` in Python double precision — the bias
    corrections, ``lr / (1 - beta1^t)``, ``1 - lr*wd`` — is computed here in double and reaches the kernels rounded once to f32.
    Parameters with the same ``t`` form a bias-correction class; runs never span two classes."""
    FORMAT = ""
    _ENTRY, _ROW_COLS, _HYPER_FLOATS = "ydl_optim_ema_step", 8, L.OPT_HYPER_FLOATS

    def _init_adaptive(self, model, defaults: dict, weight_decay: float, ema, ema_decay, ema_tau, ema_updates) -> None:
        g0, g1, g2, dev = self._init_arenas(model, 2, ema, ema_decay, ema_tau, ema_updates)
        self.state1_arena, self.state2_arena = self._state_arenas
        self._steps: List[int] = [0] * len(self._slots)          # torch's state['step'] of every slot
        self._init_groups(g0, g1, g2, dev, defaults, weight_decay)

    # ------------------------------------------------------------------ per-step numbers (host, double precision)
    def _betas(self) -> Tuple[float, float, float]:
        """(beta1 | momentum, beta2 | alpha, eps) of the weights group"""
        g = self.param_groups[1]
        if self.RULE == L.OPT_RMSPROP:
            return float(g["momentum"]), float(g["alpha"]), float(g["eps"])
        return float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])

    def _corrections(self, t: int, lr: float) -> Tuple[float, float]:
        """(step_size, bc2_sqrt) of a parameter at step count ``t`` with learning rate ``lr``"""
        if self.RULE == L.OPT_RMSPROP:
            return lr, 1.0
        b1, b2, _eps = self._betas()
        return lr / (1.0 - b1 ** t), (1.0 - b2 ** t) ** 0.5

    def _advance(self) -> None:
        """step_t += 1 of every parameter that received a gradient"""
        for i, (p, *_r) in enumerate(self._slots):
            if getattr(p, "_ydl_touched", False):
                self._steps[i] += 1

    def _classes(self) -> Dict[int, int]:
        """step count -> bias-correction class, over the live parameters, in ascending order of the count: while the same set of
        parameters stays live every count advances together, so a recorded / captured class index keeps its meaning"""
        if self.RULE == L.OPT_RMSPROP:
            return {}
        ts = sorted({t for (p, *_r), t in zip(self._slots, self._steps) if getattr(p, "_ydl_touched", False)})
        return {t: c for c, t in enumerate(ts)}

    def _run_state(self, i: int, p: nn.Parameter, touched: bool) -> int:
        """the step count: runs never span two bias-correction classes"""
        return self._steps[i] if touched and self.RULE != L.OPT_RMSPROP else 0

    def _row_tail(self, gi: int, t: int, cls) -> tuple:
        return 1 if gi == 0 else 0, cls.get(t, 0), 0

    def _hyper_vals(self, lrs, wd, grad_scale, d) -> List[float]:
        b1, b2, eps = self._betas()
        return lrs + [b1, wd, grad_scale, d, b2, eps, 1.0 - b1, 1.0 - b2, 1.0 - lrs[0] * wd]

    def _class_vals(self, vals: List[float]) -> List[float]:
        """the bias corrections of every class, per lr index"""
        cls = self._classes()
        if len(cls) > L.OPT_MAX_CLASSES:
            raise RuntimeError(f"{len(cls)} distinct step counts among the live parameters: the device hyper vector holds "
                               f"{L.OPT_MAX_CLASSES} bias-correction classes (use step(), which has no such limit)")
        tail = [0.0] * (self._HYPER_FLOATS - len(vals))
        for t, c in cls.items():
            for i in range(3):
                tail[4 * c + i], tail[4 * c + 3] = self._corrections(t, vals[i])
        return tail

    def _dev_args(self, row) -> tuple:
        """lr index, bias-correction class, weight decay"""
        return row[4], row[6], row[5] & 1

    def _host_args(self, gi, t, hv) -> tuple:
        """step_size, bc2_sqrt, decay_mul, weight decay, beta1, beta2, 1 - beta1, 1 - beta2, eps, grad_scale, EMA decay"""
        if gi is None:
            return 0.0, 1.0, 1.0, 0.0, hv[3], hv[7], hv[9], hv[10], hv[8], 1.0, hv[6]
        return (*self._corrections(t, hv[gi]), hv[11], hv[4] if gi == 0 else 0.0, hv[3], hv[7], hv[9], hv[10], hv[8], hv[5], hv[6])

    # ------------------------------------------------------------------ checkpoint state
    def state_dict(self):
        """hyper-parameters per group, both state arenas, the step count of every slot and the EMA update counter (plain tensors /
        numbers only, so the file loads with ``torch.load(..., weights_only=True)``); ``format`` names the rule"""
        return {"format": self.FORMAT,
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups],
                "state1": self.state1_arena.detach().cpu().clone(),
                "state2": self.state2_arena.detach().cpu().clone(),
                "steps": torch.tensor(self._steps, dtype=torch.int64),
                "updates": int(self.updates)}

    def load_state_dict(self, sd) -> None:
        if sd.get("format") != self.FORMAT:
            raise ValueError(f"optimizer state was not written by yolo_dual_amd.{type(self).__name__} "
                             f"(format {sd.get('format')!r}, expected {self.FORMAT!r})")
        if (sd["state1"].numel() != self.state1_arena.numel() or sd["state2"].numel() != self.state2_arena.numel()
                or sd["steps"].numel() != len(self._slots)):
            raise ValueError("optimizer state belongs to a different model (arena size or slot count differs)")
        for g, gs in zip(self.param_groups, sd["param_groups"]):
            g.update(gs)
            if "betas" in g:
                g["betas"] = tuple(g["betas"])
        self.state1_arena.copy_(sd["state1"].to(self.state1_arena.device))
        self.state2_arena.copy_(sd["state2"].to(self.state2_arena.device))
        self._steps = [int(t) for t in sd["steps"].tolist()]
        self.updates = int(sd.get("updates", 0))


class FlatAdamEMA(_FlatAdaptiveEMA):
    """torch.optim.Adam(betas=(momentum, 0.999)) — weight decay coupled (added to the gradient), on the weights group only"""
    RULE, FORMAT = L.OPT_ADAM, "ydl-flat-adam-ema-1"

    def __init__(self, model: nn.Module, lr: float = 0.001, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, ema: bool = True, ema_decay: float = 0.9999, ema_tau: float = 2000.0, ema_updates: int = 0):
        self._init_adaptive(model, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0.0, amsgrad=False, maximize=False),
                            weight_decay, ema, ema_decay, ema_tau, ema_updates)


class FlatAdamWEMA(_FlatAdaptiveEMA):
    """torch.optim.AdamW(betas=(momentum, 0.999)) — weight decay decoupled (``p *= 1 - lr*wd``), on the weights group only"""
    RULE, FORMAT = L.OPT_ADAMW, "ydl-flat-adamw-ema-1"

    def __init__(self, model: nn.Module, lr: float = 0.001, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, ema: bool = True, ema_decay: float = 0.9999, ema_tau: float = 2000.0, ema_updates: int = 0):
        self._init_adaptive(model, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0.0, amsgrad=False, maximize=False),
                            weight_decay, ema, ema_decay, ema_tau, ema_updates)


class FlatRMSPropEMA(_FlatAdaptiveEMA):
    """torch.optim.RMSprop(momentum=momentum) — alpha 0.99, not centered; weight decay coupled, on the weights group only"""
    RULE, FORMAT = L.OPT_RMSPROP, "ydl-flat-rmsprop-ema-1"

    def __init__(self, model: nn.Module, lr: float = 0.01, alpha: float = 0.99, eps: float = 1e-8, momentum: float = 0.0,
                 weight_decay: float = 0.0, ema: bool = True, ema_decay: float = 0.9999, ema_tau: float = 2000.0, ema_updates: int = 0):
        self._init_adaptive(model, dict(lr=lr, alpha=alpha, eps=eps, momentum=momentum, centered=False, weight_decay=0.0, maximize=False),
                            weight_decay, ema, ema_decay, ema_tau, ema_updates)


def smart_optimizer(model: nn.Module, name: str = "SGD", lr: float = 0.001, momentum: float = 0.9,
                    decay: float = 1e-5, ema: bool = True) -> FlatArenaOptimizer:
    """utils/torch_utils.py:318-346 signature and names: Adam / AdamW take ``betas=(momentum, 0.999)``, RMSProp and SGD take
    ``momentum``, SGD is nesterov; every name runs the fused HIP step."""
    if name == "Adam":
        return FlatAdamEMA(model, lr=lr, betas=(momentum, 0.999), weight_decay=decay, ema=ema)
    if name == "AdamW":
        return FlatAdamWEMA(model, lr=lr, betas=(momentum, 0.999), weight_decay=decay, ema=ema)
    if name == "RMSProp":
        return FlatRMSPropEMA(model, lr=lr, momentum=momentum, weight_decay=decay, ema=ema)
    if name == "SGD":
        return FlatSGDEMA(model, lr=lr, momentum=momentum, weight_decay=decay, ema=ema)
    raise NotImplementedError(f'Optimizer {name} not implemented.')
