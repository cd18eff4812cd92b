"""Plain float64 reference of the prediction tail (csrc/loss.hip): channel softmax with nearest replication and its backward, the
CE + 0.5 * (Dice | Jaccard) segmentation loss with its gradient, and the argmax confusion matrix.  torch on the CPU, whole-tensor
expressions, gradients by autograd; pinned by tests/test_loss_ref_cpu.py and used by tests/test_gpu_prediction_tail.py.

Every function takes an optional ``dtype``: float64 is the reference, float32 evaluates the same expressions in the kernels' own
precision and gives the float32-vs-float64 floor that the GPU bounds are cross-checked against."""
from collections import namedtuple

import torch
import torch.nn.functional as F

LossRef = namedtuple("LossRef", "total ce overlap dpred I P T")


def replicate(x, rep):
    """nearest up-sampling by whole factors: (N, C, H, W) -> (N, C, H*rh, W*rw)"""
    return x.repeat_interleave(rep[0], 2).repeat_interleave(rep[1], 3)


def replica_sum(g, rep):
    """adjoint of ``replicate``: (N, C, H*rh, W*rw) -> (N, C, H, W)"""
    N, C, LH, LW = g.shape
    return g.reshape(N, C, LH // rep[0], rep[0], LW // rep[1], rep[1]).sum((3, 5))


def softmax_ref(x, rep=(1, 1)):
    """x: (N, C, H, W) logits -> softmax over C, replicated to (N, C, H*rh, W*rw)"""
    return replicate(torch.softmax(x, 1), rep)


def softmax_bwd_ref(p, dp, rep=(1, 1)):
    """p: (N, C, H, W) stored probabilities, dp: gradient of the replicated output -> gradient of the logits"""
    g = replica_sum(dp, rep)
    return p * (g - (p * g).sum(1, keepdim=True))


def resize_labels(target, hw):
    """F.interpolate(mode='nearest') of the label map, as oracle/ref_cpu.py::seg_loss does it"""
    if tuple(target.shape[1:]) == tuple(hw):
        return target
    return F.interpolate(target.unsqueeze(1).float(), size=tuple(hw), mode="nearest").squeeze(1).long()


def seg_loss_terms(pred, target, cw=None, kind="dice", ls=0.0, eps=1e-6, target_hw=None):
    """differentiable (total, ce, overlap, I, P, T) of ``pred`` (N, C, H, W), any float dtype.  Labels outside [0, C) have no class:
    CE ignores them (ignore_index) and their one-hot row is all zero."""
    N, C, H, W = pred.shape
    t = resize_labels(target, target_hw if target_hw is not None else (H, W))
    assert tuple(t.shape[1:]) == (H, W)
    known = (t >= 0) & (t < C)
    w = None if cw is None else cw.to(pred.dtype)
    ce = F.cross_entropy(torch.log_softmax(pred, 1), torch.where(known, t, torch.full_like(t, -100)), weight=w,
                         ignore_index=-100, label_smoothing=ls)
    p = torch.softmax(pred, 1)
    onehot = (t.unsqueeze(1) == torch.arange(C).view(1, C, 1, 1)).to(pred.dtype)
    if w is not None:
        p = p * w.view(1, C, 1, 1)
    I, P, T = (p * onehot).sum((2, 3)), p.sum((2, 3)), onehot.sum((2, 3))
    if kind == "dice":
        R = (2.0 * I + eps) / (P + T + eps)
    elif kind == "jaccard":
        R = (I + eps) / (P + T - I + eps)
    else:
        raise ValueError(kind)
    overlap = 1.0 - R.mean()
    return ce + 0.5 * overlap, ce, overlap, I, P, T


def seg_loss_ref(pred, target, cw=None, kind="dice", ls=0.0, eps=1e-6, target_hw=None, dloss=1.0, dtype=torch.float64):
    """-> LossRef: the three loss items as python floats, d(dloss * total)/d pred by autograd, and the (N, C) sums I, P, T"""
    x = pred.detach().to(dtype).requires_grad_(True)
    total, ce, ov, I, P, T = seg_loss_terms(x, target, cw, kind, ls, eps, target_hw)
    (dpred,) = torch.autograd.grad(total * dloss, x)
    return LossRef(float(total.detach()), float(ce.detach()), float(ov.detach()), dpred, I.detach(), P.detach(), T.detach())


def seg_loss_rep_ref(low, target, rep, cw=None, kind="dice", ls=0.0, eps=1e-6, dloss=1.0, dtype=torch.float64):
    """the loss of the materialised nearest replication of ``low`` (N, C, h, w) against full-size labels; ``dpred`` is the
    full-resolution gradient summed over each stored pixel's replicas"""
    r = seg_loss_ref(replicate(low.detach().to(dtype), rep), target, cw, kind, ls, eps, None, dloss, dtype)
    return r._replace(dpred=replica_sum(r.dpred, rep))


def confusion_ref(pred, target, C, ignore):
    """rows = label, columns = argmax of ``pred`` (N, C, H, W) (first maximum wins); labels outside [0, C) and labels equal to
    ``ignore`` are dropped.  int64 (C, C)."""
    cls = torch.argmax(pred, 1).flatten().to(torch.int64)
    t = target.flatten().to(torch.int64)
    keep = (t >= 0) & (t < C) & (t != ignore)
    return torch.bincount(C * t[keep] + cls[keep], minlength=C * C).view(C, C)
