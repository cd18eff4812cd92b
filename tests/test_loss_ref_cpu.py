"""The float64 reference of the prediction tail (tests/loss_ref.py) held to what the reference project's own loss classes and
evaluator produced (tests/golden/loss_*.npz, miou.npz) and to float64 autograd, on the CPU: tests/test_gpu_prediction_tail.py
judges the HIP kernels by these routines, so they must be right on their own.

The goldens were computed in float32.  Measured float32-vs-float64 gap of this reference over the nine loss fixtures (worst case):
loss items 1.4e-7 relative, glogits 7.6e-7 of the largest gradient element (loss_jaccard_w_ls, whose gradient also runs through the
input softmax; 2.0e-7 for the others) — the goldens against the float64 reference show the same items figure and 5.5e-7 for glogits.
The asserted bounds are 16 float32 unit roundoffs for the items (2^-20 = 9.5e-7) and 32 for the gradients (2^-19 = 1.9e-6): 7x and
2.5x the gap, and fifty times tighter than the 1e-4 of test_losses."""
import pytest
import torch

from tests import loss_ref as R
from tests.util import Golden, names, rel_err

ITEM_TOL = 2.0 ** -20
GRAD_TOL = 2.0 ** -19
assert ITEM_TOL < 1e-4 and GRAD_TOL < 1e-4


def _golden_loss(g, name, dtype):
    x = g.t("logits").to(dtype).requires_grad_(True)
    pred = x.softmax(1) if int(g.flat["softmax_in"]) else x
    cw = g.t("cw") if g.t("cw").numel() else None
    kind = "jaccard" if "jaccard" in name else "dice"
    total, ce, ov, _I, _P, _T = R.seg_loss_terms(pred, g.t("target"), cw, kind, float(g.flat["ls"]), 1e-6)
    (gx,) = torch.autograd.grad(total, x)
    return [float(total.detach()), float(ce.detach()), float(ov.detach())], gx


@pytest.mark.parametrize("name", names("loss_"))
def test_reference_reproduces_the_loss_goldens(name):
    g = Golden(name)
    items64, gx64 = _golden_loss(g, name, torch.float64)
    items32, gx32 = _golden_loss(g, name, torch.float32)
    gap_items = max(abs(a - b) / abs(b) for a, b in zip(items32, items64))
    gap_grad = rel_err(gx32, gx64)
    err_items = max(abs(a - float(b)) / abs(float(b)) for a, b in zip(items64, g.flat["items"]))
    err_grad = rel_err(g.t("glogits"), gx64)
    print(f"{name}: f32-vs-f64 gap items {gap_items:.2e} grad {gap_grad:.2e}; golden vs f64 items {err_items:.2e} grad {err_grad:.2e}")
    assert gap_items < ITEM_TOL and gap_grad < GRAD_TOL, (gap_items, gap_grad)      # the bounds have headroom over the gap
    assert err_items < ITEM_TOL, (name, items64, g.flat["items"])
    assert abs(items64[0] - float(g.flat["total"])) < ITEM_TOL * abs(items64[0])
    assert err_grad < GRAD_TOL, (name, err_grad)


def test_reference_wrappers_agree_with_the_terms():
    """seg_loss_ref / seg_loss_rep_ref are seg_loss_terms plus autograd: same numbers, dloss scales the gradient only, and the
    replicated gradient is the replica sum of the dense one"""
    gen = torch.Generator().manual_seed(11)
    low = (torch.rand(2, 5, 3, 4, generator=gen, dtype=torch.float64) * 16 - 8)
    rep = (2, 3)
    t = torch.randint(0, 5, (2, 6, 12), generator=gen)
    cw = torch.rand(5, generator=gen) * 24.5 + 0.5
    full = R.replicate(low, rep)
    assert full.shape == (2, 5, 6, 12) and torch.equal(full[:, :, 3, 7], low[:, :, 1, 2])
    a = R.seg_loss_ref(full, t, cw, "jaccard", 0.1, 1e-6)
    b = R.seg_loss_ref(full, t, cw, "jaccard", 0.1, 1e-6, dloss=0.7)
    c = R.seg_loss_rep_ref(low, t, rep, cw, "jaccard", 0.1, 1e-6, dloss=0.7)
    assert (a.total, a.ce, a.overlap) == (b.total, b.ce, b.overlap) == (c.total, c.ce, c.overlap)
    assert abs(a.total - (a.ce + 0.5 * a.overlap)) < 1e-14
    assert rel_err(b.dpred, 0.7 * a.dpred) < 1e-14
    x = low.clone().requires_grad_(True)
    total = R.seg_loss_terms(R.replicate(x, rep), t, cw, "jaccard", 0.1, 1e-6)[0]
    (gl,) = torch.autograd.grad(0.7 * total, x)
    assert rel_err(c.dpred, gl) < 1e-13
    # labels outside [0, C): no CE term, an all-zero one-hot row
    t2 = t.clone()
    t2[0, :2] = 255
    t2[1, 3] = -1
    r = R.seg_loss_ref(full, t2, cw, "dice", 0.0, 1e-6)
    assert float(r.T.sum()) == float(((t2 >= 0) & (t2 < 5)).sum())
    k = (t2 >= 0) & (t2 < 5)
    nlp = -torch.log_softmax(full, 1).gather(1, t2.clamp(0, 4).unsqueeze(1)).squeeze(1)
    w = cw.double()[t2.clamp(0, 4)]
    assert abs(r.ce - float((w * nlp)[k].sum() / w[k].sum())) < 1e-13


def test_label_resize_is_torch_nearest():
    t = torch.arange(2 * 7 * 9).view(2, 7, 9) % 12
    out = R.resize_labels(t, (20, 12))
    ih = torch.floor(torch.arange(20, dtype=torch.float32) * (torch.tensor(7.0) / 20)).long().clamp(max=6)
    iw = torch.floor(torch.arange(12, dtype=torch.float32) * (torch.tensor(9.0) / 12)).long().clamp(max=8)
    assert torch.equal(out, t[:, ih][:, :, iw])
    assert R.resize_labels(t, (7, 9)) is t


def test_confusion_reference_reproduces_the_golden():
    g = Golden("miou")
    pred_cls, target = g.t("pred"), g.t("target")
    scores = torch.nn.functional.one_hot(pred_cls, 12).permute(0, 3, 1, 2).float()
    cm = R.confusion_ref(scores, target, 12, 11)
    assert cm.dtype == torch.int64 and torch.equal(cm, g.t("matrix"))
    # first maximum wins on exact ties; ignore and out-of-range labels are dropped
    s = torch.tensor([[0.5, 2.0, 2.0, 1.0]]).view(1, 4, 1, 1).expand(1, 4, 1, 5).contiguous()
    t = torch.tensor([[[0, 1, 3, 7, -1]]])
    cm = R.confusion_ref(s, t, 4, 3)
    want = torch.zeros(4, 4, dtype=torch.int64)
    want[0, 1] = want[1, 1] = 1
    assert torch.equal(cm, want)


@pytest.mark.parametrize("rep", [(1, 1), (2, 3), (4, 4), (1, 4)])
@pytest.mark.parametrize("C", [1, 12, 17])
def test_softmax_backward_reference_is_the_autograd_of_softmax_and_replication(C, rep):
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand(2, C, 5, 7, generator=gen, dtype=torch.float64) * 16 - 8).requires_grad_(True)
    out = torch.softmax(x, 1).repeat_interleave(rep[0], 2).repeat_interleave(rep[1], 3)
    assert torch.equal(out.detach(), R.softmax_ref(x.detach(), rep))
    dp = torch.randn(out.shape, generator=gen, dtype=torch.float64)
    (gx,) = torch.autograd.grad(out, x, dp)
    got = R.softmax_bwd_ref(torch.softmax(x.detach(), 1), dp, rep)
    assert float((got - gx).abs().max()) <= 1e-14 * float(dp.abs().max()) * rep[0] * rep[1]
