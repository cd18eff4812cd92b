"""CPU: the pieces of tests/block_harness.py that decide whether a block-family test passes -- the error measure, the key classes, the
zero-bias-gradient rule and the judging half of the two bf16 checkers -- on hand-made numbers."""
import numpy as np
import pytest
import torch

from tests.block_harness import judge_against_floor, judge_against_tol, kind, rel_max_err, worst_by_kind, zero_bias_scale


def test_error_is_relative_to_the_wanted_tensors_max():
    want = np.array([1.0, -4.0, 2.0], dtype=np.float32)
    got = torch.tensor([1.0, -4.0, 2.5])
    assert rel_max_err(got, want) == pytest.approx(0.5 / 4.0)
    assert rel_max_err(got.to(torch.bfloat16), want) == pytest.approx(0.5 / 4.0)         # the comparison itself runs in float64
    assert rel_max_err(torch.tensor([1.0, -4.0, 2.0]), want) == 0.0


def test_error_against_an_all_zero_tensor_is_absolute_and_a_scale_overrides():
    assert rel_max_err(torch.tensor([0.0, 3e-5]), np.zeros(2)) == pytest.approx(3e-5)
    assert rel_max_err(torch.tensor([1.0, 2.5]), np.array([1.0, 2.0]), scale=10.0) == pytest.approx(0.05)
    assert rel_max_err(torch.tensor([1.0, 2.5]), np.array([1.0, 2.0]), scale=0.0) == pytest.approx(0.5)


def test_key_classes():
    assert [kind(k) for k in ("out", "grad_x", "g.a.b", "rm.x", "rv.x")] == ["out", "grad", "grad", "run", "run"]


Z = {"g.cv.bn.bias": np.full(4, 1e-12), "g.cv.bn.weight": np.array([0.25, -1.0, 0.5, 0.1]), "g.cv.conv.weight": np.ones((4, 2, 1, 1))}


@pytest.mark.parametrize("rel", [1e-9, 1e-6])
def test_a_zero_bias_gradient_is_measured_against_the_weight_gradient(rel):
    assert zero_bias_scale(Z, "cv.bn.bias", rel) == 1.0
    got = torch.full((4,), 1e-12) + 2e-5
    assert rel_max_err(got, Z["g.cv.bn.bias"], zero_bias_scale(Z, "cv.bn.bias", rel)) == pytest.approx(2e-5)
    # only a BatchNorm bias, and only below the threshold: 1e-12 is not below 1e-13 of the weight gradient
    assert zero_bias_scale(Z, "cv.bn.weight", rel) is None and zero_bias_scale(Z, "cv.conv.weight", rel) is None
    assert zero_bias_scale(Z, "cv.bn.bias", 1e-13) is None


def test_the_two_thresholds_differ_between_them():
    z = dict(Z, **{"g.cv.bn.bias": np.full(4, 1e-8)})          # between 1e-9 and 1e-6 of the weight gradient
    assert zero_bias_scale(z, "cv.bn.bias", 1e-9) is None and zero_bias_scale(z, "cv.bn.bias", 1e-6) == 1.0


def test_without_the_rule_a_bias_gradient_is_measured_against_itself():
    assert zero_bias_scale(Z, "cv.bn.bias", None) is None
    got = torch.full((4,), 3e-12)
    assert rel_max_err(got, Z["g.cv.bn.bias"], zero_bias_scale(Z, "cv.bn.bias", None)) == pytest.approx(2.0)


TOL = {"out": 1e-2, "grad": 5e-2, "run": 1e-3}
ERRS = {"out": 9e-3, "grad_x": 4e-2, "g.cv.conv.weight": 1e-2, "rm.cv.bn.running_mean": 5e-4, "rv.cv.bn.running_var": 9e-4}


def test_the_tolerance_judge_accepts_below_and_rejects_at_or_above_each_kinds_bound():
    assert judge_against_tol(ERRS, TOL) == {}
    for key, planted in (("out", 1.1e-2), ("g.cv.conv.weight", 5e-2), ("rv.cv.bn.running_var", 2e-3), ("grad_x", float("nan"))):
        bad = judge_against_tol(dict(ERRS, **{key: planted}), TOL)
        assert list(bad) == [key] and (bad[key] == planted or planted != planted)
    assert judge_against_tol({"out": 9e-3, "grad_x": 1e-2}, {"out": 1e-2, "grad": 5e-2}) == {}        # a family without running statistics


def test_the_floor_judge_accepts_below_and_rejects_at_or_above_factor_times_the_floor():
    floor = {"out": 2e-3, "grad": 4e-3, "run": 1e-3}
    errs = {"out": 7.9e-3, "grad_x": 1.5e-2, "g.w": 4e-3, "rm.m": 3.9e-3}
    assert judge_against_floor(errs, floor, 4.0) == {}
    assert judge_against_floor(dict(errs, out=8.1e-3), floor, 4.0) == {"out": (8.1e-3, 8e-3)}
    assert judge_against_floor(dict(errs, **{"g.w": 1.6e-2}), floor, 4.0) == {"g.w": (1.6e-2, 1.6e-2)}
    assert list(judge_against_floor(dict(errs, **{"rm.m": float("nan")}), floor, 4.0)) == ["rm.m"]
    assert list(judge_against_floor(errs, floor, 2.0)) == ["out", "grad_x", "rm.m"]                  # the factor is the caller's
    with pytest.raises(KeyError):                                                                   # a kind the fixture records no floor for
        judge_against_floor(errs, {"out": 2e-3, "grad": 4e-3}, 4.0)


def test_worst_by_kind_names_the_tensor():
    assert worst_by_kind(ERRS) == {"out": (9e-3, "out"), "grad": (4e-2, "grad_x"), "run": (9e-4, "rv.cv.bn.running_var")}
    assert worst_by_kind({"out": 1e-3, "g.w": 2e-3}, ("out", "grad")) == {"out": (1e-3, "out"), "grad": (2e-3, "g.w")}
