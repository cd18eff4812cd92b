"""Launch census (tests/census.py): every distinct convolution and BatchNorm launch of one recorded bf16 training step of bench.py's
workloads — at the workload's own batch and size, i.e. at the pixel counts, tile counts and strides its dispatch really sees — is
replayed on its own through the C ABI and compared element by element with a float64 reference under derived bounds; the kernel the
stand-alone call runs must be, as a whole string, the one the step ran.  cfg2 (the benchmark) must be complete: a launch of the two
families without a checker is a failure naming the entry point.  A case already checked under an earlier workload is checked once.

Not covered: the f32 parity leg of cfg2 (partial-row statistics have their own contract tests in test_gpu_bn_statistics.py), cfg5dcn
(DCNv3 has its own tests), and ydl_conv_dgrad_bnred / ydl_bn_finalize, which no bf16 workload launches with the default switches (they
would be reported as failures if one did).

Measured on an MI355X (this module: 22 s for the four workloads; cfg2 115 distinct cases for 81 convolution + 66 BatchNorm launches,
cfg3 93 for 143 + 96, cfg4 114 for 80 + 58, cfg5 131 for 113 + 88).  What it found: igemm2w_kernel (weights in registers) took its
replica sums from the bf16-ROUNDED values it stores; on cfg3's N32 160x160x64 k3 layer one channel's sum was off by 5.07e-3
sqrt(sum of squares), above the project's 5e-3.  The kernel now reduces its f32 accumulators like the other forward kernels."""
import pytest
import torch

from tests import census as Z

pytestmark = pytest.mark.gpu

_CHECKED = {}          # case key -> (workload, result) of the first check


@pytest.mark.parametrize("workload", ["cfg2", "cfg3", "cfg4", "cfg5"])
def test_every_launch_of_the_step_against_float64(workload):
    import yolo_dual_amd as ydl
    try:
        cen = Z.record_step(workload)
    finally:
        ydl.set_compute_dtype("bf16")
    failures, rows = [], []
    represented = {"conv": 0, "bn": 0}
    for key, slot in cen.cases.items():
        case = slot["case"]
        fam = "conv" if case["entry"] in Z.CONV_ENTRIES else "bn"
        names = sorted(slot["kernels"])
        if len(names) != 1:
            failures.append(f"{case['entry']} {Z.describe(case)}: one argument list ran on several kernels inside the step: {names}")
        if key in _CHECKED:
            first, res = _CHECKED[key]
            note = f"(checked under {first})"
        else:
            note = ""
            try:
                res = Z.check_case(case)
            except Z.CensusFailure as e:
                res = dict(kernel="?", ratio=float("inf"), over=-1, detail=str(e))
            torch.cuda.synchronize()
            _CHECKED[key] = (workload, res)
        represented[fam] += slot["count"]
        if res["over"]:
            failures.append(f"{case['entry']} {Z.describe(case)} [{res['kernel']}]: {res['detail']}")
        if res["kernel"] != "?" and names and res["kernel"] != names[0]:
            failures.append(f"{case['entry']} {Z.describe(case)}: ran on {names[0]} inside the step, on {res['kernel']} alone")
        rows.append((case["entry"], Z.describe(case), names[0] if names else "", slot["count"], res["ratio"], note))
    print(f"\n== launch census, {workload}: {len(rows)} distinct cases; conv launches {cen.total['conv']}, BatchNorm launches {cen.total['bn']}")
    print("entry | geometry, strides, flags | kernel | launches | worst error / bound")
    for r in rows:
        print(f"{r[0]} | {r[1]} | {r[2]} | {r[3]} | {r[4]:.3f} {r[5]}")
    # every launch counted in the step is represented by exactly one checked case, and the step is not trivially small
    assert represented["conv"] == cen.total["conv"] and represented["bn"] == cen.total["bn"], (represented, dict(cen.total))
    entries = {slot["case"]["entry"] for slot in cen.cases.values()}
    assert {"ydl_conv_fwd_sums", "ydl_conv_dgrad", "ydl_bn_act_fwd_sums", "ydl_bn_act_bwd_sums"} <= entries, entries
    assert entries & {"ydl_conv_wgrad", "ydl_conv_bwd_pw"}, entries
    print(f"represented: conv {represented['conv']} of {cen.total['conv']}, BatchNorm {represented['bn']} of {cen.total['bn']}")
    assert not failures, f"{len(failures)} of {len(rows)} cases:\n" + "\n".join(failures)
