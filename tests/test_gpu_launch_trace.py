"""GPU: the sequence of entry-point calls of a training step — every name, every scalar argument, every geometry, every stream and
every cross-stream edge (tests/launch_trace.py) — equals the recorded one, tests/golden/launch_trace.json.gz.  A change that is meant
to leave what the GPU executes alone (a refactor of the tape) is checked exactly here; the numeric tests cover the data flow, which
the trace leaves out (buffer addresses are not compared).  The fixture is compared against only, never a second run of the code
under test; ``python -m tests.test_gpu_launch_trace`` records it, which is done on the commit BEFORE such a change.

Every case seeds its weights and inputs and traces the first full step (zero_grad, forward, loss, backward, optimizer step: it
holds the weight preparation and the cache fills) and the second one separately; ``eval`` cases trace one forward under no_grad."""
import gzip
import importlib
import json
import os

import pytest
import torch

from tests.launch_trace import launch_trace

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "launch_trace.json.gz")
# the yaml models of tests/test_builders_<name>_cpu.py and the side of their output for a 32 x 32 input
YAMLS = {"ghost": 4, "gconv": 8, "cross": 8, "act": 8, "up": 32, "dilated": 8, "spp": 8}
# further yaml models: case name -> (builder test, its variable, side of the output for a 32 x 32 input).  "dcn" is built with
# deformable=True; "acon" is the act yaml under nn.Mish() with an AconC and an FReLU Conv swapped in (tests/test_gpu_act_blocks.py)
VARIANTS = {"convnext": ("convnext", "YAML", 2), "attention": ("attention", "YAML", 16), "transformer": ("transformer", "YAML", 16),
            "sd": ("sd", "YAML", 32), "mnv3": ("se", "YAML_MNV3", 2), "effb0": ("se", "YAML_EFF", 2), "dcn": ("dcn", "YAML", 16),
            "acon": ("act", "YAML", 8)}
# case name -> bench.WORKLOADS
MODELS = {"YOLOv5Seg": "cfg2", "YOLOv8Seg": "cfg4", "YOLOv9Seg": "cfg5", "ResNet50Seg": "cfg3", "YOLOv9SegDCNv3": "cfg5dcn"}


def _yaml_model(name):
    """the yaml model of a case name, on the CPU"""
    import yolo_dual_amd as ydl
    mod, var, _side = VARIANTS.get(name, (name, "YAML", None))
    yaml = getattr(importlib.import_module(f"tests.test_builders_{mod}_cpu"), var)
    if name == "acon":
        from tests.test_gpu_act_blocks import _swap_in_acon_and_frelu
        m = ydl.SegYoloModel(dict(yaml, activation="nn.Mish()"))
        _swap_in_acon_and_frelu(m)
        return m
    m = ydl.SegYoloModel(yaml, deformable=(name == "dcn"))
    for sub in m.modules():                  # CNBlock, MBConv: under a recorder the keep draw of stochastic depth is refused
        if getattr(sub, "stochastic_depth_prob", 0.0):
            sub.stochastic_depth_prob = 0.0
    return m


def _yaml_setup(name, freeze=False):
    """model, optimizer, loss and two batches as tests/test_gpu_gconv_blocks.py::_setup builds them; ``freeze``: every parameter of
    the middle block (SPPCSPC_group / C3x) frozen"""
    import yolo_dual_amd as ydl
    torch.manual_seed(11)
    m = _yaml_model(name)
    side = VARIANTS[name][2] if name in VARIANTS else YAMLS[name]
    if freeze:
        for p in m.model[2].parameters():
            p.requires_grad_(False)
    m = m.cuda().train()
    opt = ydl.smart_optimizer(m, "SGD", lr=0.01, momentum=0.937, decay=5e-4)
    crit = ydl.SegmentationLoss(12, 0.0, torch.ones(12), "dice", sync=False)
    gen = torch.Generator("cuda").manual_seed(3)
    xs = [torch.rand(2, 3, 32, 32, device="cuda", generator=gen) for _ in range(2)]
    ts = [torch.randint(0, 12, (2, side, side), device="cuda", generator=gen) for _ in range(2)]
    return m, opt, crit, xs, ts


def _model_setup(name, n, size):
    """a model of bench.WORKLOADS with its config, swaps, loss and class weights, filled as tests/test_gpu_model.py fills it"""
    import bench
    import yolo_dual_amd as ydl
    from oracle.fill import fill_state_dict
    wl = bench.WORKLOADS[MODELS[name]]
    out = size
    if name == "ResNet50Seg":
        m, out = ydl.ResNet50Seg({"nc": 12}), 640           # its head resizes to 640 x 640 whatever the input
    else:
        m = getattr(ydl, wl["model"])(bench.load_cfg(wl["yaml"], wl["swap"]))
        m.img_size = [size, size]
    sd = m.state_dict()
    fill_state_dict(sd, 1234, bn_stats=False)
    m.load_state_dict(sd)
    m = m.cuda().train()
    opt = ydl.FlatSGDEMA(m, lr=0.01, momentum=0.937, weight_decay=5e-4)
    crit = ydl.SegmentationLoss(12, 0.0, torch.tensor(bench.CW, dtype=torch.float32) if wl["cw"] else None, wl["loss"], sync=False)
    gen = torch.Generator("cuda").manual_seed(3)
    xs = [torch.rand(n, 3, size, size, device="cuda", generator=gen) for _ in range(2)]
    ts = [torch.randint(0, 12, (n, out, out), device="cuda", generator=gen) for _ in range(2)]
    return m, opt, crit, xs, ts


# case id -> (setup, its arguments, compute dtype, config setters as {name: (value for the case, value to restore)}, eval only)
CASES = {}
for _n in YAMLS:
    CASES[f"{_n}-bf16"] = (_yaml_setup, (_n,), "bf16", {}, False)
    CASES[f"{_n}-f32"] = (_yaml_setup, (_n,), "f32", {}, False)
    CASES[f"{_n}-bf16-rows"] = (_yaml_setup, (_n,), "bf16", {"set_bn_sums": (False, True)}, False)
    CASES[f"{_n}-eval"] = (_yaml_setup, (_n,), "bf16", {}, True)
for _n in VARIANTS:
    CASES[f"{_n}-bf16"] = (_yaml_setup, (_n,), "bf16", {}, False)
    CASES[f"{_n}-f32"] = (_yaml_setup, (_n,), "f32", {}, False)
    CASES[f"{_n}-eval"] = (_yaml_setup, (_n,), "bf16", {}, True)
for _n in ("gconv", "cross"):
    CASES[f"{_n}-bf16-frozen"] = (_yaml_setup, (_n, True), "bf16", {}, False)
for _n in MODELS:
    CASES[f"{_n}-bf16"] = (_model_setup, (_n, 2, 64), "bf16", {}, False)
    CASES[f"{_n}-f32"] = (_model_setup, (_n, 2, 64), "f32", {}, False)
    CASES[f"{_n}-eval"] = (_model_setup, (_n, 2, 64), "bf16", {}, True)
CASES["YOLOv5Seg-bf16-bnfuse"] = (_model_setup, ("YOLOv5Seg", 2, 64), "bf16", {"set_bn_bwd_fuse": (True, False)}, False)
CASES["YOLOv5Seg-bf16-serial"] = (_model_setup, ("YOLOv5Seg", 2, 64), "bf16", {"set_overlap_wgrad": (False, True)}, False)
# 8 * 128 * 128 = 131072 pixels in the stride-4 128-channel layers: the smallest the one-pass 1x1 backward kernels take
CASES["YOLOv5Seg-bf16-512"] = (_model_setup, ("YOLOv5Seg", 8, 512), "bf16", {}, False)


def trace_case(cid):
    """{"step1": ops, "step2": ops} of a training case, {"forward": ops} of an eval case"""
    import yolo_dual_amd as ydl
    from yolo_dual_amd import config
    setup, args, mode, setters, eval_only = CASES[cid]
    ydl.set_compute_dtype(mode)
    try:
        for k, (on, _off) in setters.items():
            getattr(config, k)(on)
        m, opt, crit, xs, ts = setup(*args)
        if eval_only:
            m.eval()

            def forward():
                with torch.no_grad():
                    m(xs[0])
            res = {"forward": launch_trace(forward)}
        else:
            def step(i):
                opt.zero_grad()
                total, _items = crit(m(xs[i]), ts[i])
                total.backward()
                opt.step()
            res = {"step1": launch_trace(lambda: step(0)), "step2": launch_trace(lambda: step(1))}
        torch.cuda.synchronize()
        return res
    finally:
        for k, (_on, off) in setters.items():
            getattr(config, k)(off)
        ydl.set_compute_dtype("bf16")


_FIX = []


def _fixture():
    """{"ops": the distinct operations, "cases": {case id: {part: indices into ops}}}"""
    if not _FIX:
        with gzip.open(FIXTURE, "rt") as f:
            _FIX.append(json.load(f))
    return _FIX[0]


def _want(cid):
    fx = _fixture()
    return {part: [fx["ops"][i] for i in idx] for part, idx in fx["cases"][cid].items()}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_launch_trace_equals_the_fixture(cid):
    want = _want(cid)
    got = trace_case(cid)
    assert sorted(got) == sorted(want)
    for part in sorted(want):
        g, w = got[part], want[part]
        end = [["<end of the trace>"]]
        for i, (a, b) in enumerate(zip(g + end, w + end)):
            if a != b:
                print(f"[{cid} {part}] {len(g)} operations, fixture {len(w)}; first difference at operation {i}:\n"
                      f"  fixture {b}\n  got     {a}")
                break
        assert g == w, f"{cid} {part}: the launch trace differs from the fixture (first differing operation printed above)"


def _names(ops):
    return {op[0] for op in ops}


def test_fixture_holds_the_one_pass_pointwise_backward():
    """the 8 x 512 x 512 case exists for ydl_conv_bwd_pw_bn / ydl_conv_bwd_pw, which take 128 -> 128 1x1 layers of >= 131072 pixels"""
    w = _want("YOLOv5Seg-bf16-512")
    assert {"ydl_conv_bwd_pw_bn", "ydl_conv_bwd_pw", "ydl_bn_act_bwd_reduce_sums"} <= _names(w["step1"]) & _names(w["step2"])


def test_fixture_holds_every_family():
    from yolo_dual_amd import _lib as L
    fx = _fixture()
    assert sorted(fx["cases"]) == sorted(CASES)
    used = [fx["ops"][i] for i in sorted({i for parts in fx["cases"].values() for idx in parts.values() for i in idx})]
    names = _names(used)
    need = {"ydl_dwconv2_fwd", "ydl_dwconv_wgrad", "ydl_dwconv2_wgrad", "ydl_gconv_wgrad", "ydl_xconv_dgrad", "ydl_resize_fwd",
            "ydl_resize_bwd", "ydl_bn_act_fwd_p", "ydl_bn_finalize", "ydl_conv_dgrad_bnred", "ydl_ln_bwd", "ydl_bias_gelu_bwd",
            "ydl_scale_res_bwd", "ydl_se_excite_bwd", "ydl_se_scale_bwd", "ydl_local_attn_bwd", "ydl_mha_bwd", "ydl_deform_bwd",
            "ydl_dcnv3_bwd", "ydl_acon_bwd", "ydl_max2_bwd", "ydl_space_to_depth", "ydl_depth_to_space", "ydl_group_softmax_bwd"}
    assert need <= names, sorted(need - names)
    for entry in ("ydl_resize_fwd", "ydl_resize_bwd"):           # the commuted conv-over-concat: bilinear, second argument
        assert any(op[0] == entry and op[2] == L.RESIZE_BILINEAR for op in used), entry


def record(path=FIXTURE):
    index, cases = {}, {}
    for cid in sorted(CASES):
        parts = trace_case(cid)
        cases[cid] = {part: [index.setdefault(json.dumps(op), len(index)) for op in tr] for part, tr in parts.items()}
        print(f"[launch trace] {cid}: " + ", ".join(f"{part} {len(tr)}" for part, tr in parts.items()), flush=True)
    ops = [json.loads(s) for s in index]
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
        f.write(json.dumps({"ops": ops, "cases": cases}, separators=(",", ":")).encode())
    print(f"[launch trace] {len(cases)} cases, {len(ops)} distinct operations -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    import sys
    record(*sys.argv[1:2])
