"""GPU: ydl_dilated_cols / ydl_dilated_cols_bwd through the C ABI on caller-owned buffers, against tests/dilated_ref.py.
* forward: a copy, so the column buffer equals the reference BIT FOR BIT in f32 and bf16, the zero padding columns and the ones
  column included; columns past round_up(k*k*C + ones, 8) are left alone; x may be a channel slice (ldx > C);
* backward: f32 within 1e-6 of the float64 sum relative to the tensor's max (nine f32 terms), bf16 within 2^-8 (one bf16 rounding of
  the stored sum); accumulate=1 adds the same values to the previous contents; two runs are bit-identical;
* the same dilation through ydl_deform_gather with zero offsets gives the same column buffer bit for bit.
Shapes: the 16-byte path (C % 8 == 0), the element path (C = 12), more than one block, d = 1, and d >= H (every off-centre tap is
outside the image)."""
import numpy as np
import pytest
import torch

from tests.dilated_ref import dilated_cols, dilated_cols_bwd, round_up

pytestmark = pytest.mark.gpu

K = 3
#        N  H  W  C   d  ldx-C ones
CASES = [(2, 5, 7, 8, 1, 0, 0), (2, 9, 7, 16, 2, 0, 0), (1, 8, 8, 12, 3, 0, 0), (2, 6, 5, 40, 5, 0, 0), (1, 4, 4, 8, 6, 0, 0),
         (2, 9, 7, 16, 2, 8, 0), (1, 8, 8, 12, 3, 4, 0), (2, 9, 7, 16, 2, 0, 1), (1, 8, 8, 12, 3, 0, 1)]
IDS = [f"N{n}H{h}W{w}C{c}d{d}" + ("_slice" if s else "") + ("_ones" if o else "") for (n, h, w, c, d, s, o) in CASES]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
BWD_TOL = {"f32": 1e-6, "bf16": 2.0 ** -8}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _call(name, *args):
    from yolo_dual_amd import _lib as L
    L.call(name, *args)
    torch.cuda.synchronize()


def _dt(mode):
    from yolo_dual_amd import _lib as L
    return L.YDL_F32 if mode == "f32" else L.YDL_BF16


def _forward(mode, x, C, d, ones, extra=0):
    """x: [N, H, W, ldx] device tensor whose first C channels are the input -> col [npix, width + extra] (pre-filled with 7)"""
    from yolo_dual_amd.tape import _p, _stream
    N, H, W, ldx = x.shape
    width = round_up(K * K * C + ones, 8)
    col = torch.full((N * H * W, width + extra), 7.0, dtype=x.dtype, device="cuda")
    _call("ydl_dilated_cols", _dt(mode), _p(x), ldx, _p(col), width + extra, ones, N, H, W, C, K, d, _stream())
    return col


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_is_a_bit_exact_copy(case, mode):
    N, H, W, C, d, pad, ones = case
    tdt = DTYPES[mode]
    g = torch.Generator().manual_seed(11 + C + d)
    xw = torch.randn(N, H, W, C + pad, generator=g).to(tdt)
    want = torch.from_numpy(dilated_cols(xw[..., :C].double().numpy(), K, d, ones_col=bool(ones))).to(tdt)
    col = _forward(mode, xw.cuda(), C, d, ones, extra=8)
    width = want.shape[1]
    assert torch.equal(_bits(col[:, :width].cpu()), _bits(want))
    assert bool((col[:, width:] == 7).all())                     # past the padded row: not the kernel's to write


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("case", CASES[:7], ids=IDS[:7])
def test_backward_is_the_float64_gather_sum(case, mode):
    from yolo_dual_amd.tape import _p, _stream
    N, H, W, C, d, pad, _ones = case
    tdt = DTYPES[mode]
    g = torch.Generator().manual_seed(23 + C + d)
    ldc = round_up(K * K * C, 8)
    dcol = torch.randn(N * H * W, ldc, generator=g).to(tdt)
    prev = torch.randn(N, H, W, C + pad, generator=g).to(tdt)
    ref = dilated_cols_bwd(dcol.double().numpy(), (N, H, W, C), K, d)
    scale = float(np.abs(ref).max())
    dcol_d = dcol.cuda()

    def run(acc):
        dx = prev.clone().cuda()
        _call("ydl_dilated_cols_bwd", _dt(mode), _p(dcol_d), ldc, _p(dx), C + pad, acc, N, H, W, C, K, d, _stream())
        return dx.cpu()
    a, b = run(0), run(0)
    assert torch.equal(_bits(a), _bits(b))                       # no atomics: bitwise reproducible
    assert torch.equal(_bits(a[..., C:]), _bits(prev[..., C:]))  # the other channels of a wider buffer are untouched
    err = float(np.abs(a[..., :C].double().numpy() - ref).max()) / scale
    print(f"[dilated bwd {mode}] {case}: {err:.2e}")
    assert err < BWD_TOL[mode]
    acc = run(1)
    ref_acc = prev[..., :C].double().numpy() + ref
    err_acc = float(np.abs(acc[..., :C].double().numpy() - ref_acc).max()) / float(np.abs(ref_acc).max())
    assert err_acc < BWD_TOL[mode]
    if mode == "f32":                                            # previous contents plus exactly the values of the plain run
        assert torch.equal(_bits(acc[..., :C]), _bits(prev[..., :C] + a[..., :C]))
    assert torch.equal(_bits(acc[..., C:]), _bits(prev[..., C:]))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_zero_offset_deform_gather_writes_the_same_columns(mode):
    from yolo_dual_amd.tape import _p, _stream
    N, H, W, C, d = 2, 9, 7, 16, 2
    tdt = DTYPES[mode]
    x = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(5)).to(tdt).cuda()
    ldc = K * K * C
    col = _forward(mode, x, C, d, 0)
    off = torch.zeros(N * H * W, 2 * K * K, dtype=tdt, device="cuda")
    ref = torch.full((N * H * W, ldc), 7.0, dtype=tdt, device="cuda")
    _call("ydl_deform_gather", _dt(mode), _p(x), C, _p(off), 2 * K * K, None, 0, 0, _p(ref), ldc, 0,
          N, H, W, C, H, W, K, K, 1, 1, d, d, d, d, 1, _stream())
    assert torch.equal(_bits(col), _bits(ref))


def test_other_geometries_are_refused():
    from yolo_dual_amd import _lib as L
    from yolo_dual_amd.tape import _p, _stream
    x = torch.zeros(1, 4, 4, 8, device="cuda")
    col = torch.zeros(16, 208, device="cuda")
    for k, d, ldc in ((2, 1, 208), (3, 0, 208), (4, 2, 208), (3, 2, 64)):
        with pytest.raises(L.YdlError):
            L.call("ydl_dilated_cols", L.YDL_F32, _p(x), 8, _p(col), ldc, 0, 1, 4, 4, 8, k, d, _stream())
        with pytest.raises(L.YdlError):
            L.call("ydl_dilated_cols_bwd", L.YDL_F32, _p(col), ldc, _p(x), 8, 0, 1, 4, 4, 8, k, d, _stream())
    torch.cuda.synchronize()
