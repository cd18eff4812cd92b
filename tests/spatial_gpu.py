"""What tests/test_gpu_spatial_exact.py and tests/test_gpu_spatial_f64.py share: buffers with sentinels on the GPU that mirror
tests/spatial_ref.Layout, and the call through the C ABI on torch's current stream."""
import ctypes

import numpy as np
import torch

from tests import spatial_ref as R

F32, F64 = np.float32, np.float64
PAD_IN = 77.0           # what the pad channels [C, Cp) of an input hold: exact in bf16, larger than every datum (it would win every max)


def lib():
    from yolo_dual_amd import _lib as L
    return L


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dt(dtype):
    """-> (C ABI dtype, torch dtype, bytes per element, elements per 16-byte chunk)"""
    L = lib()
    return (L.YDL_F32, torch.float32, 4, 4) if dtype == "f32" else (L.YDL_BF16, torch.bfloat16, 2, 8)


class Buf:
    """a Layout's buffer on the GPU.  ``values`` (rows x C, numbers exact in the storage type) fill the answer columns, ``pad`` the pad
    channels [C, Cw); without values everything is sentinel (an output)"""

    def __init__(self, lay, tdt=torch.float32, values=None, pad=PAD_IN, sent=R.SENT):
        self.lay, self.tdt, self.sent = lay, tdt, sent
        if tdt in (torch.float32, torch.bfloat16):
            host = lay.canvas(F32, sent) if values is None else lay.embed(values, F32, pad, sent)
            self.t = torch.from_numpy(host).to(tdt).cuda()
        else:
            npdt = {torch.uint8: np.uint8, torch.int32: np.int32}[tdt]
            host = lay.canvas(npdt, sent) if values is None else lay.embed(values, npdt, pad, sent)
            self.t = torch.from_numpy(host).cuda()
        self.p = ctypes.c_void_p(self.t.data_ptr() + lay.lead * self.t.element_size())

    def host(self):
        t = self.t.cpu()
        return t.float().numpy() if t.dtype == torch.bfloat16 else t.numpy()


def slice_layout(rows, C, dtype, wide, pad="free", Cw=None):
    """ld == Cp, or (wide) the tensor as a channel slice of a buffer two chunks wider, one chunk in: an offset of 16 bytes"""
    V = R.vec(dtype)
    Cp = R.rup(C, V)
    Cw = Cp if Cw is None else Cw
    return R.Layout(rows, Cp + 2 * V, C, Cw, pad, R.LEAD + V) if wide else R.Layout(rows, Cp, C, Cw, pad)


def call(name, *args):
    lib().call(name, *args)


def sync():
    torch.cuda.synchronize()


def report(what, res):
    error, floor, bound = res
    print(f"  {what}: gpu {error:.2e}  floor {floor:.2e}  bound {bound:.2e}" + (f"  ({error / bound:.2f} of the bound)" if bound > 0 else ""))


def check(what, fn, got, case):
    """the GPU answer and the float32 floor of the same expression must both pass the bound"""
    res = fn(got, case)
    report(what, res)
    error, floor, bound = res
    assert floor <= bound, (what, "the float32 evaluation of the reference misses its own bound", floor, bound)
    assert error <= bound, (what, error, bound)
    return res


def refused(name, args, outs, needle=None):
    """the call returns non-zero, ydl_last_error names the function, every output buffer is still all sentinel"""
    L = lib()
    rc = getattr(L.lib(), name)(*args)
    sync()
    msg = (L.lib().ydl_last_error() or b"").decode()
    assert rc != 0, (name, "was not refused")
    assert msg.startswith(name + ":"), (name, msg)
    if needle:
        assert needle in msg, (name, msg)
    for b in outs:
        assert bool((b.t.float() == float(b.sent)).all()), (name, "wrote although it refused")
