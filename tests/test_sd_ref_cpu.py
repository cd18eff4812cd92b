"""CPU: tests/sd_ref.py, the reference of the space-to-depth / depth-to-space kernel tests, against the layers it stands for: order 1 at
s = 2 is Focus's concat of the four pixel phases (models/common.py:249), order 0 is Contract's and Expand's reshape / permute
(:288-293, :302-307), the two maps invert each other, and they are each other's transpose (the backward)."""
import pytest
import torch

from tests.sd_ref import depth_to_space_ref, space_to_depth_ref


def _x(shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_order_1_is_the_concat_of_focus():
    x = _x((2, 3, 4, 6))
    want = torch.cat((x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]), 1)
    assert torch.equal(space_to_depth_ref(x, 2, 1), want)
    assert not torch.equal(space_to_depth_ref(x, 2, 0), want)


@pytest.mark.parametrize("s", [1, 2, 3])
def test_order_0_is_contract_and_expand(s):
    N, C, H, W = 2, 5, 2 * s, 3 * s
    x = _x((N, C, H, W), s)
    contract = x.reshape(N, C, H // s, s, W // s, s).permute(0, 3, 5, 1, 2, 4).reshape(N, C * s * s, H // s, W // s)
    assert torch.equal(space_to_depth_ref(x, s, 0), contract)
    y = _x((N, C * s * s, 2, 3), 10 + s)
    expand = y.reshape(N, s, s, C, 2, 3).permute(0, 3, 4, 1, 5, 2).reshape(N, C, 2 * s, 3 * s)
    assert torch.equal(depth_to_space_ref(y, s, 0), expand)
    assert torch.equal(space_to_depth_ref(x, s, 0), torch.nn.functional.pixel_unshuffle(x, s).reshape(N, C, s * s, H // s, W // s)
                       .transpose(1, 2).reshape(N, C * s * s, H // s, W // s))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("s", [2, 3])
def test_the_maps_invert_and_transpose_each_other(s, order):
    x = _x((2, 4, 2 * s, 3 * s), 3)
    y = space_to_depth_ref(x, s, order)
    assert torch.equal(depth_to_space_ref(y, s, order), x)
    g = _x(tuple(y.shape), 4)
    # <S x, g> = <x, S^T g> with S^T = depth_to_space: a permutation's transpose is its inverse
    assert float((y * g).sum()) == pytest.approx(float((x * depth_to_space_ref(g, s, order)).sum()), rel=1e-12)
