"""GPU tier: the stem max pool on a tensor of more than 2^31 elements.  Offsets inside a plane are 32-bit, the plane
base is 64-bit (csrc/maxpool.hip): 2049 planes of 1024 x 1024 put the last plane's base at 2^31 elements, where
a 32-bit base would wrap onto plane 0.  y is held to `F.max_pool2d` on the same device tensor, bit for bit; the
code and gx of the last plane (and of the one before the boundary) to testing/maxpool_ref.py on the CPU."""
import pytest
import torch
import torch.nn.functional as F

from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.testing import maxpool_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
PLANES, H, W = 2049, 1024, 1024


def test_planes_behind_two_to_the_31_elements():
    assert (PLANES - 1) * H * W == 2 ** 31
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.empty((1, PLANES, H, W), dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
    y, code = ops.maxpool3x3s2(x)
    assert R.same_bits(y, F.max_pool2d(x, 3, 2, 1))
    gy = torch.empty(y.shape, dtype=torch.bfloat16, device=DEV).normal_(generator=gen)
    gx = ops.maxpool3x3s2_backward(gy, code, (H, W))
    for plane in (PLANES - 1, PLANES - 2, 0):
        xs = x[:, plane:plane + 1].cpu()
        want_y, want_code = R.forward(xs)
        assert torch.equal(code[:, plane:plane + 1].cpu(), want_code), plane
        assert R.same_bits(y[:, plane:plane + 1].cpu(), want_y), plane
        want_gx = R.backward_f32(gy[:, plane:plane + 1].cpu(), want_code, H, W).to(torch.bfloat16)
        assert R.same_bits(gx[:, plane:plane + 1].cpu(), want_gx), plane
