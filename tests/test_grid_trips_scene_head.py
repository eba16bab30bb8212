"""GPU tier: the backward kernel of the scene head past the first trip of its grid-stride loop, in the manner of
tests/test_grid_trips.py.  The kernel launches min(items, 8 x compute units) workgroups of four wave items each
and walks the rest in a loop; with ONE compute unit assumed (`NMSA_ASSUME_CUS`, read by the library at every
call) the cap is 8 workgroups.  At (2, 66, 7, 37, 45) there are 132 plane items, 47 gweight items and one gbias
item: 45 workgroup trips' worth, so every workgroup runs five or six trips and the three kinds of items meet
inside one workgroup.  The results must be the bits the device's own count gives, and the restatement's."""
import pytest
import torch

from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.testing import scene_head_ref as R

from _gpu_support import assume_cus  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
SHAPE = (2, 66, 7, 37, 45)
WAVES_PER_WORKGROUP, WORKGROUPS_PER_CU = 4, 8


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16, torch.float16), ids=str)
def test_backward_runs_several_trips_with_the_same_bits(assume_cus, dtype):
    B, C, H, W, K = SHAPE
    wave_items = B * C + -(-K * C // 64) + -(-K // 64)
    workgroup_items = -(-wave_items // WAVES_PER_WORKGROUP)
    assert workgroup_items == 45 and workgroup_items > 5 * WORKGROUPS_PER_CU
    gen = torch.Generator().manual_seed(77)
    x = torch.randn((B, C, H, W), generator=gen).to(dtype)
    weight = torch.randn((K, C), generator=gen) / C ** 0.5
    g = torch.randn((B, K), generator=gen).to(dtype)
    logits, pooled = R.forward(x, weight, None)
    want = R.backward(g, pooled, weight, x.shape, dtype)
    xd, wd, gd = x.to(DEV), weight.to(DEV), g.to(DEV)
    results = {}
    for cus in (None, 1, 3):
        n = assume_cus(cus)
        assert (workgroup_items > WORKGROUPS_PER_CU * n) == (cus is not None)       # more than one trip, or one
        _, pooled_d = ops.scene_head(xd, wd, None)
        results[cus] = ops.scene_head_backward(gd, pooled_d, wd, x.shape, dtype)
        torch.cuda.synchronize()
    for cus, got in results.items():
        for name, a, b in zip(('gx', 'gweight', 'gbias'), got, want):
            assert R.same_bits(a, b), (cus, name)
