"""GPU tier: the two kernels of csrc/maxpool.hip past the first trip of their grid-stride loops, in the manner of
tests/test_grid_trips_block.py.

Both kernels launch min(items, MP_BLOCKS_PER_CU = 8 workgroups per compute unit) workgroups of 256 lanes and walk
the rest in a loop; an item is 256 consecutive lane units (a unit: a row tile of 8 output rows x one lane group
of one plane, planes numbered first), so an item crosses planes and tiles.  `NMSA_ASSUME_CUS` (read by the
library at every call) shrinks the cap: every kernel runs under assumed counts of 1, 3 and the device's own.
Held: the results are bit-identical across the three counts and equal to testing/maxpool_ref.py.

Items (B = 2, C = 53: 106 planes):
  one-pixel route, 33x41: Ho x Wo = 17 x 21, 3 tiles x 21 groups = 63 units a plane, 6678 units, 27 items;
      cap 8: 3 trips + 3 workgroups, cap 24: 1 + 3; the last item holds 22 units.
  vector route, 81x48 (float32) / 81x96 (half): Ho = 41, 6 tiles x 12 groups = 72 units a plane, 7632 units,
      30 items; cap 8: 3 + 6, cap 24: 1 + 6; the last item holds 208 units.
"""
import pytest
import torch

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.testing import maxpool_ref as R

from _gpu_support import assume_cus  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
COUNTS = (1, 3, None)                   # assumed compute units; None: the device's own count
MP_BLOCKS_PER_CU = 8                    # csrc/maxpool.hip
MP_THREADS = 256
MP_TILE_H = 8
B, C = 2, 53


def cdiv(a, b):
    return -(-a // b)


def assert_trips(items):
    """non-vacuity: with one compute unit assumed every workgroup makes at least 3 trips; with one or with
    three the last trip is ragged; with the device's own count there is one trip"""
    ragged = False
    for cus, least in ((1, 3), (3, 1)):
        grid = min(items, MP_BLOCKS_PER_CU * cus)
        assert grid == MP_BLOCKS_PER_CU * cus and items // grid >= least, (items, cus)
        ragged = ragged or items % grid != 0
    assert ragged, items
    assert items <= MP_BLOCKS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count, items


@pytest.mark.parametrize('dtype', (F32, BF16, F16), ids=str)
@pytest.mark.parametrize('vector', (False, True), ids=('pixel', 'vector'))
def test_both_kernels_past_the_first_trip(assume_cus, dtype, vector):
    H, W = (81, 48 if dtype == F32 else 96) if vector else (33, 41)
    Ho, Wo = R.out_hw(H, W)
    run = (2 if dtype == F32 else 4) if vector else 1
    units = cdiv(Ho, MP_TILE_H) * (Wo // run)
    total = B * C * units
    assert_trips(cdiv(total, MP_THREADS))
    assert total % MP_THREADS != 0 and units % MP_THREADS != 0 and cdiv(Ho, MP_TILE_H) > 1
    gen = torch.Generator().manual_seed(41)
    x = ((torch.randn((B, C, H, W), generator=gen) * 2).round() / 2).to(dtype)       # many ties
    gy = torch.randn((B, C, Ho, Wo), generator=gen).to(dtype)
    xd, gd = x.to(DEV), gy.to(DEV)
    results = []
    for count in COUNTS:
        assume_cus(count)
        y, code = ops.maxpool3x3s2(xd)
        route = ops.maxpool3x3s2_route(xd, y, code)
        assert (route == L.NMSA_MP_ROUTE_VECTOR) == vector
        gx = ops.maxpool3x3s2_backward(gd, code, (H, W))
        results.append((y, code, gx))
    torch.cuda.synchronize()
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    want_y, want_code = R.forward(x)
    y, code, gx = (t.cpu() for t in results[0])
    assert torch.equal(code, want_code) and R.same_bits(y, want_y)
    assert R.same_bits(gx, R.backward_f32(gy, want_code, H, W).to(dtype))
