"""GPU tier: the four map kernels of csrc/encoder_fusion.hip past the first trip of their grid-stride
loops, in the manner of tests/test_grid_trips.py.

The kernels launch min(items, k x compute units) workgroups (k = SEF_BLOCKS_PER_CU = 8 workgroups of 256
lanes, k = SEF_BLOCK_ROUTE_PER_CU = 2 of 1024 lanes on the BLOCK route of the plane sums) and walk the
rest in a loop.  `NMSA_ASSUME_CUS` (read by the library at every call) shrinks the cap: every kernel
runs under assumed counts of 1, 3 and the device's own.  Held: the results are bit-identical across
the three counts and lie within the per-kernel bounds of testing/encoder_fusion_ref.py.

Items (B = 2, C = 53: 106 planes, no multiple of the four planes of a WAVE-route workgroup):
  k_sefuse_squeeze   WAVE route (15x20): ceil(212 / 4) = 53 items, cap 8: 6 trips + 5 workgroups, cap 24:
      2 + 5.  BLOCK route (48x80): 212 items, cap 2: 106 trips (barriers inside, LDS reused every
      trip), cap 6: 35 + 2.
  k_sefuse_wgrad     WAVE route: ceil(106 / 4) = 27 items, the last with two waves without a plane, cap 8:
      3 + 3, cap 24: 1 + 3.  BLOCK route: 106 items, cap 2: 53 trips, cap 6: 17 + 4.
  k_sefuse_scale_add, k_sefuse_apply   an item is 1024 accesses of 4 float32 / 8 half elements (VECTOR
      route) or one (ELEMENT route) of the flat tensor of 407040 elements (48x80): 100 / 50 / 398 items,
      cap 8: 12 + 4 / 6 + 2 / 49 + 6, cap 24: 4 + 4 / 2 + 2 / 16 + 14.
"""
import pytest
import torch

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.testing import encoder_fusion_ref as R

from _gpu_support import assume_cus  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
COUNTS = (1, 3, None)                   # assumed compute units; None: the device's own count
SEF_BLOCKS_PER_CU = 8                   # csrc/encoder_fusion.hip
SEF_BLOCK_ROUTE_PER_CU = 2
SEF_WAVES = 4                           # planes of a WAVE-route workgroup
SEF_ITEM = 256 * 4                      # SEF_THREADS * SEF_UNROLL accesses of an elementwise item
B, C = 2, 53
WAVE_HW, BLOCK_HW = (15, 20), (48, 80)


def cdiv(a, b):
    return -(-a // b)


def assert_trips(items, per_cu, what):
    """non-vacuity: with one compute unit assumed every workgroup makes at least 3 trips; with one or
    with three the last trip is ragged; with the device's own count there is one trip"""
    ragged = False
    for cus, least in ((1, 3), (3, 1)):
        grid = min(items, per_cu * cus)
        assert grid == per_cu * cus and items // grid >= least, (what, items, cus)
        ragged = ragged or items % grid != 0
    assert ragged, (what, items)
    own = torch.cuda.get_device_properties(0).multi_processor_count
    assert items <= per_cu * own, (what, items, own)


def moved(t):
    buf = torch.empty((t.numel() + 16,), dtype=t.dtype, device=DEV)
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    return out


@pytest.mark.parametrize('dtype', (F32, BF16, F16))
@pytest.mark.parametrize('hw,element', ((WAVE_HW, False), (BLOCK_HW, False), (BLOCK_HW, True)))
def test_map_kernels_past_the_first_trip(assume_cus, dtype, hw, element):
    n = hw[0] * hw[1]
    wave = n <= L.NMSA_SEFUSE_WAVE_PLANE_MAX
    x_rgb, x_depth, gy = R.make_inputs(B, C, hw, 77, dtype)
    gen = torch.Generator().manual_seed(78)
    w = torch.rand((2, B, C), generator=gen)
    gs = torch.randn((2, B, C), generator=gen)
    place = (lambda t: moved(t.to(DEV))) if element else (lambda t: t.to(DEV))
    xr, xd, g, wd, gsd = place(x_rgb), place(x_depth), place(gy), w.to(DEV), gs.to(DEV)
    vec = 1 if element or n % (4 if dtype == F32 else 8) else (4 if dtype == F32 else 8)
    route = ops.sefuse_route(xr, xd, g)
    assert bool(route & L.NMSA_SEFUSE_ROUTE_VECTOR) == (vec != 1) and bool(route & L.NMSA_SEFUSE_ROUTE_WAVE) == wave
    planes = B * C
    if wave:
        assert_trips(cdiv(2 * planes, SEF_WAVES), SEF_BLOCKS_PER_CU, 'k_sefuse_squeeze')
        assert_trips(cdiv(planes, SEF_WAVES), SEF_BLOCKS_PER_CU, 'k_sefuse_wgrad')
        assert planes % SEF_WAVES != 0
    else:
        assert_trips(2 * planes, SEF_BLOCK_ROUTE_PER_CU, 'k_sefuse_squeeze')
        assert_trips(planes, SEF_BLOCK_ROUTE_PER_CU, 'k_sefuse_wgrad')
        assert_trips(cdiv(planes * n // vec, SEF_ITEM), SEF_BLOCKS_PER_CU, 'k_sefuse_scale_add')
    results = []
    for count in COUNTS:
        assume_cus(count)
        results.append((ops.sefuse_squeeze(xr, xd), ops.sefuse_weight_grad(g, xr, xd), ops.sefuse_scale_add(xr, xd, wd))
                       + ops.sefuse_apply_backward(g, wd, gsd))
    torch.cuda.synchronize()
    for other in results[1:]:
        for i, (a, b) in enumerate(zip(results[0], other)):
            assert torch.equal(a, b), i
    s, gw, y, gxr, gxd = results[0]
    assert R.worst_ratio(s, R.squeeze64(x_rgb, x_depth), R.squeeze_bound(x_rgb, x_depth)) <= 1.0
    assert R.worst_ratio(gw, R.weight_grad64(gy, x_rgb, x_depth), R.weight_grad_bound(gy, x_rgb, x_depth)) <= 1.0
    assert R.worst_ratio(y, R.scale_add64(x_rgb, x_depth, w), R.scale_add_bound(x_rgb, x_depth, w, dtype=dtype)) <= 1.0
    for got, want, bnd in zip((gxr, gxd), R.apply64(gy, w, gs), R.apply_bound(gy, w, gs, dtype=dtype)):
        assert R.worst_ratio(got, want, bnd) <= 1.0
