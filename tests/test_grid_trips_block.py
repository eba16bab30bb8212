"""GPU tier: the four kernels of csrc/block_tail.hip past the first trip of their grid-stride loops, in the
manner of tests/test_grid_trips_encoder_fusion.py.

Every kernel launches min(items, BNT_BLOCKS_PER_CU = 8 workgroups per compute unit) workgroups of four waves
and walks the rest in a loop; an item is four consecutive units (a unit: one segment of 2048 elements of one
plane, one wave), or a whole channel when the backward reduction finishes alone.  `NMSA_ASSUME_CUS` (read
by the library at every call) shrinks the cap: every kernel runs under assumed counts of 1, 3 and the
device's own.  Held: the results are bit-identical across the three counts and lie within the bounds of
testing/block_ref.py.

Items (B = 2, C = 53: 106 planes):
  15x20 (one segment a plane): 106 units, ceil(106 / 4) = 27 items, the last with two waves without a unit;
      cap 8: 3 trips + 3 workgroups, cap 24: 1 + 3.
  48x80 (3840 elements, two segments a plane, the second of 1792): 212 units, 53 items; cap 8: 6 + 5,
      cap 24: 2 + 5.
  the reduction that finishes alone: 53 items (channels), barriers inside, cap 8: 6 + 5, cap 24: 2 + 5.
"""
import pytest
import torch

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.testing import block_ref as R

from _gpu_support import assume_cus  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
COUNTS = (1, 3, None)                   # assumed compute units; None: the device's own count
BNT_BLOCKS_PER_CU = 8                   # csrc/block_tail.hip
BNT_WAVES = 4                           # units of a workgroup and trip
B, C = 2, 53
EPS, MOM = 1e-5, 0.1


def cdiv(a, b):
    return -(-a // b)


def assert_trips(items, what):
    """non-vacuity: with one compute unit assumed every workgroup makes at least 3 trips; with one or with
    three the last trip is ragged; with the device's own count there is one trip"""
    ragged = False
    for cus, least in ((1, 3), (3, 1)):
        grid = min(items, BNT_BLOCKS_PER_CU * cus)
        assert grid == BNT_BLOCKS_PER_CU * cus and items // grid >= least, (what, items, cus)
        ragged = ragged or items % grid != 0
    assert ragged, (what, items)
    assert items <= BNT_BLOCKS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count, (what, items)


def moved(t):
    buf = torch.empty((t.numel() + 16,), dtype=t.dtype, device=DEV)
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    return out


@pytest.mark.parametrize('dtype', (F32, BF16, F16))
@pytest.mark.parametrize('hw,element', (((15, 20), False), ((48, 80), False), ((48, 80), True)))
def test_every_kernel_past_the_first_trip(assume_cus, dtype, hw, element):
    n = hw[0] * hw[1]
    c = R.make_tail_inputs(B, C, hw, 88, dtype)
    place = (lambda t: moved(t.to(DEV))) if element else (lambda t: t.to(DEV))
    x, idt, gy = place(c['x']), place(c['identity']), place(c['gy'])
    sc, gamma, beta = c['scale'].to(DEV), c['gamma'].to(DEV), c['beta'].to(DEV)
    vector = not element and n % (4 if dtype == F32 else 8) == 0
    route, segments = ops.bntail_route(x, idt, gy)
    assert (route == L.NMSA_BNTAIL_ROUTE_VECTOR) == vector and segments == cdiv(n, L.NMSA_BNTAIL_SEGMENT)
    units = B * C * segments
    assert_trips(cdiv(units, BNT_WAVES), 'units')
    assert_trips(C, 'channels')
    assert segments > 1 or units % BNT_WAVES != 0                # 15x20: the last workgroup has waves without a unit
    results = []
    for count in COUNTS:
        assume_cus(count)
        for act in ('relu', 'silu'):
            rm, rv = c['running_mean'].to(DEV), c['running_var'].to(DEV)
            part = ops.bntail_stats(x).clone()
            y, m, s = ops.bntail_apply(x, gamma, beta, rm, rv, EPS, MOM, act, part=part, identity=idt, scale=sc, save=True)
            args = (gy, x, y if act == 'relu' else idt, gamma, beta, m, s, act)
            ws = ops.bntail_backward_reduce(*args, scale=sc).clone()
            back = ops.bntail_backward_apply(*args, scale=sc, part=ws, need_identity=True, need_params=True)
            alone = ops.bntail_backward_reduce(*args, scale=sc, finish=True)
            results.append((part[:units * 2], y, m, s, rm, rv, ws[:units * 2]) + back + alone)
    torch.cuda.synchronize()
    per_count = len(results) // len(COUNTS)
    for k in range(per_count, len(results)):
        for i, (a, b) in enumerate(zip(results[k % per_count], results[k])):
            assert torch.equal(a, b), (k, i)
    for k, act in enumerate(('relu', 'silu')):
        part, y, m, s, rm, rv, ws, gx, gid, dg, db, dg2, db2 = results[k]
        assert torch.equal(dg, dg2) and torch.equal(db, db2)
        f = R.tail_forward(c['x'], c['gamma'], c['beta'], c['running_mean'], c['running_var'], EPS, MOM, True, act,
                           c['identity'], c['scale'], dtype)
        for got, key in ((y, 'y'), (m, 'mean'), (s, 'invstd'), (rm, 'running_mean'), (rv, 'running_var')):
            assert R.worst_ratio(got, f[key]) <= 1.0, (act, key)
        # the backward kernels took y, mean and invstd from the device: held to the restatement of exactly these
        want = R.tail_backward(c['gy'], c['x'], c['gamma'], c['beta'], m.cpu(), s.cpu(), True, act, y.cpu(),
                               c['identity'], c['scale'], dtype)
        for got, key in ((gx, 'gx'), (gid, 'gid'), (dg, 'dgamma'), (db, 'dbeta')):
            assert R.worst_ratio(got, want[key]) <= 1.0, (act, key)
