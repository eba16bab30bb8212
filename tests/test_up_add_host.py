"""CPU tier of the fused upsampling + skip addition: the two conditions the error bounds of `testing.up_add_ref`
must meet before the GPU tier (tests/test_up_add.py) may hold the kernel to them — torch's own float32 CPU result
of the composition stays inside them on every input the bounds tier uses, and a defective restatement (bilinear
without the half-pixel offset) does not; that the float64 reference and torch agree exactly on the integer grid;
and what `ops.up2x_add` refuses without a device."""
import pytest
import torch

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.testing import up_add_ref as R

BOUNDS_SHAPES, seed_of = R.BOUNDS_SHAPES, R.bounds_seed     # the inputs of the bounds tier of tests/test_up_add.py


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('shape', BOUNDS_SHAPES)
def test_torch_float32_stays_inside_the_bounds(shape, mode):
    x, skip, _, wt, b = R.make_inputs(shape, torch.float32, seed_of(shape))
    want = R.reference64(x, skip, mode, wt, b)
    bound = R.bounds(x, skip, mode, wt, b, torch.float32)
    worst = R.worst_ratio(R.torch_up_add(x, skip, mode, wt, b), want, bound)
    print(f'torch float32 {mode} {shape}: worst error / bound {worst:.3f}')
    assert worst <= 1.0


def test_a_defective_restatement_falls_outside_the_bounds():
    shape = BOUNDS_SHAPES[0]
    x, skip, _, _, _ = R.make_inputs(shape, torch.float32, seed_of(shape))
    want = R.reference64(x, skip, 'bilinear')
    bad = R.reference64(x, skip, 'bilinear', defect='no_half_pixel')
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        assert R.worst_ratio(bad, want, R.bounds(x, skip, 'bilinear', dtype=dtype)) > 1.0, dtype


@pytest.mark.parametrize('mode', R.MODES)
def test_torch_float32_is_exact_on_the_exact_tier(mode):
    """integers in -8..8, k/16 weights: every product and sum is exact in float32, so torch's float32 composition
    equals the float64 value — the exact tier of the GPU tests asks the same of the kernel"""
    for shape in ((2, 3, 3, 5), (1, 2, 9, 8)):
        x, skip, _, wt, b = R.make_inputs(shape, torch.float32, 7, integer=True)
        want = R.reference64(x, skip, mode, wt, b)
        assert torch.equal(R.torch_up_add(x, skip, mode, wt, b).double(), want)
        assert R.bounds(x, skip, mode, wt, b).shape == want.shape


def test_bilinear_rule_of_the_reference():
    """the weights the kernel's comment names: 0.25 / 0.75 inside, 1 / 0 at the first row, 0.75 + 0.25 on the
    clamped last one"""
    from nicr_mt_scene_analysis_amd.testing.context_ref import resize_matrix
    Rm = resize_matrix(3, 6, 'bilinear')
    want = torch.tensor([[1, 0, 0], [.75, .25, 0], [.25, .75, 0], [0, .75, .25], [0, .25, .75], [0, 0, 1]],
                        dtype=torch.float64)
    assert torch.equal(Rm, want)


def test_what_the_wrapper_refuses_without_a_device():
    x, skip, _, wt, b = R.make_inputs((1, 2, 3, 4), torch.float32, 1)
    with pytest.raises(ValueError):
        ops.up2x_add(x, skip, 'bicubic')
    with pytest.raises(L.NmsaError):
        ops.up2x_add(x, skip, 'nearest')                    # CPU tensors
    with pytest.raises(L.NmsaError):
        ops.up2x_add(x, skip, 'learned-3x3', wt, b)
    assert set(ops._UPADD_MODES) == set(R.MODES)
    with pytest.raises(ValueError):
        ops.up2x_add_route(x, skip[:, :, :-1], skip)        # not [B, C, 2h, 2w]
    # the route query reads shapes, the dtype and addresses only: host tensors answer
    y = torch.empty_like(skip)
    assert ops.up2x_add_route(x, skip, y) in (L.NMSA_UPADD_ROUTE_VECTOR, L.NMSA_UPADD_ROUTE_PIXEL)
    assert ops.up2x_add_route(x[..., :3].contiguous(), skip[..., :6].contiguous(),
                              y[..., :6].contiguous()) == L.NMSA_UPADD_ROUTE_PIXEL
    with pytest.raises(L.NmsaError):
        ops.up2x_add_route(x, skip, skip)                   # y overlaps skip
