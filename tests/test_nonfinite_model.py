"""GPU tier: NaN, +inf, -inf and half-precision overflow through the model-side kernels (the batch-norm tail of
the residual blocks, the encoder RGB-D fusion, the LayerNorm-transpose fusion, the context module, the MLP
decoders, the learned upsampling).

Oracle: the plain torch composition of every entry point on the CPU in float64, forward and through autograd
(`testing.nonfinite`, which also holds the table of cases, the placements and the three assertions: class,
containment, touched-and-finite).  ONE poisoned value goes into ONE input map; the device runs once clean and
once poisoned.  The kernels that may answer NaN for an infinity (or the reverse) at a touched element are the
keys of `nonfinite.REGROUPED`, each with its reason; every other kernel must give ATen's class everywhere.
The block and the encoder-fusion cases run a second time with ONE assumed compute unit, where a workgroup
walks a poisoned unit and clean units in successive trips.

Overflow: finite float16 inputs whose float64 result passes 2 * 65504 at chosen elements and stays below
65504 / 2 elsewhere must give +-inf of the right sign exactly there (what float64 -> float16 gives); bfloat16
inputs that put the largest finite bfloat16 at chosen outputs must leave every output finite.  Not every output
can overflow: an average pool and a resize are convex combinations of their inputs.

Module level: the fused path and the torch path of the three residual blocks and of the 'se-add' fusion answer
one poisoned input with the same classes; `GradScaler` skips the step behind an infinite gradient.
"""
import pytest
import torch
import torch.nn.functional as F

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.model import block as block_module
from nicr_mt_scene_analysis_amd.testing import block_cases as BC
from nicr_mt_scene_analysis_amd.testing import block_ref as RB
from nicr_mt_scene_analysis_amd.testing import context_cases as CC
from nicr_mt_scene_analysis_amd.testing import context_ref as RC
from nicr_mt_scene_analysis_amd.testing import encoder_fusion_cases as EC
from nicr_mt_scene_analysis_amd.testing import encoder_fusion_ref as RE
from nicr_mt_scene_analysis_amd.testing import mlp_decoder_ref as RM
from nicr_mt_scene_analysis_amd.testing import nonfinite as NF
from nicr_mt_scene_analysis_amd.testing import upsampling_ref as RU

from _gpu_support import assume_cus  # noqa: F401
import test_block as TB
import test_encoder_fusion as TE

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
EPS, MOM = NF.EPS, NF.MOM
F16_MAX = 65504.0
BF16_MAX = float(torch.finfo(BF16).max)


def dev(inputs):
    return {k: v.to(DEV) for k, v in inputs.items()}


# ------------------------------------------------------------------------------ the device chains
def block_chain(case):
    act, training, backward = case.info['act'], case.info['training'], case.info['backward']

    def chain(inputs, feed):
        d = dev(inputs)
        x, idt, sc, gamma, beta = d['x'], d.get('identity'), d.get('scale'), d['gamma'], d['beta']
        B, C, H, W = x.shape
        if not backward:
            rm, rv = d['running_mean'].clone(), d['running_var'].clone()
            out = {}
            part = None
            if training:
                part = ops.bntail_stats(x)
                out['part'] = part[:C * RB.units(B, H * W) * 2].reshape(C, -1, 2).clone()
            y, mean, invstd = ops.bntail_apply(x, gamma, beta, rm, rv, EPS, MOM, act, part=part, identity=idt, scale=sc,
                                               save=True)
            out.update(y=y, mean=mean.clone(), invstd=invstd.clone(), running_mean=rm, running_var=rv)
            return out
        # the saved tensors of the composition's forward pass, rounded as the forward kernel stores them
        y_in = feed['y'].to(x.dtype).to(DEV)
        mean, invstd = feed['mean'].float().to(DEV), feed['invstd'].float().to(DEV)
        args = (d['gy'], x, y_in if act == 'relu' else idt, gamma, beta, mean, invstd, act)
        if training:
            ws = ops.bntail_backward_reduce(*args, scale=sc)
            gx, gid, dg, db = ops.bntail_backward_apply(*args, scale=sc, part=ws, need_identity=idt is not None,
                                                        need_params=True)
        else:
            dg, db = ops.bntail_backward_reduce(*args, scale=sc, finish=True)
            gx, gid, _, _ = ops.bntail_backward_apply(*args, scale=sc, need_identity=idt is not None)
        out = {'gx': gx, 'dgamma': dg.clone(), 'dbeta': db.clone()}
        if idt is not None:
            out['gid'] = gid
        return out
    return chain


def sefuse_chain(case):
    act = case.info['act']

    def chain(inputs, feed):
        d = dev(inputs)
        xr, xd, gy = d['x_rgb'], d['x_depth'], d['gy']
        P = NF.sefuse_params(d)
        s = ops.sefuse_squeeze(xr, xd)
        w, z1 = ops.sefuse_excite(s, P[0], P[1], act, save_z1=True)
        y = ops.sefuse_scale_add(xr, xd, w)
        gw = ops.sefuse_weight_grad(gy, xr, xd)
        gz2, gz1, gs, h = ops.sefuse_excite_backward(gw, w, z1, (P[0][0], P[0][2]), (P[1][0], P[1][2]), act)
        gxr, gxd = ops.sefuse_apply_backward(gy, w, gs)
        return {'s': s, 'z1': z1, 'w': w, 'y': y, 'gw': gw, 'gz2': gz2, 'gz1': gz1, 'gs': gs, 'h': h, 'gx_rgb': gxr,
                'gx_depth': gxd}
    return chain


def lnt_chain(case):
    def chain(inputs, feed):
        d = dev(inputs)
        y, mean, rstd = ops.ln_nhwc_to_nchw(d['x'], d['gamma'], d['beta'], EPS, add=d.get('add'), out_dtype=d['gy'].dtype,
                                            save_stats=True)
        gx, gg, gb = ops.ln_nhwc_to_nchw_backward(d['gy'], d['x'], d['gamma'], mean, rstd)
        return {'y': y.reshape(d['gy'].shape), 'gx': gx, 'ggamma': gg, 'gbeta': gb}
    return chain


def ppm_chain(case):
    sizes, mode = case.info['sizes'], case.info['mode']

    def chain(inputs, feed):
        d = dev(inputs)
        n = len(sizes)
        ys, gps = tuple(d[f'ys{i}'] for i in range(n)), tuple(d[f'gps{i}'] for i in range(n))
        out = {f'pooled{i}': p for i, p in enumerate(ops.ppm_pool(d['x'], sizes))}
        out['gx_pool'] = ops.ppm_pool_backward(gps, tuple(d['x'].shape), sizes)
        out['cat'] = ops.ppm_upsample_concat(d['x'], ys, mode)
        gys = ops.ppm_upsample_concat_backward(d['g_out'], d['x'].shape[1], [tuple(y.shape) for y in ys], mode)
        out.update({f'gys{i}': g for i, g in enumerate(gys)})
        return out
    return chain


def mld_chain(case):
    mode, hw, need, n = case.info['mode'], case.info['hw'], case.info['need'], case.info['n']

    def chain(inputs, feed):
        d = dev(inputs)
        ys = tuple(d[f'ys{i}'] for i in range(n))
        out = {'cat': ops.mlpdec_upsample_concat(ys, mode, size=hw)}
        gys = ops.mlpdec_upsample_concat_backward(d['g_out'], [tuple(y.shape) for y in ys], mode, need)
        for i, g in enumerate(gys):
            assert (g is None) == (need is not None and not need[i])
            if g is not None:
                out[f'gys{i}'] = g
        return out
    return chain


def up_chain(case):
    zeropad = case.info['zeropad']

    def chain(inputs, feed):
        d = dev(inputs)
        y = ops.upsample2x_dw3x3(d['x'], d['weight'], d['bias'], zeropad)
        gx, gw, gb = ops.upsample2x_dw3x3_backward(d['gy'], d['x'], d['weight'], zeropad)
        return {'y': y, 'gx': gx, 'gw': gw, 'gb': gb}
    return chain


CHAINS = {'block': block_chain, 'sefuse': sefuse_chain, 'lnt': lnt_chain, 'ppm': ppm_chain, 'mld': mld_chain,
          'up': up_chain}
DTYPE_IDS = {F32: 'f32', BF16: 'bf16', F16: 'f16'}


def _params(cases, dtypes):
    return [pytest.param(c, dt, id=f"{c.id}-{'-'.join(DTYPE_IDS[t] for t in dt) if isinstance(dt, tuple) else DTYPE_IDS[dt]}")
            for c in cases for dt in dtypes]


# ------------------------------------------------------------------------------ one poison, one input
def test_the_exception_table_names_entry_points_of_the_cases():
    kernels = set()
    for c in NF.all_cases():
        outputs, _ = c.comp(NF.to64(c.make(NF.LNT_PAIRS[0] if c.family == 'lnt' else F32)))
        kernels |= {c.kernel_of(k) for k in outputs}
    assert set(NF.REGROUPED) <= kernels, set(NF.REGROUPED) - kernels
    for exact in ('bntail_apply/eval', 'sefuse_scale_add', 'ppm_upsample_concat', 'mlpdec_upsample_concat', 'ppm_pool',
                  'ln_nhwc_to_nchw', 'sefuse_squeeze', 'sefuse_excite', 'sefuse_excite_backward'):
        assert exact in kernels and exact not in NF.REGROUPED


def test_both_routes_of_the_block_and_the_fusion_occur():
    routes = {(hw, dt): BC.expected_route(dt, hw)[0] for _, _, hw in NF.BLOCK_SHAPES for dt in NF.DTYPES}
    VECTOR, ELEMENT = L.NMSA_BNTAIL_ROUTE_VECTOR, L.NMSA_BNTAIL_ROUTE_ELEMENT
    assert routes[((15, 20), F16)] == ELEMENT and routes[(BC.EXACT_HW, F16)] == VECTOR
    assert routes[(BC.SEG_HW, F32)] == ELEMENT and routes[((15, 20), F32)] == VECTOR
    assert EC.expected_route(F32, (15, 20)) & L.NMSA_SEFUSE_ROUTE_VECTOR
    assert EC.expected_route(F16, (15, 20)) & L.NMSA_SEFUSE_ROUTE_ELEMENT
    assert EC.expected_route(F32, EC.BLOCK_HW) & L.NMSA_SEFUSE_ROUTE_BLOCK
    lds = {ops.ppm_route(hw, sizes) for hw, sizes in NF.PPM_GEOMETRIES}
    assert lds == {L.NMSA_PPM_ROUTE_LDS, L.NMSA_PPM_ROUTE_GLOBAL}


@pytest.mark.parametrize('case,dtype', _params(NF.block_cases(), NF.DTYPES))
@pytest.mark.parametrize('cus', (None, 1), ids=('own-cus', 'one-cu'))
def test_block_tail(assume_cus, case, dtype, cus):
    assume_cus(cus)
    assert NF.run(case, dtype, block_chain(case)) == 9 * len(case.maps)


@pytest.mark.parametrize('case,dtype', _params(NF.sefuse_cases(), NF.DTYPES))
@pytest.mark.parametrize('cus', (None, 1), ids=('own-cus', 'one-cu'))
def test_encoder_fusion(assume_cus, case, dtype, cus):
    assume_cus(cus)
    assert NF.run(case, dtype, sefuse_chain(case)) == 27


@pytest.mark.parametrize('case,pair', _params(NF.lnt_cases(), NF.LNT_PAIRS))
def test_layer_norm_transpose(case, pair):
    assert NF.run(case, pair, lnt_chain(case)) == 9 * len(case.maps)


@pytest.mark.parametrize('case,dtype', _params(NF.ppm_cases() + NF.mld_cases() + NF.up_cases(), NF.DTYPES))
def test_context_module_mlp_decoders_and_upsampling(case, dtype):
    assert NF.run(case, dtype, CHAINS[case.family](case)) > 0


# ------------------------------------------------------------------------------ overflow of a half output
def check_f16_overflow(got, want64, keys, floor=2.0):
    """`want64` passes `floor` * 65504 at some elements and stays below 65504 / 2 at all others; the device writes
    what float64 -> float16 gives there: +-inf of the right sign, and finite values everywhere else"""
    for k in keys:
        a = want64[k].abs()
        hot = a >= floor * F16_MAX
        assert bool(hot.any()) and not bool(hot.all()), k
        assert bool(((a < F16_MAX / 2) | hot).all()), (k, 'a value between the two sides')
        assert got[k].dtype == F16, k
        want_class = NF.classify(want64[k].to(F16))
        assert set(want_class[hot].tolist()) <= {NF.POS_INF, NF.NEG_INF} and not bool(want_class[~hot].any())
        assert torch.equal(NF.classify(got[k]).cpu(), want_class), (k, 'overflow')


def check_bf16_extreme(got, want64, keys):
    """`want64` rounds to the largest finite bfloat16 (in magnitude) at some elements; the device stays finite everywhere
    and writes that value there"""
    for k in keys:
        want = want64[k].to(BF16).double()                          # float64 -> bfloat16, one rounding
        hot = want.abs() == BF16_MAX
        assert bool(hot.any()) and bool(torch.isfinite(want).all()), k
        assert got[k].dtype == BF16 and bool(torch.isfinite(got[k]).all()), (k, 'not finite')
        assert torch.equal(got[k].cpu().double()[hot], want[hot]), k


def extreme_block_inputs(dtype, big_x, big_gamma, big_gy):
    """eval mode with running_mean 0 and running_var 1 (invstd = 1 - 5e-6): x and gy are +-1 everywhere except
    four elements of channel 2, two of each sign"""
    B, C, hw = 2, 5, (15, 20)
    gen = torch.Generator().manual_seed(71)
    sign = lambda: torch.randint(0, 2, (B, C) + hw, generator=gen) * 2.0 - 1.0
    x, gy = sign(), sign()
    hot = [(0, 2, 0, 0), (0, 2, 7, 7), (1, 2, 14, 19), (1, 2, 3, 8)]
    for n, i in enumerate(hot):
        x[i] = big_x * (1 if n % 2 == 0 else -1)
        gy[i] = big_gy * (1 if n < 2 else -1)
    gamma = torch.ones(C)
    gamma[2] = big_gamma
    return {'x': x.to(dtype), 'gy': gy.to(dtype), 'gamma': gamma, 'beta': torch.zeros(C), 'running_mean': torch.zeros(C),
            'running_var': torch.ones(C)}


def run_extreme_block(inp, act):
    d = dev(inp)
    x64 = inp['x'].double().requires_grad_(True)
    z = F.batch_norm(x64, inp['running_mean'].double(), inp['running_var'].double(), inp['gamma'].double(),
                     inp['beta'].double(), False, 0.0, EPS)
    y64 = F.relu(z) if act == 'relu' else F.silu(z)
    gx64 = torch.autograd.grad(y64, x64, inp['gy'].double())[0]
    rm, rv = d['running_mean'].clone(), d['running_var'].clone()
    y, mean, invstd = ops.bntail_apply(d['x'], d['gamma'], d['beta'], rm, rv, EPS, 0.0, act, save=True)
    gx = ops.bntail_backward_apply(d['gy'], d['x'], y if act == 'relu' else None, d['gamma'], d['beta'], mean, invstd, act)[0]
    return {'y': y, 'gx': gx}, {'y': y64.detach(), 'gx': gx64}


@pytest.mark.parametrize('act', BC.ACTS)
def test_f16_overflow_block_tail(act):
    """z = x * gamma = +-256 * 1024 = +-2^18 at the chosen elements (+-1024 elsewhere in the channel); the backward
    pass gx = gamma * gy * act' = 1024 * +-256 where the gate is open"""
    got, want = run_extreme_block(extreme_block_inputs(F16, 256.0, 1024.0, 256.0), act)
    check_f16_overflow(got, want, ('y', 'gx'))
    assert bool((got['y'] == float('inf')).any()) and bool((got['gx'] == -float('inf')).any())


def test_f16_overflow_block_tail_in_training():
    """x = +-1 in equal counts per channel (mean 0, variance 1) and gamma = 2^18 in channel 2: y = relu(+-2^18) is
    +inf where x is 1 and 0 elsewhere.  (gid = gy * act' cannot leave the range: |act'| <= 1.1 and |gy| <= 65504.)"""
    B, C, hw = 2, 5, (15, 20)
    gen = torch.Generator().manual_seed(77)
    x = torch.ones((B, C, hw[0] * hw[1]))
    for b in range(B):
        for c in range(C):
            x[b, c, torch.randperm(hw[0] * hw[1], generator=gen)[:hw[0] * hw[1] // 2]] = -1.0
    x = x.reshape((B, C) + hw).to(F16)
    gamma = torch.ones(C)
    gamma[2] = 2.0 ** 18
    y64 = F.relu(F.batch_norm(x.double(), torch.zeros(C).double(), torch.ones(C).double(), gamma.double(),
                              torch.zeros(C).double(), True, MOM, EPS))
    xd = x.to(DEV)
    y = ops.bntail_apply(xd, gamma.to(DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV),
                         torch.ones(C, device=DEV), EPS, MOM, 'relu', part=ops.bntail_stats(xd))
    check_f16_overflow({'y': y}, {'y': y64}, ('y',))


def test_bf16_extreme_block_tail():
    """x = +-max at the chosen elements under gamma 1: y = relu(x) and gx = gy pass the value itself"""
    got, want = run_extreme_block(extreme_block_inputs(BF16, BF16_MAX, 1.0, BF16_MAX), 'relu')
    check_bf16_extreme(got, want, ('y', 'gx'))


def extreme_sefuse(dtype, big, gs_big):
    """w = 1 for the rgb half and 1/2 for the depth half; x_rgb = x_depth = gy = +-`big` at four elements"""
    B, C, hw = 2, 16, (15, 20)
    gen = torch.Generator().manual_seed(72)
    xr, xd, gy = (torch.randint(-8, 9, (B, C) + hw, generator=gen).double() for _ in range(3))
    for n, i in enumerate([(0, 0, 0, 0), (0, 3, 7, 7), (1, 15, 14, 19), (1, 2, 3, 8)]):
        s = 1 if n % 2 == 0 else -1
        xr[i], xd[i], gy[i] = s * big, s * big, s * big
    w = torch.stack((torch.ones(B, C), torch.full((B, C), 0.5)))
    gs = torch.zeros(2, B, C)
    gs[0, 1, 5], gs[1, 0, 9] = gs_big * 300, -gs_big * 300           # gs / (H * W): a whole plane of each sign
    want = {'y': xr * 1.0 + xd * 0.5, 'gx_rgb': gy * 1.0 + gs[0].double()[:, :, None, None] / 300,
            'gx_depth': gy * 0.5 + gs[1].double()[:, :, None, None] / 300}
    xr, xd, gy = xr.to(dtype).to(DEV), xd.to(dtype).to(DEV), gy.to(dtype).to(DEV)
    gxr, gxd = ops.sefuse_apply_backward(gy, w.to(DEV), gs.to(DEV))
    return {'y': ops.sefuse_scale_add(xr, xd, w.to(DEV)), 'gx_rgb': gxr, 'gx_depth': gxd}, want


def test_f16_overflow_encoder_fusion():
    """scale_add: 49152 * 1 + 49152 * 0.5 = 73728 at the chosen elements; with x <= 65504 and w <= 1 no y passes
    2 * 65504, so this output is held to 65504 * 9 / 8 (73728), far above the rounding boundary 65520.
    apply_backward: gy * w + gs / n with gs / n = +-2^18 over one plane per modality"""
    got, want = extreme_sefuse(F16, 49152.0, 2.0 ** 18)
    check_f16_overflow(got, {'y': want['y']}, ('y',), floor=9.0 / 8.0)
    for k in ('gx_rgb', 'gx_depth'):
        a = want[k].abs()
        hot = a >= 2 * F16_MAX
        mid = (a >= F16_MAX / 2) & ~hot
        got_k, want_k = got[k].cpu(), want[k].clone()
        # gx_rgb = gy * 1 = +-49152 at the four elements where gy is large lies between the two sides (the planes of
        # gs hold none of them): those four are held to be finite, every other element to its class
        assert bool(hot.any()) and int(mid.sum()) == (4 if k == 'gx_rgb' else 0)
        assert torch.equal(NF.classify(got_k)[~mid], NF.classify(want_k.to(F16))[~mid]), k
        assert bool(torch.isfinite(got_k[mid]).all()), k


def test_bf16_extreme_encoder_fusion():
    """x_rgb = +-max under w = 1 beside x_depth = 0: y = x_rgb; gy = +-max under w = 1 and gs = 0: gx_rgb = gy"""
    B, C, hw = 2, 16, (15, 20)
    gen = torch.Generator().manual_seed(73)
    xr, gy = (torch.randint(-8, 9, (B, C) + hw, generator=gen).double() for _ in range(2))
    for n, i in enumerate([(0, 0, 0, 0), (0, 3, 7, 7), (1, 15, 14, 19), (1, 2, 3, 8)]):
        xr[i] = gy[i] = BF16_MAX * (1 if n % 2 == 0 else -1)
    w = torch.stack((torch.ones(B, C), torch.full((B, C), 0.5))).to(DEV)
    xd = torch.zeros_like(xr)
    y = ops.sefuse_scale_add(xr.to(BF16).to(DEV), xd.to(BF16).to(DEV), w)
    gxr, gxd = ops.sefuse_apply_backward(gy.to(BF16).to(DEV), w, torch.zeros(2, B, C, device=DEV))
    check_bf16_extreme({'y': y, 'gx_rgb': gxr}, {'y': xr, 'gx_rgb': gy}, ('y', 'gx_rgb'))
    assert bool(torch.isfinite(gxd).all())


def extreme_lnt(dtype, gamma0, big_gamma, big_add, big_gy):
    """rows of +-1 in equal counts (mean 0, variance 1); the weights are `gamma0`, channel 3 has `big_gamma`, four elements of the
    added tensor are +-`big_add` and four of gy +-`big_gy`"""
    B, P, C = 2, 33, 160
    gen = torch.Generator().manual_seed(74)
    sigma = torch.ones(C)
    sigma[torch.randperm(C, generator=gen)[:C // 2]] = -1.0
    x = sigma.expand(B, P, C).clone()
    gamma, beta = torch.full((C,), gamma0), torch.zeros(C)
    gamma[3] = big_gamma
    add = torch.randint(-8, 9, (B, C, P), generator=gen).float()
    gy = torch.randint(-2, 3, (B, C, P), generator=gen).float()
    gy[:, 3] = 0.0                                                  # the heavy channel carries no gradient
    for n, i in enumerate([(0, 0, 0), (0, 9, 31), (1, 159, 32), (1, 77, 5)]):
        s = 1 if n % 2 == 0 else -1
        add[i], gy[i] = s * big_add, s * big_gy
    inp = {'x': x.to(dtype), 'gamma': gamma, 'beta': beta, 'add': add.to(dtype), 'gy': gy.to(dtype)}
    want, _ = NF.lnt_composition(NF.to64(inp))
    d = dev(inp)
    y, mean, rstd = ops.ln_nhwc_to_nchw(d['x'], d['gamma'], d['beta'], EPS, add=d['add'], out_dtype=dtype, save_stats=True)
    gx = ops.ln_nhwc_to_nchw_backward(d['gy'], d['x'], d['gamma'], mean, rstd)[0]
    return {'y': y.reshape(B, C, P), 'gx': gx}, want


def test_f16_overflow_layer_norm_transpose():
    """y: xh * gamma = +-2^18 over the heavy channel; gx: rstd * (a - mean(a) - xh * mean(a * xh)) with a = gy * gamma
    = +-512 * 512 at four elements (the means over 160 channels stay below 65504 / 2)"""
    got, want = extreme_lnt(F16, 512.0, 2.0 ** 18, 8.0, 512.0)
    check_f16_overflow(got, want, ('y', 'gx'))


def test_bf16_extreme_layer_norm_transpose():
    """the added tensor is +-max at four elements: y = n + add rounds to +-max, nothing overflows on the way"""
    got, want = extreme_lnt(BF16, 1.0, 1.0, BF16_MAX, 1.0)
    check_bf16_extreme(got, want, ('y',))
    assert bool(torch.isfinite(got['gx']).all())


@pytest.mark.parametrize('mode', NF.PPM_MODES)
def test_f16_overflow_and_bf16_extreme_upcat_backwards(mode):
    """the only half outputs of the context module and of the MLP decoders that can leave the range: a cell's
    gradient is a SUM over the output pixels that read it (pools and resizes are convex combinations).  g_out
    = +-2048 over the 128 pixels of an 8 x 16 map: the 1 x 1 cell gets +-2^18, the other cells stay in range
    under small gradients.  bfloat16: ONE pixel of +-max beside zeros under 'nearest' hands the value through"""
    B, C, hw = 2, 3, (8, 16)
    sizes = CC.sizes_of((1, 8))
    gen = torch.Generator().manual_seed(75)
    g = torch.randint(-2, 3, (B, C + 2 * NF.PPM_CR) + hw, generator=gen).double()
    g[0, C], g[1, C + 1] = 2048.0, -2048.0                          # two planes of the 1 x 1 branch
    shapes = [(B, NF.PPM_CR, ph, pw) for ph, pw in sizes]
    ys = [torch.zeros(s, dtype=torch.float64, requires_grad=True) for s in shapes]
    want = torch.autograd.grad(RC.torch_upcat(torch.zeros((B, C) + hw, dtype=torch.float64), ys, mode), ys, g)
    got = ops.ppm_upsample_concat_backward(g.to(F16).to(DEV), C, shapes, mode)
    check_f16_overflow({'gys0': got[0]}, {'gys0': want[0]}, ('gys0',))
    assert bool(torch.isfinite(got[1]).all())
    # the MLP decoders: the same gradient without the channels of x, branches of factor 8 and 1
    gm = g[:, C:]
    mshapes = [(B, NF.PPM_CR, 1, 2), (B, NF.PPM_CR, 8, 16)]
    ym = [torch.zeros(s, dtype=torch.float64, requires_grad=True) for s in mshapes]
    wantm = torch.autograd.grad(RM.torch_upcat(ym, mode, size=hw), ym, gm)
    gotm = ops.mlpdec_upsample_concat_backward(gm.to(F16).to(DEV), mshapes, mode)
    check_f16_overflow({'gys0': gotm[0]}, {'gys0': wantm[0]}, ('gys0',))
    if mode == 'nearest':
        z = torch.zeros((B, C + 2 * NF.PPM_CR) + hw, dtype=torch.float64)
        z[0, C, 3, 5], z[1, C + 4, 7, 15] = BF16_MAX, -BF16_MAX
        want = torch.autograd.grad(RC.torch_upcat(torch.zeros((B, C) + hw, dtype=torch.float64), ys, mode), ys, z)
        got = ops.ppm_upsample_concat_backward(z.to(BF16).to(DEV), C, shapes, mode)
        check_bf16_extreme({'a': got[0], 'b': got[1]}, {'a': want[0], 'b': want[1]}, ('a', 'b'))
        gotm = ops.mlpdec_upsample_concat_backward(z[:, C:].to(BF16).to(DEV), mshapes, mode)
        wantm = torch.autograd.grad(RM.torch_upcat(ym, mode, size=hw), ym, z[:, C:])
        check_bf16_extreme({'a': gotm[0], 'b': gotm[1]}, {'a': wantm[0], 'b': wantm[1]}, ('a', 'b'))


@pytest.mark.parametrize('zeropad', (False, True))
@pytest.mark.parametrize('w', (8, 7))
def test_f16_overflow_and_bf16_extreme_upsampling(zeropad, w):
    """channel 4 has nine weights of 256 and x = gy = +-512 at an interior and a corner pixel, 0 elsewhere: every
    output a tap of them reaches is a multiple of +-2^17, every other one small.  bfloat16: the
    centre weight 1 alone hands +-max through"""
    B, C, h = 2, 13, 9
    gen = torch.Generator().manual_seed(76)
    x = torch.randint(-1, 2, (B, C, h, w), generator=gen).float()
    gy = torch.randint(-1, 2, (B, C, 2 * h, 2 * w), generator=gen).float()
    wt = torch.randint(-8, 9, (C, 1, 3, 3), generator=gen).float() / 16
    wt[4] = 256.0
    x[:, 4], gy[:, 4] = 0.0, 0.0
    b = torch.randint(-8, 9, (C,), generator=gen).float() / 16
    x[0, 4, 4, 3], x[1, 4, 0, 0], gy[0, 4, 9, 6], gy[1, 4, 17, 2 * w - 1] = 512.0, -512.0, -512.0, 512.0
    y64, gx64, _, _ = RU.reference64(x, wt, b, gy, zeropad)
    y = ops.upsample2x_dw3x3(x.to(F16).to(DEV), wt.to(DEV), b.to(DEV), zeropad)
    gx = ops.upsample2x_dw3x3_backward(gy.to(F16).to(DEV), x.to(F16).to(DEV), wt.to(DEV), zeropad)[0]
    check_f16_overflow({'y': y, 'gx': gx}, {'y': y64, 'gx': gx64}, ('y', 'gx'))
    wt[4], b[4] = 0.0, 0.0
    wt[4, 0, 1, 1] = 1.0
    x[0, 4, 4, 3], x[1, 4, 0, 0], gy[0, 4, 9, 6], gy[1, 4, 17, 2 * w - 1] = BF16_MAX, -BF16_MAX, -BF16_MAX, BF16_MAX
    y64, gx64, _, _ = RU.reference64(x.double(), wt, b, gy.double(), zeropad)
    y = ops.upsample2x_dw3x3(x.to(BF16).to(DEV), wt.to(DEV), b.to(DEV), zeropad)
    gx = ops.upsample2x_dw3x3_backward(gy.to(BF16).to(DEV), x.to(BF16).to(DEV), wt.to(DEV), zeropad)[0]
    check_bf16_extreme({'y': y, 'gx': gx}, {'y': y64, 'gx': gx64}, ('y', 'gx'))


# ------------------------------------------------------------------------------ module level
def poisoned_block_runs(module, x, gy):
    module.zero_grad(set_to_none=True)
    xx = x.clone().requires_grad_(True)
    y = module(xx)
    y.backward(gy)
    out = {'y': y.detach(), 'gx': xx.grad}
    out.update({f'grad/{k}': p.grad for k, p in module.named_parameters()})
    return out


@pytest.mark.parametrize('poison', tuple(NF.POISONS))
@pytest.mark.parametrize('training', (True, False), ids=('train', 'eval'))
@pytest.mark.parametrize('name', BC.NAMES)
def test_block_fused_and_torch_path_answer_a_poison_with_the_same_classes(monkeypatch, name, training, poison):
    """a small map takes the torch path and a large one the fused path (`block.FUSED_MIN_ELEMENTS`): the same module
    must not answer NaN for the one and 0 for the other"""
    planes, B, hw = 8, 2, (8, 16)
    inplanes = planes * BC.EXPANSION[name]
    torch.manual_seed(11)
    fused = model.get_block_class(name)(inplanes, planes).to(DEV).train(training)
    BC.randomise_running_stats(fused, 12)
    plain = model.get_block_class(name)(inplanes, planes).to(DEV).train(training)
    plain.load_state_dict(fused.state_dict())
    gen = torch.Generator().manual_seed(13)
    x = torch.randn((B, inplanes) + hw, generator=gen)
    gy = torch.randn((B, inplanes) + hw, generator=gen).to(DEV)
    x[1, 2, 3, 5] = NF.POISONS[poison]
    calls = TB.count_calls(monkeypatch)
    monkeypatch.setattr(block_module, 'FUSED_MIN_ELEMENTS', 0)
    got = poisoned_block_runs(fused, x.to(DEV), gy)
    assert calls.count('bntail_apply') == (3 if name == 'bottleneck' else 2)
    monkeypatch.setattr(block_module, '_fused_act', lambda *a: None)
    calls.clear()
    want = poisoned_block_runs(plain, x.to(DEV), gy)
    assert not calls and set(got) == set(want)
    assert not bool(torch.isfinite(want['y']).all())
    for k in want:
        a, b = NF.classify(got[k]), NF.classify(want[k])
        assert torch.equal(a, b), (k, int((a != b).sum()))


@pytest.mark.parametrize('poison', tuple(NF.POISONS))
@pytest.mark.parametrize('act', EC.ACTS)
@pytest.mark.parametrize('modality', ('x_rgb', 'x_depth'))
def test_fusion_fused_and_torch_formulation_answer_a_poison_with_the_same_classes(monkeypatch, act, modality, poison):
    C, hw = 48, (15, 20)
    inp = NF._sefuse_make(C, hw, 931)(F32)
    params = NF.sefuse_params(inp)
    module = TE.load_params(TE.build('se-add', C, act), params).to(DEV)
    inp = NF.place(inp, modality, (C + 5) * hw[0] * hw[1] + 77, NF.POISONS[poison])      # image 1, channel 5
    calls = []
    for name in ('sefuse_scale_add', 'sefuse_apply_backward'):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: calls.append(_n) or _r(*a, **k))
    got = TE.run_module(module, inp['x_rgb'].to(DEV), inp['x_depth'].to(DEV), inp['gy'].to(DEV))
    assert calls == ['sefuse_scale_add', 'sefuse_apply_backward'], 'the module did not take the fused path'
    xr, xd = (inp[k].to(DEV).requires_grad_(True) for k in ('x_rgb', 'x_depth'))
    P = tuple(tuple(p.to(DEV).requires_grad_(True) for p in group) for group in params)
    y = RE.torch_formulation(xr, xd, P, act)
    y.backward(inp['gy'].to(DEV))
    want = {'y': y.detach(), 'gx_rgb': xr.grad, 'gx_depth': xd.grad}
    for i, key in enumerate(RE.PARAM_GRADS):
        want[key] = torch.stack([group[i].grad for group in P])
    assert not bool(torch.isfinite(want['y']).all())
    for k in want:
        assert torch.equal(NF.classify(got[k]), NF.classify(want[k].reshape(got[k].shape))), k


@pytest.mark.parametrize('overflow', (True, False), ids=('inf', 'clean'))
def test_grad_scaler_skips_the_step_behind_an_infinite_gradient(monkeypatch, overflow):
    monkeypatch.setattr(block_module, 'FUSED_MIN_ELEMENTS', 0)
    B, C, hw = 2, 16, (15, 20)
    c = RB.make_tail_inputs(B, C, hw, 81, F16)
    m = TB.load_tail(TB.tail_module(C), c)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    scaler = torch.amp.GradScaler('cuda', init_scale=4.0)
    before = [p.detach().clone() for p in m.parameters()]
    calls = TB.count_calls(monkeypatch)
    mask = torch.ones((B, C) + hw, device=DEV)
    if overflow:
        mask[1, 3, 7, 11] = float('inf')
    with torch.autocast('cuda', dtype=F16):
        y = m(c['x'].to(DEV), c['identity'].to(DEV))
    assert y.dtype == F16 and calls == ['bntail_stats', 'bntail_apply']
    y = y + 1.0                                                     # the chosen element is not 0: inf * 0 would be NaN
    scaler.scale((y.float() * mask).sum()).backward()
    assert calls == list(TB.OPS[:3])                                # only the parameters need a gradient
    assert bool(torch.isinf(m.norm.bias.grad).any() | torch.isnan(m.norm.bias.grad).any()) == overflow
    scaler.step(opt)
    scaler.update()
    moved = [not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters())]
    if overflow:
        assert not any(moved) and scaler.get_scale() == 2.0
    else:
        assert all(moved) and scaler.get_scale() == 4.0
