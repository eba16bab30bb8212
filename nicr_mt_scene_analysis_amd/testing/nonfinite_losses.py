"""TEST INFRASTRUCTURE — never imported by the product path.

NaN, +inf, -inf and extreme finite values through the loss kernels and the scene step: the table of cases
(inputs, placements, launch path) and the oracles, on the CPU in float64, that tests/test_nonfinite_losses.py
holds the device to and tests/test_nonfinite_losses_host.py checks for honesty.  The class map, the placer
and the three assertions are those of the model side (testing/nonfinite.py).

The rule.  A run puts ONE poison at ONE element of the prediction and compares the device
with the oracle of the same, already dtype-rounded inputs, forward and through torch.autograd with the
upstream gradient w / n (w = 1; one case with w = 3), n from the labels or the mask:
  count        equals the oracle's
  loss sum     the oracle's class; where that is finite, within RTOL (tests/test_losses.py) of it
  gradient     the class map of the oracle's gradient ROUNDED TO THE PREDICTION'S DTYPE, at every element (a
               kernel of `REGROUPED` may answer another non-finite class at a touched element)
  containment  every gradient element the poison does not touch in the oracle holds the bits of the device's
               own clean run
  touched and finite   nonfinite.assert_touched_finite with the absolute bound of the loss's clean parity test
  uncounted pixels (void label, mask 0, index 0)
               cross entropy: the oracle is F.cross_entropy(ignore_index=-1) as it is — the loss is the clean
               one, the pixel's gradient column is NaN for NaN and +inf (log_softmax's backward forms
               0 - softmax * 0) and exactly 0 for -inf;
               every other loss: the pixel is never read — loss and count hold the bits of the clean run, the
               gradient at the pixel is exactly 0 and every other element holds the clean bits (`DEVIATIONS`)

What the host tier asserts of every (case, dtype, placement, poison), on the oracle alone:
  counted placement    at least one touched and one untouched gradient element; NaN and +inf leave a non-finite
                       loss; -inf leaves a non-finite loss unless the placement's `neg_inf_finite` says that the
                       oracle maps it to a finite one (a -inf non-target class without label smoothing; the
                       exponential of the von Mises loss; the clamp of the focal loss)
  focal                torch.clamp maps +inf and -inf to its bounds: BOTH leave a finite loss (and a zero
                       gradient at the element, which is a touched one); only NaN passes the clamp
  uncounted placement  the loss is finite; cross entropy under NaN / +inf: a touched (NaN) column and an
                       untouched rest; otherwise nothing is touched at all
"""
import copy
import math

import torch
import torch.nn.functional as F

from .nonfinite import (BF16, DTYPES, F16, F32, FINITE, POISONS, U_OUT, assert_class, assert_contained,      # noqa: F401
                        assert_touched_finite, classify, place, touched)

RTOL = 1e-5                                     # tests/test_losses.py: the loss sums of the clean parity tests
EPS_COS = 1e-12                                 # ATen's cosine_embedding_loss, inside both norms
B = 2
SHAPES = ((3, 5), (4, 16))                      # P = 15: element route, ragged last lane; P = 64: 16-byte route

# The losses whose reference multiplies by the mask (`pred * mask`: instance helper's MSE / L1; the focal
# test oracle's `val * mask`) where the kernels select (`mask ? x : 0`).  A NaN or an infinity at a masked-out
# pixel gives the reference a NaN loss (NaN * 0); on the device the pixel is never read.  Stated and pinned,
# like the normal task's and the cosine loss's no-target pixels; the oracles below select as the kernels do.
DEVIATIONS = {
    'masked-out pixels of mse / l1 / focal': 'the kernels select on the mask, the reference multiplies by it: a '
                                             'poison at a masked-out pixel leaves loss, count and every gradient '
                                             'element as in the clean run, the gradient at the pixel exactly 0',
}

# Kernels whose arithmetic is grouped otherwise than ATen's and which may therefore answer NaN for an infinity
# or the reverse at a touched element (never a finite value for a non-finite one, or the reverse).
REGROUPED = {
}

# Domain limits, stated in DESIGN.md 6n and not tested past:
CE_MAX_ABS = 1.7e38                             # FLT_MAX / 2: with two logits of opposite sign beyond it, x - max
                                                # and the loss term lse - x_t leave float32's range
COS_MAX_ABS = 1.8e19                            # a square beyond float32's largest value (sqrt(3.4e38))


def grad_rtol(dtype):
    """tests/test_wide_column_losses.py `_grad_tol`"""
    return {F32: 2e-5, BF16: 2.0 ** -7, F16: 2.0 ** -9}[dtype]


def upstream(w_up: float, n: int) -> float:
    """the float32 value of ATen's `w / n` (loss/_functional.py expected_scale), as a Python float"""
    return float(torch.tensor(float(w_up), dtype=torch.float32) / torch.tensor(max(int(n), 1), dtype=torch.int64))


def to64(inputs: dict) -> dict:
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inputs.items()}


class Place:
    """one placement: the flat index of the poisoned element of `x` (per poison where the loss needs it), whether
    the pixel counts, and whether the oracle maps a -inf there to a finite loss"""

    def __init__(self, label, index, counted=True, neg_inf_finite=False, pixel=None):
        self.label, self.counted, self.neg_inf_finite, self.pixel = label, counted, neg_inf_finite, pixel
        self._index = index

    def index(self, poison):
        return self._index[poison] if isinstance(self._index, dict) else self._index

    def __repr__(self):
        return self.label


class Case:
    """kind: ce | mse | l1 | focal | vonmises | cos; path: how the GPU tier reaches the kernel the row names
    make(dtype) -> dict of CPU tensors, `x` the prediction rounded to dtype
    count(inputs) -> n; oracle(inputs64, up) -> {'loss': 0-d, 'grad': like x} in float64
    places(inputs) -> [Place]; w_up: the factor of the upstream gradient w / n; clamps: the loss clamps infinities"""

    def __init__(self, ident, kind, path, make, count, oracle, places, w_up=1.0, clamps=False, **info):
        self.id, self.kind, self.path, self.make, self.count, self.oracle = ident, kind, path, make, count, oracle
        self.places, self.w_up, self.clamps, self.info = places, w_up, clamps, info

    def __repr__(self):
        return self.id


def grad_tol(case, dtype, inputs, clean_grad64, up) -> float:
    """the absolute bound of the clean parity test of the loss and dtype"""
    sub = 6e-8 if dtype == F16 else 0.0                             # f16 subnormals
    gmax = float(clean_grad64[torch.isfinite(clean_grad64)].abs().max())
    if case.kind in ('ce', 'scene'):                                # test_ce_split_vs_torch_fp64
        return max(grad_rtol(dtype) * gmax * 0.05, 4e-6 * float(inputs['w'].max()) * up, sub)
    if case.kind == 'cos':                                          # test_cos_emb_vs_torch_fp64
        return grad_rtol(dtype) * gmax * 0.05 + (sub or 1e-12)
    if case.kind == 'focal':                                        # test_center_focal_loss_extension_vs_torch
        return 1e-5 if dtype == F32 else 2e-2                       # (float16: the bound of the coarser bfloat16)
    return 1e-7 + sub                                               # test_instance_losses_vs_reference_golden


def clean_rtol(case, dtype) -> float:
    if case.kind == 'focal':
        return 1e-4 if dtype == F32 else 2e-2
    return grad_rtol(dtype)


# ------------------------------------------------------------------------------------------ cross entropy
def _pixel_mask(x, b, p):
    """boolean map of x [B, C, H, W] / [B, H, W]: every channel of pixel p of image b"""
    m = torch.zeros(x.shape, dtype=torch.bool)
    if x.ndim == 3:
        m.view(x.shape[0], -1)[b, p] = True
    else:
        m.view(x.shape[0], x.shape[1], -1)[b, :, p] = True
    return m


def _flat(x, b, c, p):
    if x.ndim == 3:
        return b * x.shape[1] * x.shape[2] + p
    return (b * x.shape[1] + c) * x.shape[2] * x.shape[3] + p


CE_T = 1                                        # the target class (label 2) at both counted placements


def _ce_make(C, hw, seed, wide):
    def make(dtype):
        g = torch.Generator().manual_seed(seed)
        H, W = hw
        x = (torch.randn((B, C, H, W), generator=g) * 3).to(dtype)
        t = torch.randint(1, C + 1, (B, H, W), generator=g)
        t[torch.rand((B, H, W), generator=g) < 0.2] = 0
        tv = t.view(B, -1)
        tv[0, 0], tv[1, -1], tv[0, (H * W) // 2] = CE_T + 1, CE_T + 1, 0
        w = torch.rand((C,), generator=g) + 0.5
        return {'x': x, 't': t.to(torch.int16 if wide else torch.uint8), 'w': w}
    return make


def _ce_count(inp):
    return int((inp['t'] != 0).sum())


def _ce_oracle(ls):
    def oracle(inp, up):
        x = inp['x'].clone().requires_grad_(True)
        loss = F.cross_entropy(x, inp['t'].long() - 1, inp['w'], reduction='sum', ignore_index=-1, label_smoothing=ls)
        grad, = torch.autograd.grad(loss, x, torch.tensor(up, dtype=torch.float64))
        return {'loss': loss.detach(), 'grad': grad}
    return oracle


def _ce_places(ls):
    def places(inp):
        x = inp['x']
        C, P = x.shape[1], x.shape[2] * x.shape[3]
        out = []
        for tag, b, p in (('first', 0, 0), ('last', 1, P - 1)):
            out.append(Place(f'{tag}/target', _flat(x, b, CE_T, p), pixel=(b, p)))
            out.append(Place(f'{tag}/non-target', _flat(x, b, CE_T + 1, p), neg_inf_finite=ls == 0.0, pixel=(b, p)))
            out.append(Place(f'{tag}/class C-1', _flat(x, b, C - 1, p), neg_inf_finite=ls == 0.0, pixel=(b, p)))
        out.append(Place('void', _flat(x, 0, C // 2, P // 2), counted=False, pixel=(0, P // 2)))
        return out
    return places


# (path, classes): the kernel each row reaches is asserted by the GPU tier from what Python can see
CE_PATHS = (('expect', (5, 40, 48, 49, 150)),   # k_ce_fused NG 3 / 5 / 6 (C <= 48), k_ce_split above
            ('two-kernel', (5, 150, 300)),      # nmsa_loss_ce_fwd + _bwd with the saved log-sum-exp; 300: int16 labels
            ('forward', (5, 150)),              # requires_grad=False
            ('multi', (40, 150)))               # _multi.multi_loss: in the joint launch / its own kernel


def ce_cases():
    out = []
    for path, classes in CE_PATHS:
        for C in classes:
            for ls in (0.0, 0.1):
                for k, hw in enumerate(SHAPES):
                    # (the upstream factor 3: once, on the widest fused column)
                    w_up = 3.0 if (path, C, ls, k) == ('expect', 48, 0.1, 0) else 1.0
                    out.append(Case(f'ce-{path}-C{C}-ls{ls}-{hw[0]}x{hw[1]}', 'ce', path,
                                    _ce_make(C, hw, 100 + C + k, C > 255), _ce_count, _ce_oracle(ls), _ce_places(ls),
                                    w_up=w_up, C=C, ls=ls, hw=hw))
    return out


# ------------------------------------------------------------------------------------------ MSE, L1, focal
def _mask(hw, g):
    """about a third of the pixels out; the two corner placements in, the middle pixel of image 0 out"""
    H, W = hw
    m = torch.rand((B, H, W), generator=g) >= 1.0 / 3.0
    mv = m.view(B, -1)
    mv[0, 0], mv[1, -1], mv[0, (H * W) // 2] = True, True, False
    return m


def _elem_make(kind, C, hw, seed):
    def make(dtype):
        g = torch.Generator().manual_seed(seed)
        H, W = hw
        shape = (B, H, W) if C == 1 else (B, C, H, W)
        x, y = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        if kind == 'l1':
            # channel 0 below its target, channel 1 above, at the counted placements: an infinity must change
            # the sign the clean gradient has there (L1Loss's gradient is the sign alone)
            for b, p in ((0, 0), (1, H * W - 1)):
                x.view(B, C, -1)[b, :, p] = torch.tensor([0.25, 0.75])
                y.view(B, C, -1)[b, :, p] = 0.5
        return {'x': x.to(dtype), 'y': y, 'm': _mask(hw, g)}
    return make


def _mask_count(inp):
    return int(inp['m'].sum())


def _elem_oracle(kind):
    def oracle(inp, up):
        x = inp['x'].clone().requires_grad_(True)
        m = inp['m'] if x.ndim == 3 else inp['m'].unsqueeze(1)
        d = torch.where(m, x, torch.zeros_like(x)) - inp['y']       # the select of the kernels (DEVIATIONS)
        f = d * d if kind == 'mse' else d.abs()
        loss = (f if x.ndim == 3 else f.mean(dim=1)).sum()
        grad, = torch.autograd.grad(loss, x, torch.tensor(up, dtype=torch.float64))
        return {'loss': loss.detach(), 'grad': grad}
    return oracle


def _elem_places(kind):
    def places(inp):
        x = inp['x']
        P = x.shape[-1] * x.shape[-2]
        out = []
        for tag, b, p in (('first', 0, 0), ('last', 1, P - 1)):
            if kind == 'l1':
                index = {'nan': _flat(x, b, 0, p), '+inf': _flat(x, b, 0, p), '-inf': _flat(x, b, 1, p)}
            else:
                index = _flat(x, b, 0 if tag == 'first' else (x.shape[1] - 1 if x.ndim == 4 else 0), p)
            out.append(Place(tag, index, neg_inf_finite=kind == 'focal', pixel=(b, p)))
        out.append(Place('masked-out', _flat(x, 0, 0, P // 2), counted=False, pixel=(0, P // 2)))
        return out
    return places


def _focal_make(hw, seed):
    def make(dtype):
        g = torch.Generator().manual_seed(seed)
        H, W = hw
        x = torch.rand((B, H, W), generator=g) * 0.9 + 0.05
        y = torch.rand((B, H, W), generator=g) ** 4
        y[torch.rand((B, H, W), generator=g) < 0.1] = 1.0
        y.view(B, -1)[0, 0] = 1.0                                   # first placement: the positive branch
        y.view(B, -1)[1, -1] = 0.3                                  # last placement: the penalty-reduced one
        return {'x': x.to(dtype), 'y': y, 'm': _mask(hw, g)}
    return make


def _focal_count(inp):
    return max(int(((inp['y'] == 1) & inp['m']).sum()), 1)


def _focal_oracle(inp, up):
    x, y = inp['x'].clone().requires_grad_(True), inp['y']
    p = torch.clamp(x, 1e-4, 1 - 1e-4)
    val = torch.where(y == 1, -(1 - p) ** 2 * torch.log(p), -(1 - y) ** 4 * p ** 2 * torch.log(1 - p))
    loss = torch.where(inp['m'], val, torch.zeros_like(val)).sum()
    grad, = torch.autograd.grad(loss, x, torch.tensor(up, dtype=torch.float64))
    return {'loss': loss.detach(), 'grad': grad}


ELEM_PATHS = ('expect', 'two-kernel', 'multi')  # k_elem_fused / k_vm_fused; *_fwd + *_bwd; the joint launch


def elem_cases():
    out = []
    for kind, C in (('mse', 1), ('mse', 2), ('l1', 2)):
        for path in ELEM_PATHS:
            for k, hw in enumerate(SHAPES):
                out.append(Case(f'{kind}-C{C}-{path}-{hw[0]}x{hw[1]}', kind, path, _elem_make(kind, C, hw, 300 + 10 * C + k),
                                _mask_count, _elem_oracle(kind), _elem_places(kind), C=C, hw=hw))
    for path in ('two-kernel', 'multi'):        # the divisor is the number of peaks: no expectation exists
        for k, hw in enumerate(SHAPES):
            out.append(Case(f'focal-{path}-{hw[0]}x{hw[1]}', 'focal', path, _focal_make(hw, 340 + k), _focal_count,
                            _focal_oracle, _elem_places('focal'), clamps=True, hw=hw))
    return out


# ------------------------------------------------------------------------------------------ von Mises
def _vm_make(hw, seed):
    def make(dtype):
        g = torch.Generator().manual_seed(seed)
        H, W = hw
        x = F.normalize(torch.randn((B, 2, H, W), generator=g), dim=1) * 0.9
        y = F.normalize(torch.randn((B, 2, H, W), generator=g), dim=1)
        for b, p in ((0, 0), (1, H * W - 1)):                       # both target components positive: +inf * y = +inf
            y.view(B, 2, -1)[b, :, p] = torch.tensor([0.6, 0.8])
        return {'x': x.to(dtype), 'y': y, 'm': _mask(hw, g)}
    return make


def _vm_oracle(kappa):
    def oracle(inp, up):
        x = inp['x'].clone().requires_grad_(True)
        rows, tgt = x.permute(0, 2, 3, 1)[inp['m']], inp['y'].permute(0, 2, 3, 1)[inp['m']]
        loss = (1 - torch.exp(kappa * ((rows * tgt).sum(dim=1) - 1))).sum()
        grad, = torch.autograd.grad(loss, x, torch.tensor(up, dtype=torch.float64))
        return {'loss': loss.detach(), 'grad': grad}
    return oracle


def _vm_places(inp):
    x = inp['x']
    P = x.shape[2] * x.shape[3]
    return [Place('first', _flat(x, 0, 0, 0), neg_inf_finite=True, pixel=(0, 0)),
            Place('last', _flat(x, 1, 1, P - 1), neg_inf_finite=True, pixel=(1, P - 1)),
            Place('masked-out', _flat(x, 0, 1, P // 2), counted=False, pixel=(0, P // 2))]


def vm_cases():
    out = []
    for kappa in (1.0, 4.0):
        for path in ELEM_PATHS:
            for k, hw in enumerate(SHAPES):
                out.append(Case(f'vonmises-k{kappa:g}-{path}-{hw[0]}x{hw[1]}', 'vonmises', path, _vm_make(hw, 360 + k),
                                _mask_count, _vm_oracle(kappa), _vm_places, kappa=kappa, hw=hw))
    return out


# ------------------------------------------------------------------------------------------ cosine, lut_sum
# (D, (H, W), the kernel, the dispatch condition of csrc/losses_cos.hip cos_kernel(), lines 558-583)
COS_L = 5
COS_ROUTES = (
    (64, (4, 16), 'k_cos_split', 'line 571: D % 64 == 0 and D / 64 <= 8 waves; line 579 keeps D < 512 there'),
    (64, (2, 6), 'k_cos_split', 'as above; 12 pixels: whole groups of 4 (f32: 2), one ragged wave of groups'),
    (100, (4, 16), 'k_cos_parts', 'line 562 / 571: D % 64 != 0 rules k_cos_split out; line 572: D <= 4 * 256'),
    (100, (2, 6), 'k_cos_parts', 'as above'),
    (1030, (3, 5), 'two-walk', 'line 572: D > 1024 rules k_cos_parts out; P = 15 is no whole pixel group either '
                               '(loss/_multi.py cos_supported): k_cos_emb forward, then backward'),
)
COS_ZERO_PIXEL = 1                              # image 0: a zero prediction vector at a counted pixel


def _cos_make(D, hw, seed):
    def make(dtype):
        g = torch.Generator().manual_seed(seed)
        H, W = hw
        x = torch.randn((B, D, H, W), generator=g)
        lut = F.normalize(torch.randn((B, COS_L, D), generator=g), dim=-1)
        idx = torch.randint(0, COS_L + 1, (B, H, W), generator=g, dtype=torch.int32)
        iv = idx.view(B, -1)
        iv[0, 0], iv[0, COS_ZERO_PIXEL], iv[1, -1], iv[0, (H * W) // 2] = 1, 3, 2, 0
        x.view(B, D, -1)[0, :, COS_ZERO_PIXEL] = 0.0
        return {'x': x.to(dtype), 'idx': idx, 'lut': lut}
    return make


def _cos_count(inp):
    return int((inp['idx'] != 0).sum())


def _cos_oracle(inp, up):
    x = inp['x'].clone().requires_grad_(True)
    valid = inp['idx'] != 0
    rows = x.permute(0, 2, 3, 1)[valid]
    tgt = inp['lut'][torch.where(valid)[0], (inp['idx'][valid] - 1).long()]
    cos = (rows * tgt).sum(1) / torch.sqrt(((rows * rows).sum(1) + EPS_COS) * ((tgt * tgt).sum(1) + EPS_COS))
    loss = (1 - cos).sum()
    grad, = torch.autograd.grad(loss, x, torch.tensor(up, dtype=torch.float64))
    return {'loss': loss.detach(), 'grad': grad}


def _cos_places(inp):
    x = inp['x']
    D, P = x.shape[1], x.shape[2] * x.shape[3]
    return [Place('first/plane 0', _flat(x, 0, 0, 0), pixel=(0, 0)),
            Place('last/plane D-1', _flat(x, 1, D - 1, P - 1), pixel=(1, P - 1)),
            Place('no target', _flat(x, 0, D // 2, P // 2), counted=False, pixel=(0, P // 2))]


def cos_cases():
    return [Case(f'cos-D{D}-{hw[0]}x{hw[1]}', 'cos', route, _cos_make(D, hw, 400 + D + hw[1]), _cos_count, _cos_oracle,
                 _cos_places, D=D, hw=hw, condition=why) for D, hw, route, why in COS_ROUTES]


def all_cases():
    return ce_cases() + elem_cases() + vm_cases() + cos_cases()


# ------------------------------------------------------------------------------------------ the run
def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    kind = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.view(kind), b.view(kind))


def check_clean(case, dtype, inputs, got, want, up):
    """the clean run within the bounds of the clean parity tests (the zero vector of the cosine cases lives here)"""
    tag = (case.id, str(dtype), 'clean')
    assert int(got['count']) == case.count(inputs), tag
    lw, lg = float(want['loss']), float(got['loss'])
    assert math.isfinite(lg) and abs(lg - lw) <= RTOL * abs(lw), (tag, 'loss', lg, lw)
    if got.get('grad') is None:
        return
    g, w = got['grad'].detach().cpu().double(), want['grad']
    assert got['grad'].dtype == dtype and g.shape == w.shape, tag
    room = grad_tol(case, dtype, inputs, w, up) + (clean_rtol(case, dtype) + U_OUT[dtype]) * w.abs()
    assert bool(torch.isfinite(g).all()) and bool(((g - w).abs() <= room).all()), (tag, 'grad', float(((g - w).abs() - room).max()))


def compare(case, dtype, inputs, pl, got, got_clean, want, want_clean, up, tag):
    """the device's answer to one poisoned (or extreme) input against the oracle's: the rule of the module docstring"""
    assert int(got['count']) == case.count(inputs), (tag, 'count')
    read = pl.counted or case.kind == 'ce'
    lw, lg = want['loss'], got['loss'].detach().cpu()
    if read:
        assert int(classify(lg)) == int(classify(lw)), (tag, 'loss class', float(lg), float(lw))
        if bool(torch.isfinite(lw)):
            assert abs(float(lg) - float(lw)) <= RTOL * abs(float(lw)), (tag, 'loss', float(lg), float(lw))
    if not pl.counted:
        assert _bits_equal(lg, got_clean['loss']), (tag, 'the loss of an uncounted pixel moved', float(lg))
    if got.get('grad') is None:
        return
    g, gc = got['grad'], got_clean['grad']
    assert g.dtype == dtype and tuple(g.shape) == tuple(want['grad'].shape), tag
    if not read:
        pixel = _pixel_mask(inputs['x'], *pl.pixel)
        assert bool((g.detach().cpu()[pixel] == 0).all()), (tag, 'the gradient of a pixel that is never read')
        assert_contained(g, gc, pixel, tag)
        return
    mask = touched(want_clean['grad'], want['grad'])
    assert_class(g, want['grad'].to(dtype).double(), mask, case.info.get('kernel') in REGROUPED, tag)
    assert_contained(g, gc, mask, tag)
    assert_touched_finite(g, want['grad'], mask, grad_tol(case, dtype, inputs, want_clean['grad'], up), tag)


def run(case, dtype, device_fn=None, poisons=POISONS):
    """every poison at every placement of the case.  `device_fn(case, inputs)` -> {'loss', 'count', 'grad' | None}
    of the device; None: the oracle alone (the host tier).  -> the number of poisoned runs"""
    clean = case.make(dtype)
    n = case.count(clean)
    up = upstream(case.w_up, n)
    want_clean = case.oracle(to64(clean), up)
    assert bool(torch.isfinite(want_clean['loss'])) and bool(torch.isfinite(want_clean['grad']).all()), case.id
    got_clean = None
    if device_fn:
        got_clean = device_fn(case, clean)
        check_clean(case, dtype, clean, got_clean, want_clean, up)
    runs = 0
    for pl in case.places(clean):
        for pname, value in poisons.items():
            tag = (case.id, str(dtype), pl.label, pname)
            inputs = place(clean, 'x', pl.index(pname), value)
            assert case.count(inputs) == n, tag
            want = case.oracle(to64(inputs), up)
            mask = touched(want_clean['grad'], want['grad'])
            finite_loss = bool(torch.isfinite(want['loss']))
            if pl.counted:
                assert 0 < int(mask.sum()) < mask.numel(), (tag, 'nothing touched or nothing left')
                if case.clamps and pname != 'nan':
                    assert finite_loss, (tag, 'torch.clamp maps an infinity to its bound')
                elif pname == '-inf':
                    assert finite_loss == pl.neg_inf_finite, (tag, 'the table says otherwise of -inf', float(want['loss']))
                else:
                    assert not finite_loss, (tag, 'a NaN and a +inf must reach the loss')
            else:
                assert finite_loss, (tag, 'an uncounted pixel reached the loss')
                if case.kind == 'ce' and pname != '-inf':
                    column = _pixel_mask(clean['x'], *pl.pixel)
                    assert torch.equal(mask, column) and bool(torch.isnan(want['grad'][column]).all()), tag
                else:
                    assert not bool(mask.any()), (tag, 'an uncounted pixel touched a gradient')
            runs += 1
            if device_fn:
                compare(case, dtype, inputs, pl, device_fn(case, inputs), got_clean, want, want_clean, up, tag)
    return runs


# ------------------------------------------------------------------------------------------ extremes (finite)
def extreme_value(dtype) -> float:
    return 65504.0 if dtype == F16 else 1e30


def extreme_cases():
    """(case, [(label, {flat index: value}, pixel)]) per dtype through `extremes(case, dtype)`: finite values at
    the edge of the formats, compared in class and within the clean bounds"""
    out = []
    # the same paths as the poisons: every (path, C) row of CE_PATHS, both label smoothings, both routes (the
    # 16-byte route also stores and loads the two saved planes of the two-kernel path as float4)
    for path, classes in CE_PATHS:
        for C in classes:
            for ls in (0.0, 0.1):
                for k, hw in enumerate(SHAPES):
                    out.append(Case(f'ce-{path}-C{C}-ls{ls}-{hw[0]}x{hw[1]}-extreme', 'ce', path,
                                    _ce_make(C, hw, 500 + C + k, C > 255), _ce_count, _ce_oracle(ls), _ce_places(ls),
                                    C=C, ls=ls, hw=hw))
    for path in ELEM_PATHS:
        for k, hw in enumerate(SHAPES):
            out.append(Case(f'mse-C1-{path}-{hw[0]}x{hw[1]}-extreme', 'mse', path, _elem_make('mse', 1, hw, 510 + k),
                            _mask_count, _elem_oracle('mse'), _elem_places('mse'), C=1, hw=hw))
            out.append(Case(f'vonmises-k1-{path}-{hw[0]}x{hw[1]}-extreme', 'vonmises', path, _vm_make(hw, 520 + k),
                            _mask_count, _vm_oracle(1.0), _vm_places, kappa=1.0, hw=hw))
    for D, hw, route, why in COS_ROUTES[::2]:
        out.append(Case(f'cos-D{D}-extreme', 'cos', route, _cos_make(D, hw, 530 + D), _cos_count, _cos_oracle,
                        _cos_places, D=D, hw=hw, condition=why))
    return out


def extremes(case, dtype):
    """-> [(label, edits {flat index of x: value} | None, x-wide edit function | None, w_up)] or [] where the issue
    names no extreme for the (loss, dtype)"""
    clean = case.make(dtype)
    x = clean['x']
    big = extreme_value(dtype)
    out = []
    if case.kind == 'ce':
        C, P = x.shape[1], x.shape[2] * x.shape[3]
        for sign in (1.0, -1.0):
            out.append((f'target {sign * big:g}', {_flat(x, 0, CE_T, 0): sign * big}, 1.0))
            out.append((f'non-target {sign * big:g}', {_flat(x, 1, CE_T + 1, P - 1): sign * big}, 1.0))
        # a column whose values all sit at 1e4 +- 1: the maximum must be subtracted before the exponential
        column = {_flat(x, 0, c, 0): 1e4 + (c % 3 - 1) for c in range(C)}
        out.append(('column at 1e4 +- 1', column, 1.0))
    elif case.kind == 'mse' and dtype == F16:
        # 65504 against -65504: d = 131008, the gradient 2 d w / n overflows float16 with w = 8: +inf on the
        # device and in the rounded oracle
        out.append(('65504 against -65504', {_flat(x, 0, 0, 0): 65504.0, 'y': -65504.0}, 8.0))
    elif case.kind == 'vonmises' and dtype == BF16:
        out.append(('1e30', {_flat(x, 0, 0, 0): 1e30}, 1.0))        # exp overflows to +inf, the loss to -inf
    elif case.kind == 'cos':
        v = 65504.0 if dtype == F16 else 1e15                       # the squares still fit float32 (COS_MAX_ABS)
        D, P = x.shape[1], x.shape[2] * x.shape[3]
        out.append((f'{v:g}', {_flat(x, 0, 0, 0): v, _flat(x, 1, D - 1, P - 1): -v}, 1.0))
    return out


def run_extremes(case, dtype, device_fn=None, only=None):
    clean = case.make(dtype)
    n = case.count(clean)
    runs = 0
    for k, (label, edits, w_up) in enumerate(extremes(case, dtype)):
        if only is not None and k != only:
            continue
        run_case = copy.copy(case)                                  # (the table's cases are shared: never written to)
        run_case.w_up = w_up
        up = upstream(w_up, n)
        inputs = dict(clean)
        inputs['x'] = clean['x'].clone()
        for index, value in edits.items():
            if index == 'y':                                        # the target of the first pixel
                inputs['y'] = clean['y'].clone()
                inputs['y'].view(-1)[0] = value
            else:
                inputs['x'].view(-1)[index] = value
        tag = (case.id, str(dtype), label)
        assert bool(torch.isfinite(inputs['x'].float()).all()), (tag, 'an extreme that the dtype does not hold')
        want, want_clean = case.oracle(to64(inputs), up), case.oracle(to64(clean), up)
        runs += 1
        if device_fn is None:
            continue
        got, got_clean = device_fn(run_case, inputs), device_fn(run_case, clean)
        assert int(got['count']) == n, tag
        lw, lg = want['loss'], got['loss'].detach().cpu()
        assert int(classify(lg)) == int(classify(lw)), (tag, 'loss class', float(lg), float(lw))
        if bool(torch.isfinite(lw)):
            assert abs(float(lg) - float(lw)) <= RTOL * abs(float(lw)), (tag, 'loss', float(lg), float(lw))
        if got.get('grad') is None:                                 # the forward-only path
            assert case.path == 'forward', tag
            continue
        mask = touched(want_clean['grad'], want['grad'])
        assert_class(got['grad'], want['grad'].to(dtype).double(), mask, False, tag)
        assert_contained(got['grad'], got_clean['grad'], mask, tag)
        # (an element whose rounded oracle value overflows the dtype is compared in class alone)
        finite = want['grad'].clone()
        finite[~torch.isfinite(want['grad'].to(dtype).double())] = math.inf
        assert_touched_finite(got['grad'], finite, mask, grad_tol(case, dtype, inputs, want_clean['grad'], up), tag)
    return runs


# ------------------------------------------------------------------------------------------ scene step
SCENE_B = 6
SCENE_VOID_ROWS = (2, 5)
SCENE_CLASSES = (3, 45, 70)                     # 70: more than one class per lane (lanes 0..5 take c and c + 64)


def scene_inputs(C, dtype, seed=0):
    g = torch.Generator().manual_seed(600 + C + seed)
    x = (torch.randn((SCENE_B, C), generator=g) * 3).to(dtype)
    labels = torch.randint(1, C + 1, (SCENE_B,), generator=g)
    labels[list(SCENE_VOID_ROWS)] = 0
    labels[0], labels[SCENE_B - 2] = 2, 2                           # class 1 at the two counted placements
    return {'x': x, 'labels': labels, 'w': torch.rand((C,), generator=g) + 0.25}


def scene_places(C):
    """(label, row, class, counted): class 0, a middle class, C - 1, and class 64 where a lane takes two"""
    classes = [0, C // 2, C - 1] + ([64] if C > 64 else [])
    out = [(f'row {r}/class {c}', r, c, True) for r in (0, SCENE_B - 2) for c in classes]
    out += [(f'void row {SCENE_VOID_ROWS[0]}/class {c}', SCENE_VOID_ROWS[0], c, False) for c in classes]
    return out


def scene_oracle(inp, eps):
    """softmax -> max for score and index (model/postprocessing/scene.py:42-44), F.cross_entropy ('mean',
    ignore_index=-1) for loss and gradient, the confusion matrix over (label - 1, index) of the non-void rows"""
    x = inp['x'].double().clone().requires_grad_(True)
    C = x.shape[1]
    target = inp['labels'].long() - 1
    score, idx = torch.max(F.softmax(x.detach(), dim=1), dim=1)
    loss = F.cross_entropy(x, target, inp['w'].double(), ignore_index=-1, label_smoothing=eps, reduction='mean')
    grad, = torch.autograd.grad(loss, x)
    valid = target >= 0
    cm = torch.bincount(target[valid] * C + idx[valid], minlength=C * C).reshape(C, C)
    return {'score': score, 'idx': idx, 'loss': loss.detach(), 'grad': grad, 'cm': cm}


def scene_all_neg_inf(inp, row):
    out = dict(inp)
    out['x'] = inp['x'].clone()
    out['x'][row] = -math.inf
    return out


# ------------------------------------------------------------------------------------------ the forms of losses_forms.hip
FORM_N = 7                                      # rows; a poison in row r touches output r and the gradient of row r only
FORM_ROWS = (0, 3, FORM_N - 1)                  # the poisoned rows: first, one with a dissimilar pair, last
FORM_LABELS = (1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0)


def _form_make(kind, D, seed):
    def make(dtype):
        g = torch.Generator().manual_seed(seed)
        x, y = torch.randn((FORM_N, D), generator=g), torch.randn((FORM_N, D), generator=g)
        for r in FORM_ROWS:
            if kind in ('mse', 'l1'):
                x[r, :2], y[r, :2] = torch.tensor([0.25, 0.75]), 0.5        # element 0 below its target, 1 above (L1's sign)
            elif kind == 'vonmises':
                y[r] = torch.tensor([0.6, 0.8])                             # +inf * y = +inf
            else:
                y[r] = x[r] + 0.25 * y[r]                                   # cos > 0: the dissimilar branch is active
        up = torch.rand((FORM_N, D if kind in ('mse', 'l1') else 1), generator=g) + 0.5
        return {'x': x.to(dtype), 'y': y, 'up': up.squeeze(1) if kind.startswith('cos') else up,
                'labels': torch.tensor(FORM_LABELS)}
    return make


def _form_oracle(kind, kappa=1.0):
    def oracle(inp):
        x, y = inp['x'].clone().requires_grad_(True), inp['y']
        if kind == 'mse':
            out = (x - y) ** 2
        elif kind == 'l1':
            out = (x - y).abs()
        elif kind == 'vonmises':
            out = 1 - torch.exp(kappa * ((x * y).sum(dim=1, keepdim=True) - 1))
        else:
            labels = inp['labels'] if kind == 'cos-labelled' else torch.ones(FORM_N, dtype=torch.float64)
            out = F.cosine_embedding_loss(x, y, labels, reduction='none')
        grad, = torch.autograd.grad(out, x, inp['up'])
        return {'out': out.detach(), 'grad': grad}
    return oracle


class FormCase:
    def __init__(self, ident, kind, D, seed, **info):
        self.id, self.kind, self.D, self.info = ident, kind, D, info
        self.make, self.oracle = _form_make(kind, D, seed), _form_oracle(kind, info.get('kappa', 1.0))

    def __repr__(self):
        return self.id

    def index(self, r, poison):
        """the poisoned element of row r: L1 takes the element whose clean sign an infinity changes"""
        col = 1 if (self.kind == 'l1' and poison == '-inf') else 0
        return r * self.D + col

    def neg_inf_finite(self):
        return self.kind == 'vonmises'


def form_cases():
    return [FormCase('elementwise_none-mse', 'mse', 5, 800), FormCase('elementwise_none-l1', 'l1', 5, 801),
            FormCase('cosine_embedding_rows', 'cos', 70, 802), FormCase('cosine_embedding_rows-labelled', 'cos-labelled', 70, 803),
            FormCase('vonmises_rows-k1', 'vonmises', 2, 804, kappa=1.0), FormCase('vonmises_rows-k4', 'vonmises', 2, 805, kappa=4.0)]


FORM_TOL = {F32: 1e-6, BF16: 1e-6, F16: 1e-6}   # absolute; the rounding of a 16-bit gradient is assert_touched_finite's own term


def run_form(case, dtype, device_fn=None, poisons=POISONS):
    clean = case.make(dtype)
    want_clean = case.oracle(to64(clean))
    got_clean = device_fn(case, clean) if device_fn else None
    runs = 0
    for r in FORM_ROWS:
        row = torch.zeros((FORM_N, case.D), dtype=torch.bool)
        row[r] = True
        for pname, value in poisons.items():
            tag = (case.id, str(dtype), r, pname)
            inputs = place(clean, 'x', case.index(r, pname), value)
            want = case.oracle(to64(inputs))
            masks = {k: touched(want_clean[k], want[k]) for k in want}
            out_row = row[:, :want['out'].shape[1]] if want['out'].ndim == 2 else row[:, 0]
            assert bool(masks['out'].any()) and not bool(masks['out'][~out_row].any()), (tag, 'output rows')
            assert bool(masks['grad'].any()) and not bool(masks['grad'][~row].any()), (tag, 'gradient rows')
            finite = bool(torch.isfinite(want['out']).all())
            assert finite == (pname == '-inf' and case.neg_inf_finite()), (tag, 'the poison must show in the output')
            runs += 1
            if device_fn is None:
                continue
            got = device_fn(case, inputs)
            for k in want:
                assert tuple(got[k].shape) == tuple(want[k].shape), (tag, k)
                rounded = want[k].to(got[k].dtype).double()
                assert_class(got[k], rounded, masks[k], False, tag + (k,))
                assert_contained(got[k], got_clean[k], masks[k], tag + (k,))
                assert_touched_finite(got[k], want[k], masks[k], FORM_TOL[dtype], tag + (k,))
    return runs
