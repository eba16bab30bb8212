"""TEST INFRASTRUCTURE — never imported by the product path.

One RGB-D network assembled from the package's own classes, one training step of it, and the same step with every
model node and every loss as plain torch (`plain_composition`): the cases of tests/test_network_host.py (CPU) and
tests/test_network.py (GPU), which pin what no single node's test can see: the fused nodes handing tensors to each
other, sharing workspaces, running statistics and the random generator over a whole step and over several.

The network.  `FusedRGBDEncoder` of two ResNet backbones (`backbone_cases._backbone`, LAYERS 1-1-1-1, fusion
'se-add': ONE fused tensor under both keys), `get_context_module`, and `SemanticMLPDecoder`,
`InstanceMLPDecoder(with_orientation=True)`, `NormalMLPDecoder` with encoder-decoder fusion 'select-rgb', skips
(4, 8, 16), non-learned branch upsampling and a learned head `prediction_upsampling`.

    config   blocks            activation           context module   branch / context upsampling   head upsampling
    A        basicblock        relu (in place)      ppm              bilinear                      learned-3x3
    B        nonbottleneck1d   silu                 appm-1-2-4-8     nearest                       learned-3x3-zeropad

The cases (B, (H, W)): (2, (96, 128)), (2, (64, 160)), (1, (64, 160)).  H and W are multiples of 32: the MLP
decoders' factors 8, 4, 2, 1 are powers of two and the fused concatenation is taken.  The B = 1 case is config B
with the APPM built for a (1, 2) map, so that its pools at 2 x 5 are (2, 3) .. (16, 24) and no branch normalises
over one value.

The routes, float32, `block.FUSED_MIN_ELEMENTS` = 1 (`routes`, printed by the GPU tier once per case):
    batch-norm tail   vector at every plane of (96, 128) (3072 elements = 2 segments, the second partial; 768, 192,
                      48, 12: one) and at (64, 160) from 2560 (2 segments) down to 40; ELEMENT at the last stage of
                      (64, 160): 2 x 5 = 10 elements
    stem max pool     vector at both shapes
    SE-weighted add   vector | block at 3072 / 2560 elements, vector | wave below, element | wave at 10
    pyramid pool      LDS
    MLP concat        vector (W / 4 = 32 and 40 pixels)
    learned upsample  vector
"""
import collections
import contextlib
import hashlib

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import backbone_cases as BC
from . import block_cases
from . import context_ref
from . import mlp_decoder_ref
from . import synthetic as syn
from . import upsampling_ref

N_CLASSES = 9
IS_THING = (False,) * 4 + (True,) * 5
CONTEXT_CHANNELS = 128
DECODER_CHANNELS = (32, 32, 32, 32)
STATS_SEED = 6100
KAPPA = 1.0

# name: (block, activation name (None: the package default, an in-place ReLU), context module, branch / context
# upsampling, head upsampling)
CONFIGS = {
    'A': ('basicblock', None, 'ppm', 'bilinear', 'learned-3x3'),
    'B': ('nonbottleneck1d', 'silu', 'appm-1-2-4-8', 'nearest', 'learned-3x3-zeropad'),
}
SHAPES = ((96, 128), (64, 160))
B1_CASE = ('B', 1, (64, 160))           # the dense-view accumulation: g[:, :C] of a B = 1 gradient is contiguous

# Input seeds, chosen on the CPU (`find_input_seed`): in the float64 oracle no stem max-pool window has its two
# largest values closer than MARGIN x the float32 rounding of the larger.  Key: (config, B, (H, W), mode).
MARGIN = 64.0
INPUT_SEEDS = {('A', 2, (96, 128), 'train'): 1, ('A', 2, (96, 128), 'eval'): 1, ('A', 2, (64, 160), 'train'): 0,
               ('A', 2, (64, 160), 'eval'): 3, ('B', 2, (96, 128), 'train'): 0, ('B', 2, (96, 128), 'eval'): 1,
               ('B', 2, (64, 160), 'train'): 0, ('B', 2, (64, 160), 'eval'): 0, ('B', 1, (64, 160), 'train'): 1}
B1_APPM_INPUT_SIZE = (1, 2)

FUSED_NODES = {
    'pool': 'MaxPool3x3S2FunctionBackward', 'tail': 'BatchNormTailFunctionBackward',
    'se': 'SEWeightedAddFunctionBackward', 'ppm_pool': 'PyramidPoolFunctionBackward',
    'ppm_upcat': 'UpsampleConcatFunctionBackward', 'mlp_upcat': 'MlpUpsampleConcatFunctionBackward',
    'learned_up': 'LearnedUpsamplingFunctionBackward', 'losses': 'MultiLossFunctionBackward',
}


# ---------------------------------------------------------------------------- the network
class Network(nn.Module):
    def __init__(self, encoder, context, decoders):
        super().__init__()
        self.encoder, self.context, self.decoders = encoder, context, nn.ModuleDict(decoders)


def state_sha256(module: nn.Module) -> str:
    digest = hashlib.sha256()
    for name, t in module.state_dict().items():
        digest.update(name.encode())
        digest.update(t.detach().cpu().double().numpy().tobytes())
    return digest.hexdigest()


def build(config: str, hw=SHAPES[0], dropout: bool = False, appm_input_size=None):
    """the float32 CPU network of a configuration for inputs of `hw`, parameters filled
    (`backbone_cases.fill_parameters`), running statistics randomised (`block_cases.randomise_running_stats`)
    -> (network, sha256 of its state).  `dropout`: 0.2 in the blocks and 0.1 in the decoders instead of 0.
    `appm_input_size`: the map the context module is built for (default: the encoder's output for `hw`)."""
    from .. import model
    from ..model.activation import get_activation_class
    block, act_name, context, up, head_up = CONFIGS[config]
    act = None if act_name is None else get_activation_class(act_name)
    extra = {} if act is None else {'activation': act}
    ns = BC.package_namespace()
    p_block = 0.2 if dropout else 0.0
    encoder = model.FusedRGBDEncoder(BC._backbone(ns, block, False, False, 3, act, p_block),
                                     BC._backbone(ns, block, False, False, 1, act, p_block),
                                     fusion=model.get_encoder_fusion_class('se-add'), skip_downsamplings=BC.SKIPS,
                                     **extra)
    size = appm_input_size or (hw[0] // encoder.downsampling, hw[1] // encoder.downsampling)
    ctx = model.get_context_module(context, n_channels_in=encoder.n_channels_out, n_channels_out=CONTEXT_CHANNELS,
                                   input_size=size, activation=act_name or 'relu', upsampling=up)
    common = dict(n_channels_in=CONTEXT_CHANNELS, downsampling_in=encoder.downsampling, n_channels=DECODER_CHANNELS,
                  fusion=model.get_encoder_decoder_fusion_class('select-rgb'),
                  fusion_n_channels=tuple(reversed(encoder.skips_n_channels)),
                  fusion_downsamplings=tuple(reversed(BC.SKIPS)), dropout_p=0.1 if dropout else 0.0,
                  upsampling=model.get_upsampling_class(up), prediction_upsampling=model.get_upsampling_class(head_up),
                  **extra)
    decoders = {'semantic': model.SemanticMLPDecoder(n_classes=N_CLASSES, **common),
                'instance': model.InstanceMLPDecoder(with_orientation=True, **common),
                'normal': model.NormalMLPDecoder(**common)}
    net = Network(encoder, ctx, decoders)
    BC.fill_parameters(net)
    block_cases.randomise_running_stats(net, STATS_SEED)
    return net, state_sha256(net)


def snapshot(net: nn.Module) -> dict:
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def restore(net: nn.Module, state: dict) -> None:
    """in place: the tensors of a captured graph stay the network's"""
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(state[k])


# ---------------------------------------------------------------------------- batches
def input_seed(config: str, B: int, hw, mode: str = 'train') -> int:
    return INPUT_SEEDS[(config, B, tuple(hw), mode)]


def make_batch(B: int, hw, seed: int, device=None, dtype=torch.float32) -> dict:
    """seeded inputs ('rgb', 'depth': multiples of 1/8 in about -3..3) and the targets of the three tasks from the
    generators of testing/synthetic.py; float tensors in `dtype`"""
    H, W = hw
    gen = torch.Generator().manual_seed(BC._seed('network', seed))
    out = {'rgb': torch.round(torch.randn((B, 3, H, W), generator=gen) * 8) / 8,
           'depth': torch.round(torch.randn((B, 1, H, W), generator=gen) * 8) / 8}
    d = syn.make_loss_inputs(B, N_CLASSES, H, W, seed=seed)
    for key, name in (('semantic', 'semantic_target'), ('instance_center', 'center_target'),
                      ('instance_center_mask', 'center_mask'), ('instance_offset', 'offset_target'),
                      ('instance_foreground', 'offset_mask'), ('orientation', 'orientation_target'),
                      ('orientation_foreground', 'orientation_mask')):
        out[key] = torch.from_numpy(np.ascontiguousarray(d[name]))
    out['normal'] = torch.from_numpy(syn._normal_target(np.random.default_rng(seed + 7000), B, H, W, False))
    return {k: v.to(device=device, dtype=dtype if v.is_floating_point() else v.dtype) for k, v in out.items()}


# ---------------------------------------------------------------------------- the losses
def fused_helpers(device) -> dict:
    """the package's task helpers: every loss of a task in one multi-loss call"""
    from .. import task_helper as T
    helpers = {'semantic': T.SemanticTaskHelper(n_classes=N_CLASSES),
               'instance': T.InstanceTaskHelper(semantic_n_classes=N_CLASSES, semantic_classes_is_thing=IS_THING),
               'normal': T.NormalTaskHelper('mse')}
    for h in helpers.values():
        h.initialize(torch.device(device))
    return helpers


class _PlainHelper:
    def __init__(self, losses):
        self._losses = losses

    def training_step(self, batch, batch_idx, post):
        return self._losses(batch, post), {}


def _plain_semantic(batch, post):
    """cross entropy with label 0 as void: the sum over the non-void pixels by their number"""
    x, t = post['semantic_output'], batch['semantic']
    loss = F.cross_entropy(x, t.long() - 1, ignore_index=-1, reduction='sum') / (t > 0).sum()
    return {'semantic_loss_main': loss, 'semantic_total_loss': loss}


def _plain_instance(batch, post):
    """center: masked MSE; offset: masked L1, the mean over the two channels; orientation: von Mises over the
    masked pixels by max(count, 1)"""
    center, offset, orientation = post['instance_output']
    dt = center.dtype
    m = batch['instance_center_mask'].to(dt)
    lc = ((center[:, 0] * m - batch['instance_center'].to(dt)) ** 2).sum() / m.sum()
    m = batch['instance_foreground'].to(dt)
    lo = (offset * m[:, None] - batch['instance_offset'].to(dt)).abs().mean(1).sum() / m.sum()
    m = batch['orientation_foreground'].to(dt)
    dot = (orientation * batch['orientation'].to(dt)).sum(1)
    lv = ((1 - torch.exp(KAPPA * (dot - 1))) * m).sum() / m.sum().clamp(min=1)
    out = {}
    for name, value in (('center', lc), ('offset', lo), ('orientation', lv)):
        out[f'instance_{name}_loss_main'] = value
    for name, value in (('center', lc), ('offset', lo), ('orientation', lv)):
        out[f'instance_{name}_total_loss'] = value
    return out


def _plain_normal(batch, post):
    """masked MSE over the pixels with a ground-truth normal (not all three channels zero), the mean over channels"""
    x, t = post['normal_output'], batch['normal'].to(post['normal_output'].dtype)
    m = (~(t == 0).all(1)).to(x.dtype)
    loss = ((x * m[:, None] - t) ** 2).mean(1).sum() / m.sum()
    return {'normal_loss_main': loss, 'normal_total_loss': loss}


def plain_helpers() -> dict:
    """the same losses as plain torch expressions (the formulas tests/test_task_helpers.py takes as its oracle)"""
    return {'semantic': _PlainHelper(_plain_semantic), 'instance': _PlainHelper(_plain_instance),
            'normal': _PlainHelper(_plain_normal)}


# ---------------------------------------------------------------------------- one step
def forward(net: Network, inputs: dict, batch: dict):
    """encoder, context module, decoders, `is_training=True` postprocessing -> (features, skips, raw, post)"""
    feats, skips = net.encoder(dict(inputs))
    ctx = net.context(feats['rgb'])
    raw, post = {}, {}
    for task, decoder in net.decoders.items():
        raw[task] = decoder(ctx, skips, batch, do_postprocessing=False)
        post[task] = decoder.postprocessing.postprocess(raw[task], batch, is_training=True)
    return feats, skips, raw, post


def step(net: Network, batch: dict, helpers: dict, zero_grad: bool = True, nodes=None, prepare=None) -> dict:
    """One training step in the network's current mode: forward, the three helpers' training steps, backward of
    the sum of their totals.  -> flat dict: `loss/<key>`, `raw/<task>[/<i>]`, `out/<key>`, `skip/<ds>/<key>`,
    `gx/<key>`, `grad/<parameter>`, `after/<buffer>`.  `nodes` (a Counter) receives the autograd node names of
    the step; `prepare(total)` is called before backward (hooks on the graph)."""
    if zero_grad:
        net.zero_grad(set_to_none=True)
    inputs = {k: batch[k] if batch[k].requires_grad else batch[k].detach().requires_grad_(True)
              for k in ('rgb', 'depth')}
    feats, skips, raw, post = forward(net, inputs, batch)
    out = {}
    total = 0
    for task, helper in helpers.items():
        losses, _ = helper.training_step(batch, 0, post[task])
        for key, value in losses.items():
            out[f'loss/{key}'] = value
            if key.endswith('_total_loss'):
                total = total + value
    for task, (main, _) in raw.items():
        if isinstance(main, tuple):
            out.update({f'raw/{task}/{i}': t for i, t in enumerate(main)})
        else:
            out[f'raw/{task}'] = main
    out.update({f'out/{k}': t for k, t in feats.items()})
    for ds, per_key in skips.items():
        out.update({f'skip/{ds}/{k}': t for k, t in per_key.items()})
    if nodes is not None:
        nodes.update(graph_node_counts(total))
    if prepare is not None:
        prepare(total)
    total.backward()
    out.update({f'gx/{k}': t.grad for k, t in inputs.items()})
    out.update({f'grad/{k}': torch.zeros_like(p) if p.grad is None else p.grad for k, p in net.named_parameters()})
    params = {k for k, _ in net.named_parameters()}
    out.update({f'after/{k}': v for k, v in net.state_dict().items() if k not in params})
    return {k: v.detach() for k, v in out.items()}


def copy_of(result: dict) -> dict:
    return {k: v.clone() for k, v in result.items()}


def field_class(field: str) -> str:
    """'grad' (gx, parameter gradients: 2-norm), 'loss', 'stat' (the buffers after the step) or 'map' (outputs,
    skips; parameters after an optimizer step): max-norm.  The statistics are a class of their own, held to their
    own, lower floor: the map floor is that of the decoders' unit-length outputs, and under it a wrong running
    variance would pass."""
    head = field.split('/')[0]
    return 'grad' if BC.is_gradient(field) else {'loss': 'loss', 'after': 'stat'}.get(head, 'map')


NULL_GRADIENT = 1e-6


def distances(got: dict, ref: dict) -> dict:
    """{field: `backbone_cases.distance`} of a step's dict from the oracle's; integer buffers must be equal.
    Null gradients: the bias of a convolution in front of a training-mode batch norm (the branch embeddings of
    the decoders in front of `fuse.norm`) has the gradient 0 analytically, what arrives is rounding noise, and
    |d|_2 / |ref|_2 says nothing.  A bias gradient whose oracle norm is below NULL_GRADIENT x the norm of its own
    convolution's weight gradient is measured against that weight gradient's norm instead."""
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    out = {}
    for field, r in ref.items():
        g = got[field]
        assert tuple(g.shape) == tuple(r.shape), field
        if not r.is_floating_point():
            assert torch.equal(g.cpu(), r.cpu()), field
            continue
        sibling = ref.get(field[:-len('bias')] + 'weight') if field.startswith('grad/') and field.endswith('.bias') \
            else None
        if sibling is not None and float(r.double().norm()) < NULL_GRADIENT * float(sibling.double().norm()):
            out[field] = float((g.double().cpu() - r.double().cpu()).norm() / sibling.double().norm())
        else:
            out[field] = BC.distance(g, r.cpu(), field)
    return out


def worst_distances(got: dict, ref: dict) -> dict:
    """{class: (largest distance, its field)}"""
    worst = {}
    for field, d in distances(got, ref).items():
        cls = field_class(field)
        if d > worst.get(cls, (-1.0, ''))[0]:
            worst[cls] = (d, field)
    return worst


# ---------------------------------------------------------------------------- the plain composition
def _plain_pyramid_forward(defect):
    def pyramid_forward(module, x, sizes):
        feats = tuple(f[1](p) for f, p in zip(module.features, context_ref.torch_pool(x, sizes)))
        ys = feats if defect != 'ppm_branch_grad' else (feats[0].detach(),) + feats[1:]
        return module.final_conv(context_ref.torch_upcat(x, ys, module._upsampling)), feats
    return pyramid_forward


def _plain_upsample_concat(upsamplings, embedded):
    return mlp_decoder_ref.torch_upcat(embedded, upsamplings[0]._mode)


def _plain_upsampling_forward(self, x):
    if not self._learned:
        return F.interpolate(x, scale_factor=self._scale_factor, mode=self._mode, align_corners=self._align_corners)
    return upsampling_ref.torch_formulation(x, self.conv.weight, self.conv.bias, self._zeropad)


def _se_forward_without_depth_weight(self, x):
    fused = self.weighting_rgb(x['rgb']) + x['depth']
    return {'rgb': fused, 'depth': fused}


def _batch_norm_biased(original):
    def batch_norm(input, running_mean, running_var, weight=None, bias=None, training=False, momentum=0.1,
                   eps=1e-5):
        if not training or running_var is None:
            return original(input, running_mean, running_var, weight, bias, training, momentum, eps)
        # (the real update goes to a copy: autograd keeps the tensor it was given)
        out = original(input, running_mean, running_var.clone(), weight, bias, training, momentum, eps)
        dims = [d for d in range(input.ndim) if d != 1]
        with torch.no_grad():
            running_var.mul_(1 - momentum).add_(momentum * input.detach().var(dims, unbiased=False))
        return out
    return batch_norm


DEFECTS = ('se_depth', 'ppm_branch_grad', 'biased_var')


@contextlib.contextmanager
def plain_composition(defect: str = None):
    """Inside, no code under test runs: `backbone_cases.fused_paths_off` (stem pool, batch-norm tails, SE fusion
    as their torch compositions), the context module through `context_ref.torch_pool` / `torch_upcat`, the MLP
    decoders' concatenation through `mlp_decoder_ref.torch_upcat`, the learned upsamplings through
    `upsampling_ref.torch_formulation`.  Runs on CPU tensors in float64 (the oracle) and on the device in
    float32 (the floor).  Use `plain_helpers()` for the losses.
    `defect`, a deliberately wrong composition (the host tier shows the end-to-end bound sees each):
      'se_depth'          the depth modality's SE weight left out
      'ppm_branch_grad'   the gradient of the first pyramid branch dropped
      'biased_var'        running_var updated with the biased batch variance"""
    assert defect is None or defect in DEFECTS
    from ..model import encoder_fusion, upsampling
    from ..model.context_module import appm, ppm
    from ..model.decoder import mlp_base
    fusion = encoder_fusion.EncoderRGBDFusionWeightedAdd
    saved = (ppm.pyramid_forward, appm.pyramid_forward, mlp_base.upsample_concat, upsampling.Upsampling.forward,
             fusion.forward, F.batch_norm)
    with BC.fused_paths_off():
        ppm.pyramid_forward = appm.pyramid_forward = _plain_pyramid_forward(defect)
        mlp_base.upsample_concat = _plain_upsample_concat
        upsampling.Upsampling.forward = _plain_upsampling_forward
        if defect == 'se_depth':
            fusion.forward = _se_forward_without_depth_weight
        if defect == 'biased_var':
            F.batch_norm = _batch_norm_biased(saved[5])
        try:
            yield
        finally:
            (ppm.pyramid_forward, appm.pyramid_forward, mlp_base.upsample_concat, upsampling.Upsampling.forward,
             fusion.forward, F.batch_norm) = saved


# ---------------------------------------------------------------------------- the graph
def graph_nodes(*outputs) -> list:
    """the autograd nodes below the outputs, each once"""
    seen, stack = {}, [t.grad_fn for t in outputs if t.grad_fn is not None]
    while stack:
        fn = stack.pop()
        if fn in seen:
            continue
        seen[fn] = None
        stack.extend(f for f, _ in fn.next_functions if f is not None)
    return list(seen)


def graph_node_counts(*outputs) -> collections.Counter:
    return collections.Counter(type(fn).__name__ for fn in graph_nodes(*outputs))


def expected_node_counts(net: Network) -> dict:
    """the fused nodes of one step, derived from the module tree: a tail per norm-to-activation segment of every
    block plus the stems; a pool per backbone; a fusion per stage; one pyramid pool and one concatenation; a
    concatenation per decoder; a learned upsampling per `Upsampling` of a head; one multi-loss call per task"""
    from ..model import block, upsampling
    tails = {block.BasicBlock: 2, block.Bottleneck: 3, block.NonBottleneck1D: 2}
    n_tail = n_pool = n_up = 0
    for bb in (net.encoder.backbone_rgb, net.encoder.backbone_depth):
        n_tail += 1 + sum(n for m in bb.modules() for cls, n in tails.items() if isinstance(m, cls))
        n_pool += 1
    for m in net.modules():
        n_up += isinstance(m, upsampling.Upsampling) and m._learned
    return {'pool': n_pool, 'tail': n_tail, 'se': len(net.encoder.fusions), 'ppm_pool': 1, 'ppm_upcat': 1,
            'mlp_upcat': len(net.decoders), 'learned_up': int(n_up), 'losses': len(net.decoders)}


def expected_torch_batch_norms(net: Network) -> int:
    """batch norms that stay torch nodes: the `downsample` branches of the blocks and every `ConvNormAct`"""
    from ..model.utils import ConvNormAct
    n = 0
    for name, m in net.named_modules():
        if isinstance(m, nn.BatchNorm2d):
            n += '.downsample.' in name
        n += isinstance(m, ConvNormAct) and hasattr(m, 'norm')
    return n


def torch_batch_norm_count(counts) -> int:
    return sum(v for k, v in counts.items() if 'BatchNorm' in k and k != FUSED_NODES['tail'])


# ---------------------------------------------------------------------------- the seed margin
def stem_pool_margin(net: Network, batch: dict) -> float:
    """Over the windows of the stem max pool (its input under 'se-add' is the fused stage-0 tensor, the same for
    both backbones): the smallest (largest - second largest) / (2^-24 |largest|).  Windows whose two largest
    values are both exactly 0 are left out: the ReLU clamped them, the selected position carries y = 0, and the
    stem tails' gates stop its gradient whichever position is selected.  The network's buffers are restored."""
    state = snapshot(net)
    with torch.no_grad():
        out = {'rgb': net.encoder.backbone_rgb.forward_stage(0, batch['rgb']),
               'depth': net.encoder.backbone_depth.forward_stage(0, batch['depth'])}
        x = net.encoder.fusions[0](out)['rgb'].double()
    restore(net, state)
    Bn, C, H, W = x.shape
    win = F.unfold(F.pad(x, (1, 1, 1, 1), value=float('-inf')), 3, stride=2).view(Bn, C, 9, -1)
    top = win.topk(2, dim=2).values
    first, second = top[:, :, 0], top[:, :, 1]
    keep = ~((first == 0) & (second == 0))
    ratio = (first - second) / (2.0 ** -24 * first.abs())
    return float(ratio[keep].min())


def find_input_seed(config: str, B: int, hw, mode: str, tries: int = 200, **build_kwargs) -> int:
    net, _ = build(config, hw, **build_kwargs)
    net.double().train(mode == 'train')
    with plain_composition():
        for seed in range(tries):
            if stem_pool_margin(net, make_batch(B, hw, seed, dtype=torch.float64)) >= MARGIN:
                return seed
    raise RuntimeError('no seed with the margin')


# ---------------------------------------------------------------------------- routes (device only)
def routes(net: Network, batch: dict) -> dict:
    """{node: sorted set of (plane or shape, route)} of one fused forward on the device, from the ops' route queries"""
    from .. import ops
    seen = collections.defaultdict(set)
    saved = {n: getattr(ops, n) for n in ('bntail_apply', 'maxpool3x3s2', 'sefuse_scale_add', 'ppm_pool',
                                          'mlpdec_upsample_concat', 'upsample2x_dw3x3')}

    def bntail_apply(x, *a, **k):
        seen['tail'].add((tuple(x.shape[2:]), ops.bntail_route(x)))
        return saved['bntail_apply'](x, *a, **k)

    def maxpool3x3s2(x, *a, **k):
        y, code = saved['maxpool3x3s2'](x, *a, **k)
        seen['pool'].add((tuple(x.shape[2:]), ops.maxpool3x3s2_route(x, y)))
        return y, code

    def sefuse_scale_add(x_rgb, x_depth, w, *a, **k):
        seen['se'].add((tuple(x_rgb.shape[2:]), ops.sefuse_route(x_rgb, x_depth)))
        return saved['sefuse_scale_add'](x_rgb, x_depth, w, *a, **k)

    def ppm_pool(x, sizes):
        seen['ppm_pool'].add((tuple(x.shape[2:]), tuple(sizes), ops.ppm_route(tuple(x.shape[2:]), sizes)))
        return saved['ppm_pool'](x, sizes)

    def mlpdec_upsample_concat(ys, mode='bilinear', size=None):
        out = saved['mlpdec_upsample_concat'](ys, mode, size)
        seen['mlp_upcat'].add((tuple(out.shape[2:]), ops.mlpdec_route(ys, out)))
        return out

    def upsample2x_dw3x3(x, *a, **k):
        y = saved['upsample2x_dw3x3'](x, *a, **k)
        seen['learned_up'].add((tuple(x.shape[1:]), ops.upsample2x_dw3x3_route(x, y)))
        return y

    local = dict(bntail_apply=bntail_apply, maxpool3x3s2=maxpool3x3s2, sefuse_scale_add=sefuse_scale_add,
                 ppm_pool=ppm_pool, mlpdec_upsample_concat=mlpdec_upsample_concat, upsample2x_dw3x3=upsample2x_dw3x3)
    state = snapshot(net)
    try:
        for n, f in local.items():
            setattr(ops, n, f)
        with torch.no_grad():
            forward(net, {k: batch[k] for k in ('rgb', 'depth')}, batch)
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
        restore(net, state)
    return {k: sorted(v) for k, v in seen.items()}


# ---------------------------------------------------------------------------- several steps
LR, MOMENTUM = 0.001, 0.9


def optimizer_steps(net: Network, batches, helpers: dict) -> list:
    """SGD with momentum, one step per batch -> per step {`param/<name>`, `after/<buffer>`} (copies)"""
    opt = torch.optim.SGD(net.parameters(), lr=LR, momentum=MOMENTUM)
    params = {k for k, _ in net.named_parameters()}
    out = []
    for batch in batches:
        step(net, batch, helpers)
        opt.step()
        out.append({('after/' if k not in params else 'param/') + k: v.detach().clone()
                    for k, v in net.state_dict().items()})
    return out


# ---------------------------------------------------------------------------- what the nodes are handed
def handover_census(table: dict):
    """-> `prepare` for `step`: backward pre-hooks on every fused node that count, per node class, in `table`
    [calls, calls with a non-contiguous incoming gradient, calls with an incoming gradient of another dtype than the
    node's first saved map (None: the node saves no map), calls with an incoming gradient that is a view, calls
    that RETURN a view as a gradient, calls that return a dense view (what autograd may accumulate into in place)]"""
    names = set(FUSED_NODES.values())

    def prepare(total):
        for fn in graph_nodes(total):
            name = type(fn).__name__
            if name not in names:
                continue
            saved = [t for t in getattr(fn, 'saved_tensors', ()) if t is not None and t.is_floating_point()
                     and t.ndim == 4]
            row = table.setdefault(name, [0, 0, 0 if saved else None, 0, 0, 0])

            def hook(grads, row=row, dtype=saved[0].dtype if saved else None):
                given = [g for g in grads if g is not None]
                row[0] += 1
                row[1] += any(not g.is_contiguous() for g in given)
                if dtype is not None:
                    row[2] += any(g.dtype != dtype for g in given)
                row[3] += any(g._base is not None for g in given)

            def after(grad_inputs, grad_outputs, row=row):
                views = [g for g in grad_inputs if g is not None and g._base is not None]
                row[4] += bool(views)
                row[5] += any(g.is_contiguous() for g in views)
            fn.register_prehook(hook)
            fn.register_hook(after)
    return prepare


# ---------------------------------------------------------------------------- which planes a dropout zeroes
@contextlib.contextmanager
def dropout_record(net: Network, events: list):
    """inside, `events` receives the all-zero (image, channel) planes of every Dropout2d draw of the network, in
    the order of the draws: forward hooks on the `nn.Dropout2d` modules (the plain composition's blocks, the
    decoders) and a wrapper of `block.dropout2d_scale` (the fused tails, which never call the module)"""
    from ..model import block
    original = block.dropout2d_scale

    def dropout2d_scale(x, p):
        scale = original(x, p)
        events.append((scale.flatten(1) == 0).nonzero().tolist())
        return scale

    def hook(module, args, out):
        if module.training and module.p > 0:
            events.append((out.flatten(2) == 0).all(2).nonzero().tolist())

    handles = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, nn.Dropout2d)]
    block.dropout2d_scale = dropout2d_scale
    try:
        yield
    finally:
        block.dropout2d_scale = original
        for h in handles:
            h.remove()


# ---------------------------------------------------------------------------- the measured floors
# The largest distance, per class, of the PLAIN composition on an MI355X in float32 from the float64 oracle
# (tools/network_floors.py; docs/measurement_log.md), over the cases of one step and per optimizer step, and over the
# runs of the tool: torch's convolutions do not repeat their bits from process to process, and the floor of a class
# moves by up to a factor of four between runs.  The fused network is held to FACTOR x these.  FLOOR_APART: records
# of config A held to their own measured floor; none was needed.
FACTOR = 4.0
FLOOR = {'map': 1.02e-2, 'grad': 1.53e-2, 'loss': 1.61e-6, 'stat': 2.55e-5}
FLOOR_APART = {}
FLOOR_STEPS = ({'map': 8.96e-6, 'stat': 2.58e-5}, {'map': 1.73e-5, 'stat': 3.21e-5}, {'map': 2.54e-5, 'stat': 5.31e-5})
FLOOR_STEPS_APART = {}


def case_name(config: str, B: int, hw, mode: str) -> str:
    return f'{config}/b{B}/{hw[0]}x{hw[1]}/{mode}'


def bound(name: str, cls: str) -> float:
    return FACTOR * FLOOR_APART.get((name, cls), FLOOR[cls])


def step_bound(name: str, idx: int, cls: str) -> float:
    return FACTOR * FLOOR_STEPS_APART.get((name, idx, cls), FLOOR_STEPS[idx][cls])
