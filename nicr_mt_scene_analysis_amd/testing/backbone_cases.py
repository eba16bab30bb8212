"""TEST INFRASTRUCTURE — never imported by the product path.

The configurations, the deterministic parameter fill and the fixture layout of the backbone and encoder tests,
shared by the host tier, the GPU tier and tools/gen_golden_backbone.py.  `build` and `run` take the classes
from a namespace, so the same code drives this package's modules and the reference's.

What a record holds.  The maps of a ResNet are far too large to commit whole (stage 0 of one record alone is
2 x 64 x 32 x 32 float32 = 512 KB), so every map is stored as a DIGEST: `SAMPLE` elements at seeded
positions (`sample_index`), and the per-channel mean and mean absolute value, summed in float64.  A digest of
a map that differs anywhere in a channel moves that channel's means; the samples pin single elements.  Small
tensors (the gradients and running statistics of norm1) are stored whole.  The weights are not stored at all:
`fill_parameters` regenerates them and the record holds the sha256 of the filled state."""
import contextlib
import hashlib
import json
from types import SimpleNamespace

import numpy as np
import torch

B, HW = 2, (64, 64)
LAYERS = [1, 1, 1, 1]
SAMPLE = 512
INPUT_SEED, GY_SEED, FILL_SEED = 5100, 5200, 5300
SKIPS = (4, 8, 16)
FUSION = 'se-add-uni-rgb'

# name: (kind, block, se, d16, n_input_channels)
CONFIGS = {
    'basicblock/plain': ('backbone', 'basicblock', False, False, 3),
    'basicblock/se': ('backbone', 'basicblock', True, False, 3),
    'nonbottleneck1d/plain': ('backbone', 'nonbottleneck1d', False, False, 3),
    'nonbottleneck1d/se': ('backbone', 'nonbottleneck1d', True, False, 3),
    'nonbottleneck1d/d16': ('backbone', 'nonbottleneck1d', False, True, 3),
    'encoder/depth': ('encoder', 'nonbottleneck1d', False, False, 1),
    'encoder/depth-d16': ('encoder', 'nonbottleneck1d', False, True, 1),
    'encoder/fused': ('fused', 'nonbottleneck1d', False, False, 3),
}
MODES = ('train', 'eval')


def records():
    """(config, mode): the four plain / SE backbones in both modes, everything else in training mode and the fused
    encoder in both"""
    out = []
    for config, (kind, _, _, d16, _) in CONFIGS.items():
        for mode in MODES:
            if mode == 'eval' and (d16 or kind == 'encoder'):
                continue
            out.append((config, mode))
    return out


def record_name(config: str, mode: str) -> str:
    return f'{config}/{mode}'


def _seed(*parts) -> int:
    return int.from_bytes(hashlib.sha256('/'.join(str(p) for p in parts).encode()).digest()[:7], 'little')


def golden_input(channels: int) -> torch.Tensor:
    """seeded float32 image batch, multiples of 1/8 in about -3..3: 3 channels rgb, 1 channel depth"""
    gen = torch.Generator().manual_seed(INPUT_SEED + channels)
    return torch.round(torch.randn((B, channels) + HW, generator=gen) * 8) / 8


def golden_gy(shape, tag: str) -> torch.Tensor:
    """the fixed upstream gradient of an output: multiples of 1/8"""
    gen = torch.Generator().manual_seed(_seed(GY_SEED, tag))
    return torch.round(torch.randn(tuple(shape), generator=gen) * 8) / 8


def fill_parameters(module: torch.nn.Module, seed: int = FILL_SEED) -> str:
    """A deterministic value for every state-dict entry, from a CPU generator seeded by `seed` and the entry's
    name: convolution weights normal with variance 2 / fan-in, norm weights about 1, biases and running means
    small, running variances in 0.5..1.5, counters 0.  Returns the sha256 of the filled state (names and
    float32 bytes in state-dict order)."""
    digest = hashlib.sha256()
    with torch.no_grad():
        for name, t in module.state_dict().items():
            gen = torch.Generator().manual_seed(_seed(seed, name))
            if name.endswith('num_batches_tracked'):
                v = torch.zeros(t.shape)
            elif t.ndim == 4:
                fan_in = t.shape[1] * t.shape[2] * t.shape[3]
                v = torch.randn(t.shape, generator=gen) * (2.0 / fan_in) ** 0.5
            elif name.endswith('running_var'):
                v = 0.5 + torch.rand(t.shape, generator=gen)
            elif name.endswith('running_mean'):
                v = 0.1 * torch.randn(t.shape, generator=gen)
            elif name.endswith('weight'):
                v = 1.0 + 0.1 * torch.randn(t.shape, generator=gen)
            else:
                v = 0.1 * torch.randn(t.shape, generator=gen)
            t.copy_(v.to(device=t.device, dtype=t.dtype))
            digest.update(name.encode())
            digest.update(v.float().numpy().tobytes())
    return digest.hexdigest()


def package_namespace() -> SimpleNamespace:
    """this package's classes, as `build` takes them"""
    from .. import model
    return SimpleNamespace(ResNetBackbone=model.ResNetBackbone, ResNetSEBackbone=model.ResNetSEBackbone,
                           get_block_class=model.get_block_class, Encoder=model.Encoder,
                           FusedRGBDEncoder=model.FusedRGBDEncoder,
                           get_encoder_fusion_class=model.get_encoder_fusion_class)


def _backbone(ns, block: str, se: bool, d16: bool, channels: int, activation=None, dropout_p: float = 0.0):
    """`activation` (a class; default: the package's) and `dropout_p` are for testing/network_cases.py"""
    cls = ns.ResNetSEBackbone if se else ns.ResNetBackbone
    kwargs = {'dropout_p': dropout_p} if block == 'nonbottleneck1d' else {}     # 0: no random draw in the records
    extra = {} if activation is None else {'activation': activation}
    return cls(block=ns.get_block_class(block, **kwargs), layers=list(LAYERS), n_input_channels=channels,
               replace_stride_with_dilation=[False, False, True] if d16 else None, **extra)


def build(config: str, ns=None):
    """the module of a configuration through the class constructors, parameters filled -> (module, sha256)"""
    ns = ns or package_namespace()
    kind, block, se, d16, channels = CONFIGS[config]
    if kind == 'backbone':
        module = _backbone(ns, block, se, d16, channels)
    elif kind == 'encoder':
        module = ns.Encoder(_backbone(ns, block, se, d16, channels), skip_downsamplings=SKIPS)
    else:
        module = ns.FusedRGBDEncoder(_backbone(ns, block, se, d16, 3), _backbone(ns, block, se, d16, 1),
                                     fusion=ns.get_encoder_fusion_class(FUSION), skip_downsamplings=SKIPS)
    return module, fill_parameters(module)


def stems(config: str):
    """state-dict prefixes of the backbones whose conv1 / norm1 the record follows"""
    return {'backbone': ('',), 'encoder': ('backbone.',), 'fused': ('backbone_rgb.', 'backbone_depth.')}[CONFIGS[config][0]]


def run(config: str, mode: str, module, device=None, nodes=None):
    """one step of `module` on the configuration's input -> dict of tensors (`nodes`, a set, receives the names of
    the autograd nodes of the step): `stage<i>` (backbones) or
    `out/<key>` and `skip/<ds>/<key>` (encoders), `gx[/<key>]`, `grad/<prefix>conv1.weight`,
    `grad/<prefix>norm1.weight|bias`, `after/<prefix>norm1.running_mean|running_var`"""
    kind = CONFIGS[config][0]
    module.train(mode == 'train')
    module.zero_grad(set_to_none=True)
    out = {}
    if kind == 'backbone':
        x = golden_input(3).to(device).requires_grad_(True)
        t = x
        for idx in range(len(module.stages)):
            t = module.forward_stage(idx, t)
            out[f'stage{idx}'] = t
        t.backward(golden_gy(t.shape, config).to(device))
        out['gx'] = x.grad
    else:
        keys = ('rgb', 'depth') if kind == 'fused' else ('depth',)
        inputs = {k: golden_input(3 if k == 'rgb' else 1).to(device).requires_grad_(True) for k in keys}
        given = dict(inputs)
        feats, skips = module(given)
        assert given.keys() == inputs.keys() and all(given[k] is inputs[k] for k in keys)
        loss = 0
        for k in sorted(feats):
            out[f'out/{k}'] = feats[k]
            if feats[k].requires_grad and feats[k] is not inputs.get(k):
                loss = loss + (feats[k] * golden_gy(feats[k].shape, f'{config}/{k}').to(device)).sum()
        for ds, per_key in skips.items():
            for k, t in per_key.items():
                out[f'skip/{ds}/{k}'] = t
        loss.backward()
        for k in keys:
            out[f'gx/{k}'] = inputs[k].grad
    state = module.state_dict()
    params = dict(module.named_parameters())
    for prefix in stems(config):
        for name in ('conv1.weight', 'norm1.weight', 'norm1.bias'):
            out[f'grad/{prefix}{name}'] = params[prefix + name].grad
        for name in ('norm1.running_mean', 'norm1.running_var'):
            out[f'after/{prefix}{name}'] = state[prefix + name]
    if nodes is not None:
        nodes.update(graph_node_names(*out.values()))
    return {k: v.detach() for k, v in out.items()}


# ---------------------------------------------------------------------------- comparisons on the device
@contextlib.contextmanager
def fused_paths_off():
    """inside: the stem pool, every batch-norm tail and the SE-weighted fusion take their torch compositions
    whatever the tensors are (the plain composition the noise floor and the benchmark baseline are measured on)"""
    from ..model import block, encoder_fusion, pooling
    saved = (block._fused_act, encoder_fusion.EncoderRGBDFusionWeightedAdd._fused_act,
             pooling.MaxPool2d.takes_hip_path)
    block._fused_act = lambda *a, **k: None
    encoder_fusion.EncoderRGBDFusionWeightedAdd._fused_act = lambda *a, **k: None
    pooling.MaxPool2d.takes_hip_path = lambda *a, **k: False
    try:
        yield
    finally:
        (block._fused_act, encoder_fusion.EncoderRGBDFusionWeightedAdd._fused_act,
         pooling.MaxPool2d.takes_hip_path) = saved


def is_gradient(field: str) -> bool:
    return field.split('/')[0] in ('gx', 'grad')


def distance(got: torch.Tensor, ref: torch.Tensor, field: str) -> float:
    """of two digests.  Maps and statistics: the largest difference over the largest reference magnitude.
    Gradients: |d|_2 / |ref|_2, because a ReLU gate or a pool tie within rounding of a flip moves single elements
    discretely."""
    got, ref = got.double().cpu(), ref.double()
    if is_gradient(field):
        return float((got - ref).norm() / ref.norm().clamp_min(1e-30))
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def graph_node_names(*outputs) -> set:
    """names of the autograd nodes below the outputs"""
    seen, names, stack = set(), set(), [t.grad_fn for t in outputs if t.grad_fn is not None]
    while stack:
        fn = stack.pop()
        if fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions if f is not None)
    return names


# ---------------------------------------------------------------------------- digests
WHOLE_BELOW = 1024                      # tensors up to this many elements are stored whole


def sample_index(numel: int, key: str) -> torch.Tensor:
    gen = torch.Generator().manual_seed(_seed('sample', key, numel))
    return torch.randperm(numel, generator=gen)[:SAMPLE].sort().values


def digest(t: torch.Tensor, key: str):
    """float32 [n] digest of a tensor: the tensor itself when small, else SAMPLE seeded elements followed by the
    per-channel (dim 1; dim 0 of a weight) means and mean absolute values from float64 sums"""
    t = t.detach().float().cpu()
    if t.numel() <= WHOLE_BELOW:
        return t.reshape(-1)
    d = t.double()
    ch = d.flatten(2).transpose(0, 1).flatten(1) if t.ndim == 4 and key.split('/')[0] != 'grad' else d.flatten(1)
    return torch.cat([t.reshape(-1)[sample_index(t.numel(), key)], ch.mean(1).float(), ch.abs().mean(1).float()])


class GoldenFile:
    """tests/golden/backbone.npz: `index` is JSON {record: {'sha256': .., 'keys': [state-dict keys],
    'shapes': {field: shape}, 'fields': {field: array key}}}; every array is the `digest` of the field's tensor;
    an array several records hold is stored once."""

    def __init__(self, path):
        self._npz = np.load(path)
        self.index = json.loads(bytes(self._npz['index']).decode())

    def record(self, name):
        meta = self.index[name]
        fields = {f: torch.from_numpy(self._npz[k].copy()) for f, k in meta['fields'].items()}
        return SimpleNamespace(sha256=meta['sha256'], keys=meta['keys'], fields=fields,
                               shapes={f: tuple(s) for f, s in meta['shapes'].items()})
