"""Writes tests/golden/block.npz: the reference's unmodified `model/block.py` (with its `activation.py`,
`normalization.py`, `utils.py`), loaded through `oracle.ref_loader`, run on the CPU in float32 for the three
blocks, ReLU and SiLU, train and eval mode, with and without a `downsample` (the reference's `ConvNormAct`,
1x1, stride 2, no activation), and for NonBottleneck1D with dropout_p 0 and 0.2 under a fixed seed, on the
seeded inputs of `testing.block_cases`.

A record (see `block_cases.GoldenFile`) holds x, gy (the fixed upstream gradient), y, gx (the gradient of
sum(y * gy) w.r.t. x), the state dict before the step and its buffers (running statistics,
num_batches_tracked) after it, the parameter gradients and, where Dropout2d drew, its scale [B, C] (checked against
what the reference's dropout module did to its input).  The file holds data only; arrays that several
records hold are stored once.

The tool also checks what the GPU tier relies on: in every record the float64 restatement of
`testing.block_ref` keeps every ReLU's |z| above 64 times the bound of its segment's forward arithmetic and
above the bound accumulated from the block's input (no gate can flip), and the reference's float32 lies
within the restatement's bounds.

Usage: python tools/gen_golden_block.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd.testing import block_cases as bc      # noqa: E402
from nicr_mt_scene_analysis_amd.testing import block_ref as R         # noqa: E402
from oracle import ref_loader                                          # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'block.npz')
DROPOUT_SEED = bc.DROPOUT_SEED


def load_reference_module():
    ref_loader.load_reference()
    for mod in ('activation', 'normalization', 'utils'):
        ref_loader._load(f'model.{mod}', f'model/{mod}.py')
    return ref_loader._load('model.block', 'model/block.py')


def main():
    ref = load_reference_module()
    act_mod = sys.modules[f'{ref_loader.PKG}.model.activation']
    utils_mod = sys.modules[f'{ref_loader.PKG}.model.utils']
    assert tuple(ref.KNOWN_BLOCKS) == bc.NAMES, ref.KNOWN_BLOCKS
    arrays, index, layouts = {}, {}, {}

    def put(t):
        a = np.ascontiguousarray(t.detach().numpy().astype(np.float32))
        key = 'a' + hashlib.sha256(a.tobytes() + str(a.shape).encode()).hexdigest()[:12]
        arrays[key] = a
        return key

    def flat(tensors, layout):
        return torch.cat([tensors[key].detach().float().reshape(-1) for key, _ in layout])

    worst_margin, worst_ratio = float('inf'), 0.0
    for name, act, mode, ds, p in bc.golden_records():
        inplanes, planes, stride = bc.golden_channels(name, ds)
        seed = bc.golden_seed(name, act, ds)
        torch.manual_seed(seed)
        down = utils_mod.ConvNormAct(inplanes, planes * bc.EXPANSION[name], kernel_size=1, stride=stride,
                                     activation=None) if ds else None
        kwargs = {} if p is None else {'dropout_p': p}
        module = ref.get_block_class(name)(inplanes, planes, stride=stride, downsample=down,
                                           activation=act_mod.get_activation_class(act), **kwargs)
        assert module.expansion == bc.EXPANSION[name]
        bc.randomise_running_stats(module, seed + 1)
        module.train(mode == 'train')
        before = {k: v.clone() for k, v in module.state_dict().items()}
        x = bc.golden_input(name, ds).requires_grad_(True)
        seen = []
        if p:
            module.dropout.register_forward_hook(lambda m, i, o: seen.append((i[0].detach().clone(), o.detach().clone())))
        torch.manual_seed(DROPOUT_SEED)
        y = module(x)
        gy = bc.golden_gy(y.shape, name, ds)
        (y * gy).sum().backward()
        rec = {'x': put(x), 'gy': put(gy), 'y': put(y), 'gx': put(x.grad)}
        scale = None
        if p and mode == 'train':
            torch.manual_seed(DROPOUT_SEED)
            scale = x.new_empty((x.shape[0], planes, 1, 1)).bernoulli_(1 - p).div_(1 - p)
            assert len(seen) == 1 and torch.equal(seen[0][1], seen[0][0] * scale), 'the dropout scale is not ATen\'s'
            scale = scale.reshape(x.shape[0], planes)
            rec['scale'] = put(scale)
        after = module.state_dict()
        params = dict(module.named_parameters())
        lkey = f"{name}/{'ds' if ds else 'id'}"
        layout = {'state': [[k, list(v.shape)] for k, v in before.items()],
                  'after': [[k, list(v.shape)] for k, v in before.items() if k not in params],
                  'grad': [[k, list(v.shape)] for k, v in params.items()]}
        assert layouts.setdefault(lkey, layout) == layout
        rec['state'] = put(flat(before, layout['state']))
        rec['state_after'] = put(flat(after, layout['after']))
        rec['grad'] = put(flat({k: v.grad for k, v in params.items()}, layout['grad']))
        rname = bc.record_name(name, act, mode, ds, p)
        index[rname] = rec
        # what the tests rely on
        want = R.block_reference(name, before, x.detach(), gy, act, mode == 'train', stride=stride, scale=scale)
        for what, margin, acc in want['margins']:
            worst_margin = min(worst_margin, margin)
            assert margin > 1.0 and acc > 1.0, (rname, what, margin, acc)
        got = {'y': y, 'gx': x.grad}
        got.update({f'grad/{k}': v.grad for k, v in params.items()})
        got.update({f'state/{k}': v for k, v in after.items() if 'running' in k})
        for key, t in got.items():
            r = R.worst_ratio(t, want[key])
            worst_ratio = max(worst_ratio, r)
            assert r <= 1.0, (rname, key, r)
    meta = {'records': index, 'layouts': layouts}
    arrays['index'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **arrays)
    print(f'{OUT}: {len(index)} records, {len(arrays) - 1} arrays, {os.path.getsize(OUT)} bytes; '
          f'smallest ReLU margin {worst_margin:.1f}, largest error / bound of the reference {worst_ratio:.3f}')


if __name__ == '__main__':
    main()
