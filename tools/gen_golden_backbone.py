"""Writes tests/golden/backbone.npz: the reference's unmodified `model/backbone/base.py`,
`model/backbone/resnet.py` and `model/encoder.py` (with its `activation.py`, `normalization.py`, `utils.py`,
`block.py`, `encoder_fusion.py`), loaded file by file through `oracle.ref_loader`, run on the CPU in float32 on
the configurations of `testing.backbone_cases`: batch 2, 3x64x64 rgb and 1x64x64 depth, layers [1, 1, 1, 1]
through the class constructors.  The reference's `backbone/__init__.py` is NOT loaded: it imports torchvision.

A record holds digests (see `backbone_cases.digest`) of every stage output or of the encoder's outputs and
skips, of gx for the fixed upstream gradient and of the gradient of conv1.weight, the gradients and the running
statistics of norm1 after the step, the state-dict key list and the sha256 of the filled state.  The file
holds data only; arrays that several records hold are stored once.

Usage: python tools/gen_golden_backbone.py
"""
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd.testing import backbone_cases as BC    # noqa: E402
from oracle import ref_loader                                          # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'backbone.npz')


def load_reference_namespace() -> SimpleNamespace:
    ref_loader.load_reference()
    for mod in ('activation', 'normalization', 'utils', 'block', 'encoder_fusion'):
        ref_loader._load(f'model.{mod}', f'model/{mod}.py')
    pkg = f'{ref_loader.PKG}.model.backbone'
    ref_loader._stub_package(pkg, os.path.join(ref_loader.REF_ROOT, 'model', 'backbone'))
    setattr(sys.modules[f'{ref_loader.PKG}.model'], 'backbone', sys.modules[pkg])
    ref_loader._load('model.backbone.base', 'model/backbone/base.py')
    resnet = ref_loader._load('model.backbone.resnet', 'model/backbone/resnet.py')
    encoder = ref_loader._load('model.encoder', 'model/encoder.py')
    block = sys.modules[f'{ref_loader.PKG}.model.block']
    fusion = sys.modules[f'{ref_loader.PKG}.model.encoder_fusion']
    assert 'torchvision' not in sys.modules
    return SimpleNamespace(ResNetBackbone=resnet.ResNetBackbone, ResNetSEBackbone=resnet.ResNetSEBackbone,
                           get_block_class=block.get_block_class, Encoder=encoder.Encoder,
                           FusedRGBDEncoder=encoder.FusedRGBDEncoder,
                           get_encoder_fusion_class=fusion.get_encoder_fusion_class)


def main():
    ns = load_reference_namespace()
    arrays, index = {}, {}

    def put(t):
        a = np.ascontiguousarray(t.numpy().astype(np.float32))
        key = 'a' + hashlib.sha256(a.tobytes() + str(a.shape).encode()).hexdigest()[:12]
        arrays[key] = a
        return key

    for config, mode in BC.records():
        module, sha = BC.build(config, ns)
        got = BC.run(config, mode, module)
        assert all(torch.isfinite(t).all() for t in got.values()), (config, mode)
        name = BC.record_name(config, mode)
        index[name] = {'sha256': sha, 'keys': list(module.state_dict()),
                       'shapes': {f: list(t.shape) for f, t in got.items()},
                       'fields': {f: put(BC.digest(t, f)) for f, t in got.items()}}
    arrays['index'] = np.frombuffer(json.dumps(index).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **arrays)
    print(f'{OUT}: {len(index)} records, {len(arrays) - 1} arrays, {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main()
