"""Writes tests/golden/encoder_fusion.npz: the reference's unmodified `model/encoder_fusion.py` (with its
`activation.py`, `normalization.py`, `utils.py`), loaded through `oracle.ref_loader`, run on the CPU in
float32 for all seven fusion names, ReLU and SiLU, at the two shapes of
`testing.encoder_fusion_cases.GOLDEN_SHAPES` on the seeded inputs of `golden_inputs`.

A record `<name>/<act>/<shape index>` holds (see `encoder_fusion_cases.GoldenFile`):
  x_rgb, x_depth        the inputs
  gy_rgb, gy_depth      the fixed upstream gradients of the two outputs
  y_rgb, y_depth        the outputs
  gx_rgb, gx_depth      the gradients of sum(y_rgb * gy_rgb) + sum(y_depth * gy_depth) w.r.t. the inputs
                        ('none' and the far side of a one-way fusion included: the handed-through part)
  state                 the module's state dict, flattened in the order of `layouts` (the 'se-add*' names;
                        seeded default initialisation, the same parameters for the three names of a
                        shape and an activation)
  grad                  the gradients of those parameters, flattened alike
The file holds data only; arrays that several records hold are stored once.

Usage: python tools/gen_golden_encoder_fusion.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd.testing import encoder_fusion_cases as ec    # noqa: E402
from oracle import ref_loader                                                 # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'encoder_fusion.npz')


def load_reference_module():
    ref_loader.load_reference()
    for mod in ('activation', 'normalization', 'utils'):
        ref_loader._load(f'model.{mod}', f'model/{mod}.py')
    return ref_loader._load('model.encoder_fusion', 'model/encoder_fusion.py')


def main():
    ref = load_reference_module()
    act_mod = sys.modules[f'{ref_loader.PKG}.model.activation']
    assert tuple(ref.KNOWN_ENCODER_FUSIONS) == ec.NAMES, ref.KNOWN_ENCODER_FUSIONS
    arrays, index, layouts = {}, {}, {}

    def put(t):
        a = np.ascontiguousarray(t.detach().numpy().astype(np.float32))
        key = 'a' + hashlib.sha256(a.tobytes() + str(a.shape).encode()).hexdigest()[:12]
        arrays[key] = a
        return key

    for name, act, k in ec.golden_records():
        C = ec.GOLDEN_SHAPES[k][1]
        inp = ec.golden_inputs(k)
        torch.manual_seed(4200 + 10 * k + ec.ACTS.index(act))
        module = ref.get_encoder_fusion_class(name)(
            n_channels_in=C, input_memory_layout='nchw', activation=act_mod.get_activation_class(act))
        assert (module._use_se_weighting, tuple(module._destinations)) == ec.EXPECTED[name], name
        x = {m: inp[f'x_{m}'].clone().requires_grad_(True) for m in ('rgb', 'depth')}
        y = module(x)
        loss = (y['rgb'] * inp['gy_rgb']).sum() + (y['depth'] * inp['gy_depth']).sum()
        loss.backward()
        rec = {field: put(t) for field, t in inp.items()}
        for m in ('rgb', 'depth'):
            rec[f'y_{m}'] = put(y[m])
            rec[f'gx_{m}'] = put(x[m].grad)
        state = module.state_dict()
        if state:
            layout = [[key, list(p.shape)] for key, p in state.items()]
            assert layouts.setdefault(str(C), layout) == layout
            grads = dict(module.named_parameters())
            rec['state'] = put(torch.cat([state[key].reshape(-1) for key, _ in layout]))
            rec['grad'] = put(torch.cat([grads[key].grad.reshape(-1) for key, _ in layout]))
        index[ec.record_name(name, act, k)] = rec
    meta = {'records': index, 'layouts': layouts}
    arrays['index'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **arrays)
    print(f'{OUT}: {len(index)} records, {len(arrays) - 1} arrays, {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    main()
