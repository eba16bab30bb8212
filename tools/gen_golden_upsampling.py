"""Writes tests/golden/upsampling.npz: the reference's unmodified `model/upsampling.py`, loaded
through `oracle.ref_loader`, run on the CPU on the seeded cases of
`testing.synthetic.UPSAMPLING_CASES`.

The fixture holds recorded results only, a few tens of KB.  The inputs are NOT stored: a SHA-256
of their bytes is, and the tests regenerate them and fail on a mismatch.  Per case (`names`):
  <case>__params   JSON {mode, use_bias, trained, shape, digest}
  <case>__y        the module's output, float32 [B,C,2h,2w]
  <case>__gx, __gw, __gb   gradients of sum(y * gy) w.r.t. the input, conv.weight and conv.bias
                   (__gb only with a bias)
  state            JSON {mode: {state_dict key: shape}} for the four mode names (4 channels)
  shapes           JSON {mode: output shape} for an input of UPSAMPLING_SHAPE_INPUT
Both learned modes, with and without bias, with trained (random) and initial weights.

Usage: python tools/gen_golden_upsampling.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd.testing import synthetic as syn      # noqa: E402
from oracle import ref_loader                                        # noqa: E402


def jdump(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def main():
    ref_loader.load_reference()
    ref = ref_loader._load('model.upsampling', 'model/upsampling.py')
    out = {'names': jdump(list(syn.UPSAMPLING_CASES))}
    for name, (mode, use_bias, trained, shape, _) in syn.UPSAMPLING_CASES.items():
        inp = syn.make_upsampling_inputs(name)
        module = ref.Upsampling(mode, n_channels=shape[1], use_bias=use_bias)
        with torch.no_grad():
            if inp['weight'] is not None:
                module.conv.weight.copy_(torch.from_numpy(inp['weight']))
            if inp['bias'] is not None:
                module.conv.bias.copy_(torch.from_numpy(inp['bias']))
        x = torch.from_numpy(inp['x']).requires_grad_(True)
        y = module(x)
        y.backward(torch.from_numpy(inp['gy']))
        out[f'{name}__params'] = jdump({'mode': mode, 'use_bias': use_bias, 'trained': trained,
                                        'shape': list(shape), 'digest': syn.upsampling_input_digest(inp)})
        out[f'{name}__y'] = y.detach().numpy()
        out[f'{name}__gx'] = x.grad.numpy()
        out[f'{name}__gw'] = module.conv.weight.grad.numpy()
        if use_bias:
            out[f'{name}__gb'] = module.conv.bias.grad.numpy()
        print(name, tuple(y.shape), float(y.detach().abs().max()))
    state, shapes = {}, {}
    probe = torch.zeros(syn.UPSAMPLING_SHAPE_INPUT)
    for mode in ref.KNOWN_UPSAMPLING_METHODS:
        module = ref.get_upsampling_class(mode)(n_channels=4)
        state[mode] = {k: list(v.shape) for k, v in module.state_dict().items()}
        shapes[mode] = list(ref.Upsampling(mode, n_channels=syn.UPSAMPLING_SHAPE_INPUT[1])(probe).shape)
    out['state'] = jdump(state)
    out['shapes'] = jdump(shapes)
    path = os.path.join(ROOT, 'tests', 'golden', 'upsampling.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
