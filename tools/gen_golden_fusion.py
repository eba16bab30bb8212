"""Writes tests/golden/encoder_decoder_fusion.npz: the reference's unmodified
`model/encoder_decoder_fusion.py` (with its `activation.py`, `normalization.py`, `utils.py`), loaded
through `oracle.ref_loader`, run on the CPU on the seeded cases of `testing.fusion_cases.FUSION_CASES`.

The fixture holds recorded results only, a few tens of KB.  The inputs are NOT stored: a SHA-256 of
their bytes is, and the tests regenerate them and fail on a mismatch.  Per case (`names`):
  <case>__params   JSON {fusion, n_enc, n_dec, shape, key, digest, grads}
  <case>__y        the module's output, float32 [B, n_dec, H, W] (training mode)
  <case>__gx_enc, __gx_dec   gradients of sum(y * gy) w.r.t. the encoder / decoder features (absent
                   where the output does not depend on them)
  <case>__g__<key> the gradient of every parameter, by state-dict key
  state            JSON {name: {"<n_enc>_<n_dec>": {state_dict key: shape}}} for all 19 names
  shapes           JSON {name: output shape} at FUSION_SHAPE_INPUT with 8 -> 8 channels

Usage: python tools/gen_golden_fusion.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd.testing import fusion_cases as fc      # noqa: E402
from oracle import ref_loader                                          # noqa: E402


def jdump(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def main():
    ref_loader.load_reference()
    for mod in ('activation', 'normalization', 'utils'):
        ref_loader._load(f'model.{mod}', f'model/{mod}.py')
    ref = ref_loader._load('model.encoder_decoder_fusion', 'model/encoder_decoder_fusion.py')
    out = {'names': jdump(list(fc.FUSION_CASES))}
    for name, (fusion, n_enc, n_dec, shape, _) in fc.FUSION_CASES.items():
        inp = fc.make_fusion_inputs(name)
        module = ref.get_encoder_decoder_fusion_class(fusion)(n_channels_encoder=n_enc, n_channels_decoder=n_dec)
        params = dict(module.named_parameters())
        assert list(params) == list(inp['params']), (name, list(params))
        with torch.no_grad():
            for key, value in inp['params'].items():
                params[key].copy_(torch.from_numpy(value))
        x_enc = torch.from_numpy(inp['x_enc']).requires_grad_(True)
        x_dec = torch.from_numpy(inp['x_dec']).requires_grad_(True)
        y = module({fc.fusion_key(fusion): x_enc}, x_dec)
        y.backward(torch.from_numpy(inp['gy']))
        grads = []
        out[f'{name}__y'] = y.detach().contiguous().numpy()
        for key, t in (('gx_enc', x_enc), ('gx_dec', x_dec)):
            if t.grad is not None:
                out[f'{name}__{key}'] = t.grad.contiguous().numpy()
                grads.append(key)
        for key, p in params.items():
            out[f'{name}__g__{key}'] = p.grad.numpy()
        out[f'{name}__params'] = jdump({'fusion': fusion, 'n_enc': n_enc, 'n_dec': n_dec, 'shape': list(shape),
                                        'key': fc.fusion_key(fusion), 'digest': fc.fusion_input_digest(inp),
                                        'grads': grads})
        print(name, tuple(y.shape), grads, list(params))
    state, shapes = {}, {}
    B, H, W = fc.FUSION_SHAPE_INPUT
    for fusion in ref.KNOWN_ENCODER_DECODER_FUSIONS:
        state[fusion] = {}
        for n_enc, n_dec in fc.FUSION_STATE_CHANNELS:
            module = ref.get_encoder_decoder_fusion_class(fusion)(n_channels_encoder=n_enc, n_channels_decoder=n_dec)
            state[fusion][f'{n_enc}_{n_dec}'] = {k: list(v.shape) for k, v in module.state_dict().items()}
        module = ref.get_encoder_decoder_fusion_class(fusion)(n_channels_encoder=8, n_channels_decoder=8)
        x_enc = torch.zeros((B, H, W, 8) if fusion.startswith('swin') else (B, 8, H, W))
        shapes[fusion] = list(module({fc.fusion_key(fusion): x_enc}, torch.zeros(B, 8, H, W)).shape)
    out['state'] = jdump(state)
    out['shapes'] = jdump(shapes)
    out['known'] = jdump(list(ref.KNOWN_ENCODER_DECODER_FUSIONS))
    path = os.path.join(ROOT, 'tests', 'golden', 'encoder_decoder_fusion.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
