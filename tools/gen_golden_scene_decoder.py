"""Writes tests/golden/scene_decoder.npz: the reference's unmodified `model/decoder/scene.py`
(`SceneClassificationDecoder`, with its `model/decoder/base.py`), loaded through `oracle.ref_loader`, run on the
CPU in float32 and once more as `.double()` on the seeded cases of `testing.scene_head_ref.SCENE_HEAD_CASES`.
The decoder is called with do_postprocessing=False (the reference's postprocessing factory is replaced by a
stand-in that is never called).

The fixture holds recorded results only.  The inputs are NOT stored: a SHA-256 of their bytes is, and the
tests regenerate them and fail on a mismatch.  Per case (`names`):
  <case>__params    JSON {digest, state: {state_dict key: shape}, dist: {logits, gx, gweight, gbias}}, dist the
                    largest distance of the float32 run from the float64 run of that quantity
  <case>__logits    the logits of the float64 run, float64 [B, K]
  <case>__gx        the gradient of sum(logits * g) w.r.t. the map the decoder pools (the first context feature,
                    or cm_output without context features), float64
  <case>__gweight   ... w.r.t. `_task_head.weight`, float64
  <case>__gbias     ... w.r.t. `_task_head.bias`, float64
  <case>__logits32  the logits of the float32 run

Usage: python tools/gen_golden_scene_decoder.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd.testing import scene_head_ref as sr                           # noqa: E402
from nicr_mt_scene_analysis_amd.testing.synthetic import input_digest                        # noqa: E402
from oracle import ref_loader                                                                # noqa: E402


def jdump(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


class _NeverCalled:
    def postprocess(self, *args, **kwargs):
        raise AssertionError('the fixture records raw decoder outputs')


def load_reference_decoder():
    ref_loader.load_reference()
    pkg, root = ref_loader.PKG, ref_loader.REF_ROOT
    post = sys.modules[f'{pkg}.model.postprocessing']
    post.get_postprocessing_class = lambda name, **kwargs: _NeverCalled
    post.PostProcessingType = _NeverCalled
    ref_loader._stub_package(f'{pkg}.model.decoder', os.path.join(root, 'model', 'decoder'))
    ref_loader._load('model.decoder.base', 'model/decoder/base.py')
    return ref_loader._load('model.decoder.scene', 'model/decoder/scene.py').SceneClassificationDecoder


def run(cls, name, dtype):
    case, inp = sr.SCENE_HEAD_CASES[name], sr.case_inputs(name)
    C = (case['features'] or case['cm_output'])[1]
    module = cls(n_channels_in=C, n_classes=case['n_classes']).to(dtype).train()
    with torch.no_grad():
        module._task_head.weight.copy_(torch.from_numpy(inp['weight']))
        module._task_head.bias.copy_(torch.from_numpy(inp['bias']))
    x, pooled_map = sr.decoder_input(inp, requires_grad=True, dtype=dtype)
    out, side = module(x, None, {}, do_postprocessing=False)
    assert side is None and out.dtype == dtype
    out.backward(torch.from_numpy(inp['g']).to(dtype))
    for t in x[1][1:] + ((x[0],) if x[1] else ()):
        assert t.grad is None, 'the decoder read a tensor it must not read'
    res = dict(logits=out.detach(), gx=pooled_map.grad, gweight=module._task_head.weight.grad,
               gbias=module._task_head.bias.grad)
    return res, {k: list(v.shape) for k, v in module.state_dict().items()}, inp


def main():
    cls = load_reference_decoder()
    out = {'names': jdump(list(sr.SCENE_HEAD_CASES))}
    for name in sr.SCENE_HEAD_CASES:
        r32, state, inp = run(cls, name, torch.float32)
        r64, state64, _ = run(cls, name, torch.float64)
        assert state == state64
        dist = {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64}
        out[f'{name}__params'] = jdump({'digest': input_digest(*sr.case_arrays(inp)), 'state': state, 'dist': dist})
        for k, v in r64.items():
            out[f'{name}__{k}'] = v.numpy()
        out[f'{name}__logits32'] = r32['logits'].numpy()
        print(name, state, dist)
    path = os.path.join(ROOT, 'tests', 'golden', 'scene_decoder.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
