"""Writes tests/golden/mlp_decoder.npz: the reference's unmodified MLP decoders
(`model/decoder/{base,dense_utils,dense_base,mlp_base,semantic,embedding,normal,instance}.py` with its
`activation.py`, `normalization.py`, `utils.py`, `upsampling.py`, `encoder_decoder_fusion.py`,
`block.py`), loaded through `oracle.ref_loader`, run on the CPU in float32 on the seeded cases of
`testing.mlp_decoder_cases.MLP_DECODER_CASES`.  BatchNorm runs in eval mode with the seeded running
statistics of the case; the decoders are called with do_postprocessing=False (the reference's
postprocessing factory is replaced by a stand-in that is never called).

The fixture holds recorded results only.  The inputs are NOT stored: a SHA-256 of their bytes is,
and the tests regenerate them and fail on a mismatch.  Per case (`names`):
  <case>__params     JSON {digest, n_outputs, skip_keys, emb_shapes}
  <case>__out<k>     output k, float32 (one output; center, offset(, orientation) for the instance decoder)
  <case>__gx         the gradient of sum_k sum(out_k * gy_k) w.r.t. x
  <case>__gskip<d>   ... w.r.t. the skip of downsampling d
  <case>__cat        the concatenated tensor in front of `fuse` (by a forward pre-hook)
  <case>__gcat       its gradient
  <case>__emb<i>     embedded branch map i (the output of the branch's `embedding`, by a forward hook)
  <case>__gemb<i>    its gradient
  train              JSON: output shapes of the train-mode case
  state              JSON {decoder: {state_dict key: shape}} for the four decoders at MLP_DECODER_STATE_PROBE
  head__<k>_<j>      InstanceHead output j without (k = 0) / with (k = 1) orientation at INSTANCE_HEAD_PROBE
  head__digest<k>    JSON digest of that probe's inputs

Usage: python tools/gen_golden_mlp_decoder.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd.model import decoder as own_decoder                         # noqa: E402
from nicr_mt_scene_analysis_amd.model import get_encoder_decoder_fusion_class as own_fusion  # noqa: E402
from nicr_mt_scene_analysis_amd.model import get_upsampling_class as own_upsampling          # noqa: E402
from nicr_mt_scene_analysis_amd.testing import mlp_decoder_cases as mc                       # noqa: E402
from nicr_mt_scene_analysis_amd.testing.synthetic import input_digest                        # noqa: E402
from oracle import ref_loader                                                                # noqa: E402


def jdump(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


class _NeverCalled:
    def postprocess(self, *args, **kwargs):
        raise AssertionError('the fixture records raw decoder outputs')


def load_reference_package():
    ref_loader.load_reference()
    pkg, root = ref_loader.PKG, ref_loader.REF_ROOT
    ref_loader._load('utils._normal', 'utils/_normal.py')
    utils_pkg = sys.modules[f'{pkg}.utils']
    utils_pkg.NormalOutputNormalization = sys.modules[f'{pkg}.utils._normal'].NormalOutputNormalization
    utils_pkg.OrientationOutputNormalization = sys.modules[f'{pkg}.utils._orientation'].OrientationOutputNormalization
    post = sys.modules[f'{pkg}.model.postprocessing']
    post.get_postprocessing_class = lambda name, **kwargs: _NeverCalled
    post.PostProcessingType = _NeverCalled
    ns = types.SimpleNamespace()
    for mod in ('activation', 'normalization', 'utils', 'upsampling', 'encoder_decoder_fusion', 'block'):
        setattr(ns, mod, ref_loader._load(f'model.{mod}', f'model/{mod}.py'))
    ref_loader._stub_package(f'{pkg}.model.decoder', os.path.join(root, 'model', 'decoder'))
    dec = types.SimpleNamespace()
    for mod in ('base', 'dense_utils', 'dense_base', 'mlp_base', 'semantic', 'embedding', 'normal', 'instance'):
        m = ref_loader._load(f'model.decoder.{mod}', f'model/decoder/{mod}.py')
        for name in ('SemanticMLPDecoder', 'EmbeddingMLPDecoder', 'NormalMLPDecoder', 'InstanceMLPDecoder',
                     'InstanceHead'):
            if hasattr(m, name):
                setattr(dec, name, getattr(m, name))
    ns.decoder = dec
    return ns


def build_pair(ref, case):
    """the reference's decoder with the case's seeded state, and the inputs (whose parameter shapes come
    from this package's decoder: the key lists must agree)"""
    own = mc.build_decoder(own_decoder, own_fusion, own_upsampling, case)
    module = mc.build_decoder(ref.decoder, ref.encoder_decoder_fusion.get_encoder_decoder_fusion_class,
                              ref.upsampling.get_upsampling_class, case)
    shapes = mc.state_shapes(own)
    assert mc.state_shapes(module) == shapes and list(mc.state_shapes(module)) == list(shapes), \
        (list(mc.state_shapes(module).items()), list(shapes.items()))
    inp = mc.make_decoder_inputs(case, shapes, mc.output_shapes(case))
    mc.load_state(module, inp['state'])
    return module, inp


def record(ref, out, key):
    module, inp = build_pair(ref, key)
    module.eval()
    taps = {}

    def keep_input(label):
        def hook(_, args):
            args[0].retain_grad()
            taps[label] = args[0]
        return hook

    def keep_output(label):
        def hook(_, args, result):
            result.retain_grad()
            taps[label] = result
        return hook

    branches = [module.main_branch] + list(module.skip_branches)
    for i, b in enumerate(branches):
        b.embedding.register_forward_hook(keep_output(f'emb{i}'))
    module.fuse.register_forward_pre_hook(keep_input('cat'))
    x = torch.from_numpy(inp['x']).requires_grad_(True)
    skips = mc.skips_to(inp, requires_grad=True)
    outs, side = module((x, ()), skips, {}, do_postprocessing=False)
    assert side == ()
    outs = outs if isinstance(outs, tuple) else (outs,)
    assert [tuple(o.shape) for o in outs] == [tuple(s) for s in mc.output_shapes(key)], [o.shape for o in outs]
    torch.autograd.backward(outs, [torch.from_numpy(g) for g in inp['gys']])
    for k, o in enumerate(outs):
        out[f'{key}__out{k}'] = o.detach().numpy()
    out[f'{key}__gx'] = x.grad.numpy()
    for d, s in skips.items():
        out[f'{key}__gskip{d}'] = s['rgb'].grad.numpy()
    out[f'{key}__cat'] = taps['cat'].detach().numpy()
    out[f'{key}__gcat'] = taps['cat'].grad.numpy()
    for i in range(len(branches)):
        out[f'{key}__emb{i}'] = taps[f'emb{i}'].detach().numpy()
        out[f'{key}__gemb{i}'] = taps[f'emb{i}'].grad.numpy()
    out[f'{key}__params'] = jdump({'digest': mc.decoder_input_digest(inp), 'n_outputs': len(outs),
                                   'skip_keys': list(skips),
                                   'emb_shapes': [list(taps[f'emb{i}'].shape) for i in range(len(branches))]})
    print(key, [tuple(o.shape) for o in outs], tuple(taps['cat'].shape))


def head_inputs(with_orientation, head):
    n_in, _, (B, H, W), seed = mc.INSTANCE_HEAD_PROBE
    rng = np.random.default_rng(seed + int(with_orientation))
    state = mc.draw_state(rng, mc.state_shapes(head))
    return rng.standard_normal((B, n_in, H, W)).astype(np.float32), state


def main():
    ref = load_reference_package()
    out = {'names': jdump(list(mc.MLP_DECODER_CASES))}
    for key in mc.MLP_DECODER_CASES:
        record(ref, out, key)
    module, inp = build_pair(ref, mc.MLP_DECODER_TRAIN_CASE)
    module.train()
    outs, _ = module((torch.from_numpy(inp['x']), ()), mc.skips_to(inp), {}, do_postprocessing=False)
    out['train'] = jdump({'out': [list(outs.shape)]})
    probe = mc.MLP_DECODER_STATE_PROBE
    state = {}
    for name, kwargs in mc.MLP_DECODER_STATE_KWARGS.items():
        case = dict(probe, decoder=name, mode='bilinear', kwargs=kwargs)
        module = mc.build_decoder(ref.decoder, ref.encoder_decoder_fusion.get_encoder_decoder_fusion_class,
                                  ref.upsampling.get_upsampling_class, case)
        state[name] = {k: list(v.shape) for k, v in module.state_dict().items()}
    out['state'] = jdump(state)
    n_in, per_task, _, _ = mc.INSTANCE_HEAD_PROBE
    for k in (0, 1):
        head = ref.decoder.InstanceHead(n_in, n_channels_per_task=per_task, with_orientation=bool(k),
                                        upsampling=ref.upsampling.get_upsampling_class('bilinear'),
                                        n_upsamplings=1).eval()
        x, st = head_inputs(bool(k), head)
        mc.load_state(head, st)
        for j, o in enumerate(head(torch.from_numpy(x))):
            out[f'head__{k}_{j}'] = o.detach().numpy()
        out[f'head__digest{k}'] = jdump(input_digest(x, *st.values()))
    path = os.path.join(ROOT, 'tests', 'golden', 'mlp_decoder.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
