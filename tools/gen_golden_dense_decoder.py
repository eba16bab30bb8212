"""Writes tests/golden/dense_decoder.npz: the reference's unmodified convolutional dense decoders
(`model/decoder/{dense_base,semantic,instance,normal}.py` with the modules `tools/gen_golden_mlp_decoder.py`
loads for them), loaded through `oracle.ref_loader`, run on the CPU in float32 and in float64 on the seeded
cases of `testing.dense_decoder_cases.DENSE_DECODER_CASES`.  The records are taken in training mode, so the side
outputs exist, with every BatchNorm in eval mode (the seeded running statistics of the case) and the
NonBottleneck1D dropout at p = 0; the decoders are called with do_postprocessing=False.

The fixture holds recorded results only.  The inputs are NOT stored: a SHA-256 of their bytes is, and the tests
regenerate them and fail on a mismatch.  Per case (`names`) and precision <p> in (f32, f64):
  <case>__params          JSON {digest, n_outputs, n_sides, skip_keys, steps}
  <case>__<p>_out<k>      output k (main outputs first, then the outputs of every side head, in order)
  <case>__<p>_gx          the gradient of sum_k sum(out_k * gy_k) w.r.t. x
  <case>__<p>_gskip<d>    ... w.r.t. the skip of downsampling d
  <case>__<p>_u<i>, _e<i>, _s<i>   around the fused step of decoder module i: the upsampled map (output of
                          `decoder_modules.<i>.upsample`), the adapted skip (output of `fusions.<j>.layer`) and their
                          sum (output of `fusions.<j>`), by forward hooks
  <case>__<p>_gs<i>       the gradient of that sum, which is the gradient of u and of e as well (asserted here)
  train                   JSON: output and side-output shapes of the train-mode case
  state                   JSON {decoder: {state_dict key: shape}} for the three decoders at DENSE_DECODER_STATE_PROBE

Usage: python tools/gen_golden_dense_decoder.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from nicr_mt_scene_analysis_amd.model import decoder as own_decoder                         # noqa: E402
from nicr_mt_scene_analysis_amd.model import get_block_class as own_block                    # noqa: E402
from nicr_mt_scene_analysis_amd.model import get_encoder_decoder_fusion_class as own_fusion  # noqa: E402
from nicr_mt_scene_analysis_amd.model import get_upsampling_class as own_upsampling          # noqa: E402
from nicr_mt_scene_analysis_amd.testing import dense_decoder_cases as dc                     # noqa: E402
from oracle import ref_loader                                                                # noqa: E402
import gen_golden_mlp_decoder as mlp_gen                                                     # noqa: E402

jdump = mlp_gen.jdump


def load_reference_package():
    ref = mlp_gen.load_reference_package()
    for mod, name in (('semantic', 'SemanticDecoder'), ('instance', 'InstanceDecoder'), ('normal', 'NormalDecoder')):
        setattr(ref.decoder, name, getattr(sys.modules[f'{ref_loader.PKG}.model.decoder.{mod}'], name))
    return ref


def build_reference(ref, case):
    return dc.build_decoder(ref.decoder, ref.encoder_decoder_fusion.get_encoder_decoder_fusion_class,
                            ref.upsampling.get_upsampling_class, ref.block.get_block_class, case)


def build_pair(ref, case):
    """the reference's decoder with the case's seeded state, and the inputs (whose parameter shapes come from this
    package's decoder: the key lists must agree)"""
    own = dc.build_decoder(own_decoder, own_fusion, own_upsampling, own_block, case)
    module = build_reference(ref, case)
    shapes = dc.state_shapes(own)
    assert list(dc.state_shapes(module).items()) == list(shapes.items()), \
        (list(dc.state_shapes(module).items()), list(shapes.items()))
    inp = dc.make_decoder_inputs(case, shapes)
    dc.load_state(module, inp['state'])
    return module, inp


def record(ref, out, key, dtype, tag):
    module, inp = build_pair(ref, key)
    module = module.to(dtype)
    dc.record_mode(module)
    taps = {}

    def keep_output(label):
        def hook(_, args, result):
            if not result.is_leaf:
                result.retain_grad()
            taps[label] = result
        return hook

    steps = dc.fused_steps(key)
    for i, j, _ in steps:
        module.decoder_modules[i].upsample.register_forward_hook(keep_output(f'u{i}'))
        module.fusions[j].layer.register_forward_hook(keep_output(f'e{i}'))
        module.fusions[j].register_forward_hook(keep_output(f's{i}'))
    x = torch.from_numpy(inp['x']).to(dtype).requires_grad_(True)
    skips = {d: {'rgb': s['rgb'].to(dtype).requires_grad_(True)} for d, s in dc.skips_to(inp).items()}
    outs, sides = module((x, ()), skips, {}, do_postprocessing=False)
    flat = dc.flat_outputs(outs, sides)
    want = [tuple(s) for s in dc.output_shapes(key)] + [tuple(s) for side in dc.side_output_shapes(key) for s in side]
    assert [tuple(o.shape) for o in flat] == want, ([tuple(o.shape) for o in flat], want)
    torch.autograd.backward(flat, dc.flat_gradients(inp, dtype))
    for k, o in enumerate(flat):
        out[f'{key}__{tag}_out{k}'] = o.detach().numpy()
    out[f'{key}__{tag}_gx'] = x.grad.numpy()
    for d, s in skips.items():
        out[f'{key}__{tag}_gskip{d}'] = s['rgb'].grad.numpy()
    for i, _, _ in steps:
        for label in ('u', 'e', 's'):
            out[f'{key}__{tag}_{label}{i}'] = taps[f'{label}{i}'].detach().numpy()
        gs = taps[f's{i}'].grad
        assert torch.equal(taps[f'u{i}'].grad, gs)
        if not taps[f'e{i}'].is_leaf:                           # an Identity layer hands the skip leaf on
            assert torch.equal(taps[f'e{i}'].grad, gs)
        out[f'{key}__{tag}_gs{i}'] = gs.numpy()
    out[f'{key}__params'] = jdump({'digest': dc.decoder_input_digest(inp), 'n_outputs': len(dc.output_shapes(key)),
                                   'n_sides': len(sides), 'skip_keys': list(skips),
                                   'steps': [list(s) for s in steps]})
    print(key, tag, [tuple(o.shape) for o in flat])


def main():
    ref = load_reference_package()
    out = {'names': jdump(list(dc.DENSE_DECODER_CASES))}
    for key in dc.DENSE_DECODER_CASES:
        record(ref, out, key, torch.float32, 'f32')
        record(ref, out, key, torch.float64, 'f64')
    module, inp = build_pair(ref, dc.DENSE_DECODER_TRAIN_CASE)
    module.train()
    outs, sides = module((torch.from_numpy(inp['x']), ()), dc.skips_to(inp), {}, do_postprocessing=False)
    out['train'] = jdump({'out': [list(outs.shape)], 'sides': [list(s.shape) for s in sides]})
    state = {}
    for name, kwargs in dc.DENSE_DECODER_STATE_KWARGS.items():
        module = build_reference(ref, dict(dc.DENSE_DECODER_STATE_PROBE, decoder=name, kwargs=kwargs))
        state[name] = {k: list(v.shape) for k, v in module.state_dict().items()}
    out['state'] = jdump(state)
    path = os.path.join(ROOT, 'tests', 'golden', 'dense_decoder.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
