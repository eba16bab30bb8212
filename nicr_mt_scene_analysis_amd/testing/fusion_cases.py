"""TEST INFRASTRUCTURE — never imported by the product path.

The seeded cases of tests/golden/encoder_decoder_fusion.npz (tools/gen_golden_fusion.py): the inputs
are regenerated here, the fixture holds the reference's results and a digest of these inputs."""
from typing import Dict

import numpy as np

from .synthetic import input_digest

# name: (fusion name, n_channels_encoder, n_channels_decoder, (B, H, W), seed)
FUSION_CASES = {
    'swin_ln_select_eq': ('swin-ln-select', 12, 12, (2, 3, 4), 110),
    'swin_ln_select_ne': ('swin-ln-select', 8, 12, (2, 3, 4), 111),
    'swin_ln_add_eq': ('swin-ln-add', 12, 12, (2, 5, 6), 112),
    'swin_ln_add_ne': ('swin-ln-add', 8, 12, (2, 3, 5), 113),
    'swin_ln_add_rgb_eq': ('swin-ln-add-rgb', 7, 7, (1, 3, 5), 114),
    'swin_ln_add_rgb_ne': ('swin-ln-add-rgb', 12, 8, (2, 3, 4), 115),
    'add_eq': ('add', 8, 8, (2, 3, 4), 116),
    'add_ne': ('add', 8, 12, (2, 3, 4), 117),
    'select_depth_ne': ('select-depth', 8, 12, (2, 4, 3), 118),
    'swin_add_eq': ('swin-add', 8, 8, (2, 3, 4), 119),
    'swin_select_ne': ('swin-select', 8, 12, (2, 3, 4), 120),
    'none': ('none', 8, 12, (2, 3, 4), 121),
}
# the channel pairs of the state-dict record of all names, and the probe of the output-shape record
FUSION_STATE_CHANNELS = ((8, 8), (8, 12))
FUSION_SHAPE_INPUT = (1, 3, 4)              # (B, H, W)


def fusion_key(fusion: str) -> str:
    """the key of the encoder's skip dict a case uses: the modality of the name, else a single key"""
    return fusion.rsplit('-', 1)[-1] if fusion.endswith(('-rgb', '-depth')) else 'enc'


def fusion_param_shapes(fusion: str, n_enc: int, n_dec: int) -> Dict[str, tuple]:
    """the trainable parameters of the fusion module, in state-dict order"""
    shapes = {}
    if fusion != 'none' and n_enc != n_dec:
        shapes.update({'layer.conv.weight': (n_dec, n_enc, 1, 1), 'layer.norm.weight': (n_dec,),
                       'layer.norm.bias': (n_dec,)})
    if fusion.startswith('swin-ln'):
        shapes.update({'ln.weight': (n_enc,), 'ln.bias': (n_enc,)})
    return shapes


def make_fusion_inputs(name: str) -> Dict[str, object]:
    """The inputs of one case of FUSION_CASES, float32: 'x_enc' ([B,H,W,n_enc] for the swin names,
    [B,n_enc,H,W] otherwise), 'x_dec' and 'gy' [B,n_dec,H,W] (gy: the upstream gradient), 'params'
    {state-dict key: values}.  Generator draws and float32 casts only."""
    fusion, n_enc, n_dec, (B, H, W), seed = FUSION_CASES[name]
    rng = np.random.default_rng(seed)
    enc_shape = (B, H, W, n_enc) if fusion.startswith('swin') else (B, n_enc, H, W)
    x_enc = rng.standard_normal(enc_shape).astype(np.float32)
    x_dec = rng.standard_normal((B, n_dec, H, W)).astype(np.float32)
    gy = rng.standard_normal((B, n_dec, H, W)).astype(np.float32)
    params = {}
    for key, shape in fusion_param_shapes(fusion, n_enc, n_dec).items():
        draw = rng.standard_normal(shape)
        if key.endswith('conv.weight'):
            params[key] = (0.3 * draw).astype(np.float32)
        elif key.endswith('weight'):
            params[key] = (1.0 + 0.25 * draw).astype(np.float32)
        else:
            params[key] = (0.5 * draw).astype(np.float32)
    return {'x_enc': x_enc, 'x_dec': x_dec, 'gy': gy, 'params': params}


def fusion_input_digest(inputs) -> str:
    return input_digest(inputs['x_enc'], inputs['x_dec'], inputs['gy'], *inputs['params'].values())
