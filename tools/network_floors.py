"""Print the noise floors of tests/test_network.py: per case and class, the distance of the plain composition
(`network_cases.plain_composition`, float32 on the device) and of the fused network from the float64 CPU oracle,
for one step and for three SGD steps, and the maximum per class over the cases.  Run on the GPU:

    python tools/network_floors.py

The `FLOOR*` tables of testing/network_cases.py and docs/measurement_log.md are written from its output."""
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nicr_mt_scene_analysis_amd.model import block                                  # noqa: E402
from nicr_mt_scene_analysis_amd.testing import network_cases as NC                  # noqa: E402

DEV = torch.device('cuda:0')
SMALL = NC.SHAPES[1]


def doubled(batch):
    return {k: v.double() if v.is_floating_point() else v for k, v in batch.items()}


def fmt(worst):
    return {k: (float(f'{d:.3g}'), f) for k, (d, f) in sorted(worst.items())}


def main():
    block.FUSED_MIN_ELEMENTS = 1
    cases = [(c, 2, hw, mode) for c in NC.CONFIGS for hw in NC.SHAPES for mode in ('train', 'eval')] + \
        [NC.B1_CASE + ('train',)]
    floor = {}
    for config, B, hw, mode in cases:
        name = NC.case_name(config, B, hw, mode)
        net, _ = NC.build(config, hw, **({'appm_input_size': NC.B1_APPM_INPUT_SIZE} if B == 1 else {}))
        net.train(mode == 'train')
        batch = NC.make_batch(B, hw, NC.input_seed(config, B, hw, mode))
        dev_batch = {k: v.to(DEV) for k, v in batch.items()}
        with NC.plain_composition():
            ref = NC.step(copy.deepcopy(net).double(), doubled(batch), NC.plain_helpers())
            plain = NC.step(copy.deepcopy(net).to(DEV), dev_batch, NC.plain_helpers())
        fused = NC.step(copy.deepcopy(net).to(DEV), dev_batch, NC.fused_helpers(DEV))
        worst = NC.worst_distances(plain, ref)
        print(json.dumps({'case': name, 'plain': fmt(worst), 'fused': fmt(NC.worst_distances(fused, ref))}), flush=True)
        for cls, (d, _) in worst.items():
            floor[(config, cls)] = max(floor.get((config, cls), 0.0), d)
    print(json.dumps({'floor': {f'{c}/{cls}': float(f'{d:.3g}') for (c, cls), d in sorted(floor.items())}}))
    for config in NC.CONFIGS:
        net, _ = NC.build(config, SMALL)
        net.train()
        seed = NC.input_seed(config, 2, SMALL, 'train')
        batches = [NC.make_batch(2, SMALL, seed + 1000 * i) for i in range(3)]
        on_dev = [{k: v.to(DEV) for k, v in b.items()} for b in batches]
        with NC.plain_composition():
            ref = NC.optimizer_steps(copy.deepcopy(net).double(), [doubled(b) for b in batches], NC.plain_helpers())
            plain = NC.optimizer_steps(copy.deepcopy(net).to(DEV), on_dev, NC.plain_helpers())
        fused = NC.optimizer_steps(copy.deepcopy(net).to(DEV), on_dev, NC.fused_helpers(DEV))
        for idx in range(3):
            print(json.dumps({'steps': NC.case_name(config, 2, SMALL, 'train'), 'step': idx + 1,
                              'plain': fmt(NC.worst_distances(plain[idx], ref[idx])),
                              'fused': fmt(NC.worst_distances(fused[idx], ref[idx]))}), flush=True)


if __name__ == '__main__':
    main()
