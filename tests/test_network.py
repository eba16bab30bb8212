"""GPU tier of the composed network (`testing/network_cases.py`): every fused model node and the multi-loss calls
behind one another in one autograd graph, over one training step and over several.

(a) nothing fell back: the census of autograd nodes against the counts derived from the module tree, in float32
    and under bfloat16 autocast;
(b) one step against the float64 oracle (the plain composition on the CPU), both configurations, both shapes, train
    and eval, plus the B = 1 case;
(c) three SGD steps against the oracle doing the same;
(d) the planes every dropout of the network zeroes, in order, against the plain composition under one seed;
(e) to (h) the same BYTES whatever ran before: twice, cold and warm caches, a workspace cache of one entry, a side
    stream; gradient accumulation; no_grad interludes; a captured step replayed;
(i) the census of what the fused nodes are handed in backward.

The bounds of (b) and (c).  No number is fixed by hand.  THE FLOOR is the largest `backbone_cases.distance`, per class
(map: max-norm over outputs, skips and parameters; stat: max-norm over the buffers; grad: 2-norm over gx and parameter
gradients; loss), of the plain
composition on the device in float32 from the oracle: no code under test, only the float32 re-association of
MIOpen's convolutions and batch norms.  The fused network gets FACTOR = 4 x the floor: one more float32
re-association of the same size per node, and MIOpen's algorithm choice varies from box to box.  The floors live in
`network_cases.FLOOR*` and are measured on an MI355X with tools/network_floors.py (docs/measurement_log.md):

    one step        map 1.02e-2 (A/b2/96x128/train raw/instance/2)    grad 1.53e-2 (B/b2/64x160/train, the squeeze bias
                    of the depth SE weighting of stage 0)             loss 1.61e-6    stat 2.55e-5 (running statistics)
    SGD step 1/2/3  map 8.96e-6 / 1.73e-5 / 2.54e-5 (parameters)      stat 2.58e-5 / 3.21e-5 / 5.31e-5

Each is the largest of four (one step) and two (SGD) runs of the tool: torch's convolutions do not repeat their bits
between processes here, and a class's floor moved by up to 4 x between runs (map 5.9e-3 .. 1.02e-2, grad of config
A 3.0e-3 .. 1.43e-2).  The fused network in the same runs: map <= 1.03e-2, grad <= 1.29e-2, loss <= 2.0e-6, stat <=
2.9e-5; SGD map <= 1.6e-5, stat <= 4.1e-5.  In eval mode both lie two orders lower (map 1.4e-4 .. 8.3e-4, grad
1.9e-5 .. 1.3e-4).  The running statistics are a class of their own ('stat') with their own, lower floor: under the map
floor a running variance updated with the biased batch variance would pass (tests/test_network_host.py).

The map floor is that of the instance decoder: its orientation output is a 2-channel field divided
by its length, which comes arbitrarily close to 0 at isolated pixels of any image, and the division amplifies the
float32 rounding of the head there (the CPU's own float32 lies 2e-4 .. 1.4e-3 from the oracle at these fields).
The gradient floor is that of training-mode steps: a few short parameter gradients (the 4-element squeeze biases of
the stage-0 SE weightings) are sums that nearly cancel.  No record had to be held apart, neither of config A nor of B.

Every run prints the plain composition's own distance on the box next to the fused network's."""
import copy

import pytest
import torch

from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.loss import _multi
from nicr_mt_scene_analysis_amd.model import block
from nicr_mt_scene_analysis_amd.model.decoder import mlp_base
from nicr_mt_scene_analysis_amd.testing import network_cases as NC

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
CASES = [(c, 2, hw, mode) for c in NC.CONFIGS for hw in NC.SHAPES for mode in ('train', 'eval')] + \
    [NC.B1_CASE + ('train',)]
SMALL = NC.SHAPES[1]
# Under torch.autocast('cuda', torch.bfloat16) every node of the float32 census is still there (the modules'
# docstrings name the fallbacks autocast can force: a mixed-dtype identity beside a half main path in a tail, a half
# SE input whose autocast result would be float32, maps of another dtype cast before a concatenation): this network
# forces none of them, {class: how many of its nodes autocast turns into torch nodes}
AUTOCAST_FALLBACKS = {}
# (i) what the fused nodes are handed and hand on in backward (`network_cases.handover_census`): {node: [calls, with a
# non-contiguous incoming gradient, with an incoming gradient of another dtype than the node's first saved map (None:
# it saves no map), with an incoming gradient that is a view, that RETURN a view, that return a DENSE view]}.
# What it says: in this wiring no fused node is ever handed a non-contiguous gradient, a view or (float32) another
# dtype: every such gradient meets a torch node or autograd's accumulation first.  The views the issue names are
# there on the way OUT: `UpsampleConcatFunction` returns g[:, :C] (dense at B = 1), each `MlpUpsampleConcatFunction`
# its factor-1 branch (dense at B = 1), and `SEWeightedAddFunction` reshaped parameter gradients.
def _table(mlp_dense, ppm_dense):
    return {'MultiLossFunctionBackward': [3, 0, 0, 0, 0, 0], 'LearnedUpsamplingFunctionBackward': [6, 0, 0, 0, 0, 0],
            'MlpUpsampleConcatFunctionBackward': [3, 0, None, 0, 3, mlp_dense],
            'SEWeightedAddFunctionBackward': [5, 0, 0, 0, 5, 5], 'BatchNormTailFunctionBackward': [18, 0, 0, 0, 0, 0],
            'MaxPool3x3S2FunctionBackward': [2, 0, None, 0, 0, 0],
            'UpsampleConcatFunctionBackward': [1, 0, None, 0, 1, ppm_dense],
            'PyramidPoolFunctionBackward': [1, 0, None, 0, 0, 0]}


HANDOVER = {}
for _key, _dense in ((('A', 2), (0, 0)), (('B', 2), (0, 0)), (('B', 1), (3, 1))):
    HANDOVER[_key + (torch.float32,)] = _table(*_dense)
    # under autocast two of the three multi-loss calls are handed a float32 gradient for bfloat16 predictions
    HANDOVER[_key + (torch.bfloat16,)] = dict(_table(*_dense), MultiLossFunctionBackward=[3, 0, 2, 0, 0, 0])


@pytest.fixture(autouse=True)
def every_tail_is_the_hip_node(monkeypatch):
    monkeypatch.setattr(block, 'FUSED_MIN_ELEMENTS', 1)


@pytest.fixture
def reproducible_torch(monkeypatch):
    """(e) to (h) compare bytes, and torch's own convolutions do not give the same bits twice here by default: the
    PLAIN composition differs from run to run from the first strided convolution on (measured,
    docs/measurement_log.md).  With torch's deterministic algorithms asked for, the convolutions do, and what is
    left to differ is this package's code."""
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)


def build_kwargs(B):
    return {'appm_input_size': NC.B1_APPM_INPUT_SIZE} if B == 1 else {}


@pytest.fixture(scope='module')
def cases():
    """(config, B, hw, mode) -> (CPU float32 network, float32 CPU batch, the oracle's step dict), computed once"""
    made = {}

    def get(config, B, hw, mode):
        key = (config, B, tuple(hw), mode)
        if key not in made:
            net, _ = NC.build(config, hw, **build_kwargs(B))
            net.train(mode == 'train')
            batch = NC.make_batch(B, hw, NC.input_seed(config, B, hw, mode))
            with NC.plain_composition():
                ref = NC.step(copy.deepcopy(net).double(), {k: v.double() if v.is_floating_point() else v
                                                            for k, v in batch.items()}, NC.plain_helpers())
            made[key] = (net, batch, ref)
        return made[key]
    return get


def on_device(net, batch):
    return copy.deepcopy(net).to(DEV), {k: v.to(DEV) for k, v in batch.items()}


def clear_caches():
    ops._BWD_WORKSPACES.clear()
    ops._PPM_SIZE_ARGS.clear()
    mlp_base._AUTOCAST_RESIZED.clear()
    _multi.reset_all()


def fresh_step(net, state, batch, **kwargs):
    """the step from a restored state with new helpers -> copies"""
    NC.restore(net, state)
    return NC.copy_of(NC.step(net, batch, NC.fused_helpers(DEV), **kwargs))


def assert_same_bytes(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (what, k)


# ---------------------------------------------------------------------------- (a)
@pytest.mark.parametrize('hw', NC.SHAPES)
@pytest.mark.parametrize('config', NC.CONFIGS)
def test_nothing_fell_back(cases, config, hw):
    net, batch, _ = cases(config, 2, hw, 'train')
    net, batch = on_device(net, batch)
    print(NC.case_name(config, 2, hw, 'train'), 'routes', NC.routes(net, batch))
    want = NC.expected_node_counts(net)
    assert want == {'pool': 2, 'tail': 18, 'se': 5, 'ppm_pool': 1, 'ppm_upcat': 1, 'mlp_upcat': 3, 'learned_up': 6,
                    'losses': 3}
    state = NC.snapshot(net)
    counts = NC.collections.Counter()
    NC.step(net, batch, NC.fused_helpers(DEV), nodes=counts)
    assert {k: counts[v] for k, v in NC.FUSED_NODES.items()} == want, counts
    # the only torch batch norms: the downsample branches and the ConvNormActs; no torch pool
    assert NC.torch_batch_norm_count(counts) == NC.expected_torch_batch_norms(net) == {'A': 13, 'B': 15}[config]
    assert not any('MaxPool' in k and k != NC.FUSED_NODES['pool'] for k in counts), counts
    NC.restore(net, state)
    auto = NC.collections.Counter()
    with torch.autocast('cuda', torch.bfloat16):
        NC.step(net, batch, NC.fused_helpers(DEV), nodes=auto)
    fell_back = {k: want[k] - auto[v] for k, v in NC.FUSED_NODES.items() if auto[v] != want[k]}
    print(NC.case_name(config, 2, hw, 'train'), 'autocast fallbacks', fell_back)
    assert fell_back == AUTOCAST_FALLBACKS
    assert NC.torch_batch_norm_count(auto) == NC.expected_torch_batch_norms(net) + fell_back.get('tail', 0)


# ---------------------------------------------------------------------------- (b)
@pytest.mark.parametrize('config,B,hw,mode', CASES)
def test_one_step_against_the_float64_oracle(cases, config, B, hw, mode):
    name = NC.case_name(config, B, hw, mode)
    cpu_net, cpu_batch, ref = cases(config, B, hw, mode)
    net, batch = on_device(cpu_net, cpu_batch)
    with NC.plain_composition():
        plain = NC.worst_distances(NC.step(copy.deepcopy(net), batch, NC.plain_helpers()), ref)
    got = NC.step(net, batch, NC.fused_helpers(DEV))
    dist = NC.distances(got, ref)
    fused = NC.worst_distances(got, ref)
    print(name, 'plain', ' '.join(f'{k} {d:.2e} ({f})' for k, (d, f) in sorted(plain.items())))
    print(name, 'fused', ' '.join(f'{k} {d:.2e} ({f})' for k, (d, f) in sorted(fused.items())))
    for field, d in dist.items():
        assert d <= NC.bound(name, NC.field_class(field)), (name, field, d, NC.bound(name, NC.field_class(field)))
    if mode == 'eval':
        before = cpu_net.state_dict()
        for field, t in got.items():
            if field.startswith('after/'):
                assert torch.equal(t.cpu(), before[field[len('after/'):]]), field
    else:
        for field, t in got.items():
            if field.endswith('num_batches_tracked'):
                assert int(t) == 1, field


# ---------------------------------------------------------------------------- (c)
@pytest.mark.parametrize('config', NC.CONFIGS)
def test_three_optimizer_steps(cases, config):
    name = NC.case_name(config, 2, SMALL, 'train')
    cpu_net, _, _ = cases(config, 2, SMALL, 'train')
    seed = NC.input_seed(config, 2, SMALL, 'train')
    batches = [NC.make_batch(2, SMALL, seed + 1000 * i) for i in range(3)]
    with NC.plain_composition():
        ref = NC.optimizer_steps(copy.deepcopy(cpu_net).double(),
                                 [{k: v.double() if v.is_floating_point() else v for k, v in b.items()}
                                  for b in batches], NC.plain_helpers())
    on_dev = [{k: v.to(DEV) for k, v in b.items()} for b in batches]
    with NC.plain_composition():
        plain = NC.optimizer_steps(copy.deepcopy(cpu_net).to(DEV), on_dev, NC.plain_helpers())
    got = NC.optimizer_steps(copy.deepcopy(cpu_net).to(DEV), on_dev, NC.fused_helpers(DEV))
    for idx in range(3):
        for cls, p in sorted(NC.worst_distances(plain[idx], ref[idx]).items()):
            f = NC.worst_distances(got[idx], ref[idx])[cls]
            print(name, 'step', idx + 1, cls, f'plain {p[0]:.2e} ({p[1]})', f'fused {f[0]:.2e} ({f[1]})')
    for idx in range(3):
        for field, d in NC.distances(got[idx], ref[idx]).items():
            limit = NC.step_bound(name, idx, NC.field_class(field))
            assert d <= limit, (name, idx, field, d, limit)
            if field.endswith('num_batches_tracked'):
                assert int(got[idx][field]) == idx + 1


# ---------------------------------------------------------------------------- (d)
def test_dropout_zeroes_the_planes_of_the_plain_composition_in_order():
    cpu_net, _ = NC.build('B', SMALL, dropout=True)
    cpu_net.train()
    net, batch = on_device(cpu_net, NC.make_batch(2, SMALL, 0))
    seen = {}
    for which in ('plain', 'fused'):
        events = seen[which] = []
        run = copy.deepcopy(net)
        torch.manual_seed(1234)
        with NC.dropout_record(run, events):
            if which == 'plain':
                with NC.plain_composition():
                    NC.step(run, batch, NC.plain_helpers())
            else:
                NC.step(run, batch, NC.fused_helpers(DEV))
    # a draw per block of both backbones and one per decoder, and planes are zeroed at all
    assert len(seen['plain']) == 2 * 4 + 3 and sum(len(e) for e in seen['plain']) > 50
    assert seen['fused'] == seen['plain']


# ---------------------------------------------------------------------------- (e)
@pytest.mark.parametrize('config', NC.CONFIGS)
def test_same_bits_whatever_the_history(cases, monkeypatch, reproducible_torch, config):
    cpu_net, cpu_batch, _ = cases(config, 2, SMALL, 'train')
    net, batch = on_device(cpu_net, cpu_batch)
    state = NC.snapshot(net)
    clear_caches()
    cold = fresh_step(net, state, batch)
    helpers = NC.fused_helpers(DEV)
    NC.restore(net, state)
    first = NC.copy_of(NC.step(net, batch, helpers))
    NC.restore(net, state)
    assert_same_bytes(NC.copy_of(NC.step(net, batch, helpers)), first, 'the step twice, one set of helpers')
    assert_same_bytes(first, cold, 'warm caches')
    assert len(ops._BWD_WORKSPACES) > 1
    ops._BWD_WORKSPACES.clear()                         # every new entry now evicts the one before it
    monkeypatch.setattr(ops, '_BWD_WORKSPACES_MAX', 1)
    assert_same_bytes(fresh_step(net, state, batch), cold, 'a workspace cache of one entry')
    assert len(ops._BWD_WORKSPACES) == 1
    monkeypatch.setattr(ops, '_BWD_WORKSPACES_MAX', 64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = fresh_step(net, state, batch)
    torch.cuda.current_stream().wait_stream(side)
    assert_same_bytes(on_side, cold, 'a side stream')


# ---------------------------------------------------------------------------- (f)
@pytest.mark.parametrize('config', NC.CONFIGS)
def test_gradient_accumulation_adds_the_micro_batches(cases, reproducible_torch, config):
    cpu_net, cpu_batch, _ = cases(config, 2, SMALL, 'train')
    net, batch1 = on_device(cpu_net, cpu_batch)
    batch2 = {k: v.to(DEV) for k, v in NC.make_batch(2, SMALL, 4321).items()}
    state = NC.snapshot(net)
    g1 = fresh_step(net, state, batch1)
    g2 = fresh_step(net, state, batch2)
    NC.restore(net, state)
    helpers = NC.fused_helpers(DEV)
    NC.step(net, batch1, helpers)
    both = NC.step(net, batch2, helpers, zero_grad=False)
    for field in g1:
        if field.startswith('grad/'):
            assert torch.equal(both[field], g1[field] + g2[field]), field


# ---------------------------------------------------------------------------- (g)
@pytest.mark.parametrize('config', NC.CONFIGS)
def test_no_grad_interludes_leave_the_next_step_alone(cases, reproducible_torch, config):
    cpu_net, cpu_batch, _ = cases(config, 2, SMALL, 'train')
    net, batch1 = on_device(cpu_net, cpu_batch)
    batch2 = {k: v.to(DEV) for k, v in NC.make_batch(2, SMALL, 4321).items()}
    other = {k: v.to(DEV) for k, v in NC.make_batch(2, SMALL, 8765).items()}
    inputs = {k: other[k] for k in ('rgb', 'depth')}
    helpers = NC.fused_helpers(DEV)
    NC.step(net, batch1, helpers)
    after_step = NC.snapshot(net)
    net.eval()
    with torch.no_grad():
        NC.forward(net, inputs, other)
    net.train()
    for k, v in net.state_dict().items():
        assert torch.equal(v, after_step[k]), ('an eval-mode forward moved', k)
    with torch.no_grad():
        NC.forward(net, inputs, other)
    after_interlude = NC.snapshot(net)
    got = NC.copy_of(NC.step(net, batch2, helpers))
    # the statistics a training forward WITH gradients leaves, from the same state
    NC.restore(net, after_step)
    NC.forward(net, inputs, other)
    moved = 0
    for k, v in net.state_dict().items():
        assert torch.equal(v, after_interlude[k]), ('a no_grad training forward differs in', k)
        moved += not torch.equal(v, after_step[k])
    assert moved > 3 * 18
    assert_same_bytes(got, fresh_step(net, after_interlude, batch2), 'the step after the interludes')


# ---------------------------------------------------------------------------- (h)
def test_captured_step_replays_the_eager_step(cases, reproducible_torch):
    cpu_net, cpu_batch, _ = cases('A', 2, SMALL, 'train')
    net, batch1 = on_device(cpu_net, cpu_batch)
    batch2 = {k: v.to(DEV) for k, v in NC.make_batch(2, SMALL, 4321).items()}
    state = NC.snapshot(net)
    eager = copy.deepcopy(net)
    eager_helpers = NC.fused_helpers(DEV)
    want = [NC.copy_of(NC.step(eager, b, eager_helpers)) for b in (batch1, batch2)]

    static = {k: v.clone() for k, v in batch1.items()}
    for k in ('rgb', 'depth'):
        static[k].requires_grad_(True)
    helpers = NC.fused_helpers(DEV)

    def run():
        for k in ('rgb', 'depth'):
            static[k].grad = None
        return NC.step(net, static, helpers)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    NC.restore(net, state)
    net.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for b, w in zip((batch1, batch2), want):
        with torch.no_grad():
            for k, v in b.items():
                static[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        assert_same_bytes(NC.copy_of(out), w, 'a replay')


# ---------------------------------------------------------------------------- (i)
@pytest.mark.parametrize('config,B', [('A', 2), ('B', 2), ('B', 1)])
def test_handover_census(cases, config, B):
    cpu_net, cpu_batch, _ = cases(config, B, SMALL, 'train')
    net, batch = on_device(cpu_net, cpu_batch)
    state = NC.snapshot(net)
    for dtype in (torch.float32, torch.bfloat16):
        table = {}
        NC.restore(net, state)
        with torch.autocast('cuda', torch.bfloat16, enabled=dtype == torch.bfloat16):
            NC.step(net, batch, NC.fused_helpers(DEV), prepare=NC.handover_census(table))
        print(NC.case_name(config, B, SMALL, 'train'), dtype, 'hand-over', table)
        assert table == HANDOVER.get((config, B, dtype))
