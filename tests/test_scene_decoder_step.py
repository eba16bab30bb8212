"""GPU tier: the scene branch of a network composed of fused nodes in one training step: context module
(`get_context_module`) -> `SceneClassificationDecoder` -> `ScenePostprocessing` -> `SceneTaskHelper.training_step`
-> backward, on a [2, 32, 3, 4] map.

The oracle is the same composition in plain torch in float64 on the CPU (`network_cases.plain_composition` for the
context module, the decoder's torch path, `F.cross_entropy`).  The floor is that plain composition in float32 on the
device.  The loss and the gradient at the context module's input must lie within 4 x the floor's measured
distance from the oracle.  The step runs once eagerly and once as a captured `torch.cuda.graph` replayed on new
inputs; the two must agree in every bit."""
import copy

import pytest
import torch
import torch.nn.functional as F

from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd.task_helper import SceneTaskHelper
from nicr_mt_scene_analysis_amd.testing import network_cases as NC

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
B, C, H, W, K = 2, 32, 3, 4, 10
FACTOR = 4.0
CONTEXT_MODULES = ('ppm', 'appm-1-2-4-8')


def build(name):
    torch.manual_seed(4100 + len(name))
    cm = model.get_context_module(name, C, C, input_size=(H, W)).train()
    dec = model.SceneClassificationDecoder(cm.n_channels_reduction, K).train()
    return cm, dec


def make_batch(seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((B, C, H, W), generator=gen)
    labels = torch.randint(1, K + 1, (B,), generator=gen).to(torch.uint8)
    return x, labels


def plain_loss(logits, labels):
    return F.cross_entropy(logits, labels.long() - 1, ignore_index=-1)


def step(cm, dec, loss_fn, x, labels):
    """-> (loss, the gradient at the context module's input)"""
    x.grad = None
    out, feats = cm(x)
    post = dec((out, feats), None, {'scene': labels})
    loss = loss_fn(post['scene_output'], labels, post)
    loss.backward()
    return loss.detach(), x.grad


def fused_loss(helper):
    return lambda logits, labels, post: helper.training_step({'scene': labels}, 0, post)[0]['scene_total_loss']


def helper_on_device():
    h = SceneTaskHelper(K)
    h.initialize(DEV)
    return h


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                                                     b.contiguous().view(torch.int32))


@pytest.fixture
def reproducible_torch(monkeypatch):
    # torch's own convolutions give the same bits twice only with its deterministic algorithms asked for
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)


@pytest.mark.parametrize('name', CONTEXT_MODULES)
def test_training_step_against_the_float64_composition(name):
    cm, dec = build(name)
    x, labels = make_batch(1)
    with NC.plain_composition():
        cm64, dec64 = copy.deepcopy(cm).double(), copy.deepcopy(dec).double()
        loss64, gx64 = step(cm64, dec64, lambda lo, la, post: plain_loss(lo, la), x.double().requires_grad_(True),
                            labels)
        cm32, dec32 = copy.deepcopy(cm).to(DEV), copy.deepcopy(dec).to(DEV)
        dec32.takes_hip_path = lambda t: False
        loss32, gx32 = step(cm32, dec32, lambda lo, la, post: plain_loss(lo, la),
                            x.to(DEV).requires_grad_(True), labels.to(DEV))
    cmf, decf = copy.deepcopy(cm).to(DEV), copy.deepcopy(dec).to(DEV)
    feats = cmf(x.to(DEV))[1]
    assert decf.takes_hip_path(feats[0]) and tuple(feats[0].shape[2:]) == (1, 1)
    loss, gx = step(cmf, decf, fused_loss(helper_on_device()), x.to(DEV).requires_grad_(True), labels.to(DEV))
    assert loss.dtype == torch.float32 and gx.dtype == torch.float32 and bool(gx64.abs().max() > 0)
    for what, got, floor, truth in (('loss', loss, loss32, loss64), ('gx', gx, gx32, gx64)):
        allowed = FACTOR * float((floor.cpu().double() - truth).abs().max())
        dist = float((got.cpu().double() - truth).abs().max())
        print(f'{name} {what}: distance {dist:.3e}, allowed {allowed:.3e}')
        assert dist <= allowed, (name, what, dist, allowed)


@pytest.mark.parametrize('name', CONTEXT_MODULES)
def test_captured_step_replays_the_eager_step(reproducible_torch, name):
    cm, dec = build(name)
    cm, dec = cm.to(DEV), dec.to(DEV)
    batches = [tuple(t.to(DEV) for t in make_batch(seed)) for seed in (1, 2)]
    eager_cm, eager_dec = copy.deepcopy(cm), copy.deepcopy(dec)
    eager_loss = fused_loss(helper_on_device())
    want = []
    for x, labels in batches:
        loss, gx = step(eager_cm, eager_dec, eager_loss, x.clone().requires_grad_(True), labels)
        want.append((loss.clone(), gx.clone()))

    state = copy.deepcopy(cm.state_dict())
    static_x = batches[0][0].clone().requires_grad_(True)
    static_labels = batches[0][1].clone()
    loss_fn = fused_loss(helper_on_device())
    # the eager calls a capture needs first, on the current stream: this file draws no stream from torch's pool,
    # so the streams of the files that run after it are the ones they get without it
    for _ in range(3):
        step(cm, dec, loss_fn, static_x, static_labels)
    torch.cuda.synchronize()
    cm.load_state_dict(state)
    cm.zero_grad(set_to_none=True)
    dec.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(cm, dec, loss_fn, static_x, static_labels)
    for (x, labels), (loss, gx) in zip(batches, want):
        with torch.no_grad():
            static_x.copy_(x)
            static_labels.copy_(labels)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bytes(out[0].reshape(1), loss.reshape(1)), 'the loss of a replay'
        assert same_bytes(out[1], gx), 'the gradient of a replay'
