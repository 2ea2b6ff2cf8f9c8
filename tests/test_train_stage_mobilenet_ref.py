"""tests/_train_stage_dw.py proved on the CPU before it judges the kernels (no GPU): the seven ops of tdrn_amd.model.networks are
replaced by float32 torch stand-ins of the same signatures (test_train_stage_ref.py's six and F.conv2d(groups=C) for
depthwise_conv2d), dualrefinedet_mobilenet's RefineSSD.forward_train + smooth_loss.backward() run on the CPU (single head, 192 px,
batch 1, synthetic weights seed 0, frames seed 5), and

  (a) the stages are the module's holders: 38 conv2d, 15 depthwise_conv2d, 33 batch_norm, 3 conv_transpose2d, 2 l2norm,
      8 conv_offset2d, no max_pool2d; every parameter in exactly one stage, every hook fired once (Recorder.finish);
  (b) a correct fp32 implementation passes every stage, so the references alone stay inside the checker's caps at this input (ReLU
      kink <= 1 % of a stage, near_decision <= max(2, numel // 1000)); the worst share per kind is printed: the yardstick of DESIGN.md;
      the same for the BatchNorm stages of the eval-mode step of the GPU file (batch 2, running statistics calibrated on the input:
      _train_stage_dw.calibrate);
  (c) a depthwise stand-in with one tap of its weight gradient dropped (backbone.6.0), and one whose grad_input is shifted by one column
      (extras.0.3.0), fail at their own stage, at the tensor the mutation breaks, and no stage next to them fails.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import _train_model_ref as T
import _train_stage_dw as W
import _train_stage_ref as R
import test_train_stage_ref as V
from tdrn_amd import _lib
from tdrn_amd.model import networks
from tdrn_amd.model.dualrefinedet_mobilenet import build_net
from tdrn_amd.utils import synth

torch.set_num_threads(min(16, torch.get_num_threads()))
SIZE, MAPS, SEED = 192, (24, 12, 6, 3), 5
EXPECTED = dict(conv2d=38, depthwise_conv2d=15, batch_norm=33, conv_transpose2d=3, l2norm=2, conv_offset2d=8)


def depthwise_conv2d(input, weight, bias=None, stride=1, padding=1):
    return F.conv2d(input, weight, bias, stride, padding, 1, input.shape[1])


STAND_INS = dict(V.STAND_INS, depthwise_conv2d=depthwise_conv2d)
MUTATED = [None]
MUTATIONS = {"backbone.6.0": ("grad_weight", "one tap of the depthwise weight gradient dropped"),
             "extras.0.3.0": ("grad_input", "depthwise grad_input shifted by one column")}


def m_depthwise_conv2d(input, weight, bias=None, stride=1, padding=1):
    fn = lambda x, w: depthwise_conv2d(x, w, None, stride, padding)
    names = {id(p): n for n, p in MUTATED[0].named_parameters()} if MUTATED[0] is not None else {}
    if names.get(id(weight)) == "backbone.6.0.weight":
        def spoil(g, leaves, go):
            g[1] = g[1].clone()
            g[1][:, :, 0, 2] = 0
            return g
        return V._WrongGradient.apply(fn, spoil, input, weight)
    if names.get(id(weight)) == "extras.0.3.0.weight":
        return V._WrongGradient.apply(fn, lambda g, leaves, go: [torch.roll(g[0], 1, 3), g[1]], input, weight)
    return depthwise_conv2d(input, weight, bias, stride, padding)


@functools.lru_cache(maxsize=None)
def _state():
    net = build_net("train", 320, 21, 1, False)
    return synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)


@functools.lru_cache(maxsize=None)
def _step(mutated=False, training=True):
    """one recorded forward_train + backward on the CPU with the stand-ins in place of the seven ops -> (finished recorder, net).
    Training mode: batch 1.  Eval mode: batch 2 on calibrated running statistics, the GPU file's eval-mode case."""
    ops = dict(STAND_INS, depthwise_conv2d=m_depthwise_conv2d) if mutated else STAND_INS
    mp = pytest.MonkeyPatch()
    try:
        for kind, fn in ops.items():
            mp.setattr(networks, kind, fn)
        mp.setattr(_lib, "require_cuda", lambda t, name="tensor": None)
        net = build_net("train", 320, 21, 1, False)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in _state().items()})
        assert net.training
        MUTATED[0] = net if mutated else None
        gen = torch.Generator().manual_seed(77)
        P = 3 * sum(f * f for f in MAPS)
        targets = tuple(torch.randn(1, P, w, generator=gen) for w in (4, 4, 21))
        x = torch.from_numpy(synth.synth_frames(1 if training else 2, SIZE, seed=SEED))
        if not training:
            W.calibrate(net, x)
        with W.Recorder(net) as rec:
            out = net.forward_train(x)
            loss = T.smooth_loss((out[0], out[2], out[3]), targets)
            loss.backward()
        assert networks.depthwise_conv2d is ops["depthwise_conv2d"], "the recorder did not restore the ops"
        rec.finish()
        return rec, net
    finally:
        MUTATED[0] = None
        mp.undo()


@pytest.fixture(scope="module", autouse=True)
def _release_the_recordings():
    yield
    _step.cache_clear()


def test_the_ops_are_restored_and_the_stages_are_the_modules_holders():
    rec, net = _step()
    assert all(getattr(networks, k) is not STAND_INS[k] for k in W.KINDS)
    kinds = [st.kind for st in rec.stages]
    assert {k: kinds.count(k) for k in W.KINDS if kinds.count(k)} == EXPECTED and "max_pool2d" not in kinds
    assert len(rec.stages) == 99 and [st.index for st in rec.stages] == list(range(99))
    first = rec.stages[0]
    assert first.name == "backbone.0.0" and first.args["stride"] == (2, 2) and "input" not in first.grad_input      # the image
    dw = [st for st in rec.stages if st.kind == W.DEPTHWISE]
    assert [st.name for st in dw] == ["backbone.%d.0" % i for i in range(1, 14)] + ["extras.0.3.0", "extras.1.3.0"]
    assert [st.args["stride"][0] for st in dw] == T.STRIDES + [2, 2]
    assert all(set(st.grad_input) == {"input"} and "bias" not in st.inputs for st in dw)
    assert set(T.bn_after_conv(_state().keys())) == set(T.CANCELLING)


def test_correct_fp32_ops_pass_every_stage():
    rec, _ = _step()
    worst = W.check_stages(rec.stages, set(T.CANCELLING))
    assert set(worst) == set(EXPECTED)
    assert all(share < 1.0 for share, _, _ in worst.values())


def test_eval_mode_batch_norm_stages_stay_inside_the_caps():
    rec, net = _step(training=False)
    assert not net.training and all(m.momentum == 0.1 for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    chosen = R.select_stages(rec.stages, "batch_norm")
    assert len(chosen) == 33 and all(st.args["training"] is False for st in chosen)
    worst = W.check_stages(rec.stages, (), "batch_norm")
    assert worst["batch_norm"][0] < 1.0


def test_depthwise_mutations_fail_at_their_stage_and_nowhere_else():
    rec, _ = _step(True)
    near = {"backbone.5.3", "backbone.5.4", "backbone.6.0", "backbone.6.1", "backbone.6.3", "extras.0.0", "extras.0.1", "extras.0.3.0",
            "extras.0.3.1", "extras.0.3.3"}
    failures = {}
    chosen = R.select_stages(rec.stages, lambda st: st.name in near)
    assert len(chosen) == len(near)
    W.check_stages(rec.stages, set(T.CANCELLING), select=lambda st: st.name in near, failures=failures)
    for name, (tensor, what) in MUTATIONS.items():
        print("%s (%s): %s" % (name, what, failures.get(name)))
        assert name in failures and tensor in failures[name], (name, what, failures.get(name))
    assert set(failures) == set(MUTATIONS), failures
