"""RefineSSD.forward_train of refinedet_vgg (bn=True): the phase-'train' outputs computed from the module's own fp32 parameters
through the library's differentiable ops (the 5x5 heads of multihead through networks.conv5x5), so that loss.backward() fills their
.grad: train.py's RefineDet loop.

Cases: use_refine with multihead (train.py's defaults --refine True --multihead True; a 4-tuple) and neither (a 2-tuple).

References.  Eval mode: oracle.net_ref.refinedet_vgg_forward(phase='train'), atol 1e-3 on every element (no deformable op, so no
exception).  Training mode: refinedet_forward of tests/_train_model_ref.py on the CPU in float64.  Inputs, the gradient rule (relative L2 per tensor,
bound 10 x the float32 yardstick's worst tensor under a cap of 0.1) and the rule for the cancelling biases are
test_gpu_train_trn.py's: 192 px (pyramid 24 / 12 / 6 / 3, P = 2295; the dense 5x5 heads run on the 3 x 3 map, the kernel larger than
the image), one image of frame seed 5 for the float64 tests (worst float32 yardstick over torch's two evaluations, measured on the CPU:
7.4e-3 with refine and multihead, 5.6e-3 without), two for eval mode and the drop-in steps.  Train-mode outputs: 1e-4 max(1, max|ref|).
Fixtures and checks: tests/_train_model_harness.py.
"""
import numpy as np
import pytest
import torch

import _train_model_harness as H
import _train_model_ref as T
from oracle import net_ref
from tdrn_amd.layers import MultiBoxLoss, RefineMultiBoxLoss
from tdrn_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = H.DEV
torch.set_num_threads(min(16, torch.get_num_threads()))

SIZE, MAPS = 192, (24, 12, 6, 3)
P = H.priors_count(MAPS)
LR = 0.01
SEED, STATE_SEED, TARGET_SEED = 5, 0, 77
CAP = 0.1                                                # on 10 x yardstick, inclusive (test_gpu_train_trn.py's)
CASES = [(True, True), (False, False)]                   # (use_refine, multihead)
CASE = pytest.mark.parametrize("use_refine,multihead", CASES, ids=["refine-multihead", "plain"])


def _build(use_refine, multihead):
    return H.build(H.refinedet(use_refine, multihead))


def _state(use_refine, multihead):
    return H.state(H.refinedet(use_refine, multihead), STATE_SEED)


def _net(use_refine, multihead):
    return H.net(H.refinedet(use_refine, multihead), STATE_SEED)


def _frames(B):
    return H.frames(B, SIZE, SEED)


def _targets(use_refine):
    return H.targets(P, (4, 4, 21) if use_refine else (4, 21), TARGET_SEED)


def _reference(use_refine, multihead, dtype, onednn=True):
    """one training step of the restatement on the CPU, computed once and never changed.  onednn=False: torch's other float32
    evaluation of the same ops"""
    return H.reference(H.refinedet(use_refine, multihead), STATE_SEED, SEED, SIZE, MAPS, TARGET_SEED, dtype, 1, LR, onednn)[0][0]


_tensors = H.tensors


def _ours(net, use_refine, compute="fp32"):
    out = net.forward_train(torch.from_numpy(_frames(1)).to(DEV), compute)
    return out, T.smooth_loss(_tensors(out), _targets(use_refine))


@CASE
def test_eval_mode_matches_the_oracle(use_refine, multihead):
    B = 2
    net = _net(use_refine, multihead).eval()
    before = H.buffers(net)
    x = _frames(B)
    with torch.no_grad():
        out = net.forward_train(torch.from_numpy(x).to(DEV))
    want = net_ref.refinedet_vgg_forward(_state(use_refine, multihead), x, 21, use_refine, True, multihead, phase="train")
    assert len(out) == len(want) == (4 if use_refine else 2)
    if use_refine:
        assert out[1] is None and want[1] is None
    shapes = ([(B, P, 4)] if use_refine else []) + [(B, P, 4), (B, P, 21)]
    assert [tuple(t.shape) for t in _tensors(out)] == shapes
    d = [float((g.cpu() - r).abs().max()) for g, r in zip(_tensors(out), _tensors(want))]
    print("eval refine=%s multihead=%s: max|d| %r (atol 1e-3)" % (use_refine, multihead, d))
    assert all(v <= 1e-3 for v in d)
    after = H.buffers(net)
    assert all(torch.equal(before[k], after[k]) for k in before), "eval mode changed a running buffer"
    net.phase = "test"                               # forward_train gives the phase-'train' outputs whatever the phase
    out = net.forward_train(torch.from_numpy(x).to(DEV))
    assert all(t.requires_grad for t in _tensors(out)) and tuple(out[-1].shape) == (B, P, 21)


@CASE
def test_train_mode_forward_and_running_statistics(use_refine, multihead):
    net = _net(use_refine, multihead)
    assert net.training
    with torch.no_grad():
        out, _ = _ours(net, use_refine)
    ref = _reference(use_refine, multihead, torch.float64)
    d = [float((g.cpu().double() - r).abs().max()) for g, r in zip(_tensors(out), ref["outs"])]
    bounds = [H.train_atol(r) for r in ref["outs"]]
    print("train refine=%s multihead=%s: max|d| %r, bounds 1e-4 max(1, max|ref|) %r" % (use_refine, multihead, d, bounds))
    assert len(d) == len(ref["outs"]) and all(v <= b for v, b in zip(d, bounds))
    H.running_statistics_check("refine=%s multihead=%s" % (use_refine, multihead), H.buffers(net), ref["buffers"])


@CASE
def test_train_mode_gradients(use_refine, multihead):
    net = _net(use_refine, multihead)
    _, loss = _ours(net, use_refine)
    loss.backward()
    ref = _reference(use_refine, multihead, torch.float64)
    yards = [_reference(use_refine, multihead, torch.float32, onednn) for onednn in (True, False)]
    grads = {n: p.grad for n, p in net.named_parameters()}
    assert set(grads) == set(ref["grads"])
    if multihead:
        assert sum(n.startswith("odm_loc_2") or n.startswith("odm_conf_2") for n in grads) == 16
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"]))
    H.gradient_check("refinedet refine=%s multihead=%s" % (use_refine, multihead), grads, ref, yards, (), CAP, True,
                     H.AbsGoRule(sorted(ref["abs_go"]), each=False))


def _drop_in_step(net, use_refine, x, targets, priors, compute, opt):
    """train.py:257-268: its two loss forms"""
    opt.zero_grad()
    out = net.forward_train(x, compute)
    if use_refine:
        arm_criterion = RefineMultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, device=DEV, only_loc=True)
        criterion = RefineMultiBoxLoss(21, 0.5, True, 0, True, 3, 0.5, False, device=DEV)
        loss_arm_l = arm_criterion(out[0], priors, targets)
        loss_l, loss_c = criterion(out[2:], priors, targets, arm_data=out[:2])
        losses = (loss_arm_l, loss_l, loss_c)
    else:
        losses = MultiBoxLoss(21, 0.5, True, 0, True, 3, 0.5, False, device=DEV)(out, priors, targets)
    sum(losses).backward()
    return out, tuple(float(v.detach()) for v in losses)


@CASE
def test_drop_in_training_step(use_refine, multihead):
    import _loss_ref as R
    B = 2
    net = _net(use_refine, multihead)
    priors = H.priors(SIZE, MAPS)
    targets = [torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in R.synth_targets(synth._rng("train_refinedet_dropin", 0), B, 3, 20, 21)]
    x = torch.from_numpy(_frames(B)).to(DEV)
    step = lambda n, compute, opt: _drop_in_step(n, use_refine, x, targets, priors, compute, opt)
    H.drop_in_fp32(net, lambda n: n(x), step, torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4))
    with torch.no_grad():
        ref = _net(use_refine, multihead).forward_train(x)
    H.drop_in_16bit(lambda: _net(use_refine, multihead), step, ref, lambda compute, losses, drift: print(
        "drop-in refine=%s multihead=%s %s: losses %r, output drift against fp32 %r" % (use_refine, multihead, compute, losses, drift)))


def test_cpu_input_raises_and_the_engine_is_left_alone():
    net = _build(True, True)
    with pytest.raises(NotImplementedError):
        net.forward_train(torch.zeros(1, 3, SIZE, SIZE))
    assert net._engine is None                                  # forward_train builds no engine
    with pytest.raises(ValueError):
        net.to(DEV).forward_train(torch.zeros(3, SIZE, SIZE, device=DEV))
    assert MAPS[-1] < 5                                         # the 5x5 heads' kernel is larger than the last map
