"""RefineSSD.forward_train of dualrefinedet_mobilenet: the phase-'train' outputs computed from the module's own fp32 parameters
through the library's differentiable ops (the depthwise 3x3 conv of conv_dw among them), so that loss.backward() fills their .grad.

References.  Eval mode: oracle.net_ref.drn_mobilenet_forward(phase='train') with test_gpu_net.py's rule (atol 1e-3; behind the
deformable heads every prior row but those net_ref.border_rows finds on a sampling discontinuity, at most 30 of them; the oracle
alone gives 0 such rows at this input).  Training mode: drn_forward of tests/_train_model_ref.py, the same walk on torch's functional
ops with F.batch_norm(training=True), on the CPU in float64.  Fixtures and checks: tests/_train_model_harness.py.

Inputs: test_gpu_train_net.py's (single head 192 px, pyramid 24 / 12 / 6 / 3, P = 2295; multihead 320 px).  The float64 tests run
ONE image of frame seed 4; eval mode and the drop-in step run two of frame seed 5.

Gradients are compared per tensor by relative L2 against float64.  The check is coarse here: thirty-three BatchNorms with ReLU
decisions make this net so sensitive that torch's own float32 run of the restatement differs from float64 by 7.3e-3 in its worst
tensor for one 192 px image of frame seed 4 (1.45e-2 at seed 5, 3.6e-2 at seed 7; two images roughly double it), so the VGG test's
cap of 5e-2 on 10 x yardstick cannot be carried over.  Bound: 10 x the yardstick's worst tensor, computed by the test itself, under
the condition that it stays below 0.1 (else the input must change, not the factor): a missing layer, a wrong stride or a lost factor
gives errors >= 0.1.  The sharp gate is tests/test_gpu_train_stages_mobilenet.py.  The two conv biases in front of a training-mode
BatchNorm (extras.0.0.bias, extras.1.0.bias) have a float64 gradient of 1e-17: they are judged by |g| <= 2e-6 sum|grad_output| of
their conv, per channel, as tests/_train_stage_ref.py judges a cancelling sum.
"""
import numpy as np
import pytest
import torch

import _train_model_harness as H
import _train_model_ref as T
from oracle import net_ref
from tdrn_amd.layers import RefineMultiBoxLoss
from tdrn_amd.model.dualrefinedet_mobilenet import build_net
from tdrn_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = H.DEV
torch.set_num_threads(min(16, torch.get_num_threads()))

CONFIG = {False: (192, (24, 12, 6, 3)), True: (320, (40, 20, 10, 5))}
LR, STEPS = 0.01, 3
SEED64, SEED = 4, 5            # frame seeds: the float64 tests' one image; eval mode's and the drop-in step's two
STATE_SEED, TARGET_SEED = 0, 77
CAP = 0.1                      # on 10 x yardstick, strict (header)
IDS = {False: "singlehead", True: "multihead"}
MH = pytest.mark.parametrize("mh", [False, True], ids=lambda v: IDS[v])


def _priors_count(mh):
    return H.priors_count(CONFIG[mh][1])


def _state(mh):
    return H.state(H.drn_mobilenet(mh), STATE_SEED)


def _net(mh):
    return H.net(H.drn_mobilenet(mh), STATE_SEED)


def _frames(mh, B, seed):
    return H.frames(B, CONFIG[mh][0], seed)


def _targets(mh):
    return H.targets(_priors_count(mh), (4, 4, 21), TARGET_SEED)


def _reference(mh, dtype):
    """the restatement's SGD run on the CPU, computed once and never changed: STEPS steps for the single-head net (its first step
    serves the forward and gradient tests), one step for the other"""
    return H.reference(H.drn_mobilenet(mh), STATE_SEED, SEED64, *CONFIG[mh], TARGET_SEED, dtype, 1 if mh else STEPS, LR, True)


def _ours(net, mh, compute="fp32"):
    x = torch.from_numpy(_frames(mh, 1, SEED64)).to(DEV)
    out = net.forward_train(x, compute)
    return out, T.smooth_loss((out[0], out[2], out[3]), _targets(mh))


@MH
def test_eval_mode_matches_the_oracle(mh):
    net = _net(mh).eval()
    before = H.buffers(net)
    assert len(before) == 3 * 33
    x = _frames(mh, 2, SEED)
    with torch.no_grad():
        out = net.forward_train(torch.from_numpy(x).to(DEV))
    assert len(out) == 4 and out[1] is None
    B, P = 2, _priors_count(mh)
    assert tuple(out[0].shape) == (B, P, 4) and tuple(out[2].shape) == (B, P, 4) and tuple(out[3].shape) == (B, P, 21)
    taps = {}
    r_arm, _, r_odm, r_conf = net_ref.drn_mobilenet_forward(_state(mh), x, 21, mh, phase="train", taps=taps)
    allowed = net_ref.border_rows(taps, mh)
    d_arm = float((out[0].cpu() - r_arm).abs().max())
    bad_odm, d_odm = H.rows_off(out[2], r_odm, allowed, 1e-3)
    bad_conf, d_conf = H.rows_off(out[3], r_conf, allowed, 1e-3)
    print("eval %s: max|d| arm %.3e odm %.3e conf %.3e (atol 1e-3), rows on a discontinuity %d" % (IDS[mh], d_arm, d_odm, d_conf, int(allowed.sum())))
    assert d_arm <= 1e-3 and bad_odm == 0 and bad_conf == 0
    after = H.buffers(net)
    assert all(torch.equal(before[k], after[k]) for k in before), "eval mode changed a running buffer"
    # with an autograd graph when asked for one, in eval mode too
    out = net.forward_train(torch.from_numpy(x).to(DEV))
    assert out[0].requires_grad and out[2].requires_grad and out[3].requires_grad


@MH
def test_train_mode_forward_and_running_statistics(mh):
    net = _net(mh)
    assert net.training
    with torch.no_grad():
        out, _ = _ours(net, mh)
    ref = _reference(mh, torch.float64)[0][0]
    allowed = net_ref.border_rows(ref["taps"], mh)
    d_arm = float((out[0].cpu().double() - ref["outs"][0]).abs().max())
    bad_odm, d_odm = H.rows_off(out[2], ref["outs"][1], allowed, 1e-3)
    bad_conf, d_conf = H.rows_off(out[3], ref["outs"][2], allowed, 1e-3)
    print("train %s: max|d| arm %.3e odm %.3e conf %.3e (atol 1e-3), rows on a discontinuity %d" % (IDS[mh], d_arm, d_odm, d_conf, int(allowed.sum())))
    assert out[1] is None and d_arm <= 1e-3 and bad_odm == 0 and bad_conf == 0
    H.running_statistics_check(IDS[mh], H.buffers(net), ref["buffers"])


def test_train_mode_gradients():
    mh = False
    net = _net(mh)
    _, loss = _ours(net, mh)
    loss.backward()
    ref = _reference(mh, torch.float64)[0][0]
    yard = _reference(mh, torch.float32)[0][0]
    grads = {n: p.grad for n, p in net.named_parameters()}
    assert set(grads) == set(ref["grads"]) and set(T.CANCELLING) <= set(grads) and set(ref["abs_go"]) == set(T.CANCELLING)
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"]))
    H.gradient_check("", grads, ref, [yard], (), CAP, False, H.AbsGoRule(T.CANCELLING, each=True))


def test_short_sgd_run_follows_float64():
    """Three plain-SGD steps on the smooth loss.  Losses only (test_gpu_train_net.py says why no parameter comparison can hold):
    the losses fall, in ours and in float64, and ours stays within 10 x the float32 yardstick's own distance from float64 at every
    step (floor: 1e-5 of the loss, the float32 evaluation of its three means)."""
    mh = False
    want = [l["loss"] for l in _reference(mh, torch.float64)[0]]
    yard = [l["loss"] for l in _reference(mh, torch.float32)[0]]
    losses = H.short_run(_net(mh), lambda net: _ours(net, mh)[1], STEPS, LR)
    H.short_run_check(losses, want, yard, STEPS)


def _drop_in_step(net, mh, compute, targets, priors, opt):
    x = torch.from_numpy(_frames(mh, 2, SEED)).to(DEV)
    arm_criterion = RefineMultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, device=DEV, only_loc=True)
    criterion = RefineMultiBoxLoss(21, 0.5, True, 0, True, 3, 0.5, False, device=DEV)
    opt.zero_grad()
    out = net.forward_train(x, compute)
    loss_arm_l = arm_criterion(out[0], priors, targets)
    loss_l, loss_c = criterion(out[2:], priors, targets, arm_data=out[:2])
    loss = loss_arm_l + loss_l + loss_c
    loss.backward()
    return out, tuple(float(v.detach()) for v in (loss_arm_l, loss_l, loss_c))


@MH
def test_drop_in_training_step(mh):
    """train.py's protocol: forward_train -> RefineMultiBoxLoss (ARM only_loc + ODM) -> backward -> one SGD step"""
    import _loss_ref as R
    B = 2
    net = _net(mh)
    priors = H.priors(*CONFIG[mh])
    targets = [torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in R.synth_targets(synth._rng("train_net_dropin", 0), B, 3, 20, 21)]
    x = torch.from_numpy(_frames(mh, B, SEED)).to(DEV)
    step = lambda n, compute, opt: _drop_in_step(n, mh, compute, targets, priors, opt)
    H.drop_in_fp32(net, lambda n: n(x), step, torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9))
    with torch.no_grad():
        ref = _net(mh).forward_train(x)
    H.drop_in_16bit(lambda: _net(mh), step, ref, lambda compute, losses, drift: print(
        "drop-in %s %s: losses %r, output drift against fp32: arm %.3e odm %.3e conf %.3e" % (IDS[mh], compute, losses, *drift)))


def test_cpu_input_raises_and_the_engine_is_left_alone():
    net = build_net("train", 320, 21, 1, False)
    with pytest.raises(NotImplementedError):
        net.forward_train(torch.zeros(1, 3, 192, 192))
    assert net._engine is None                                  # forward_train builds no engine
    with pytest.raises(ValueError):
        net.to(DEV).forward_train(torch.zeros(3, 192, 192, device=DEV))
    assert net._engine is None
