"""RefineSSD.forward_train of refinedet_vgg (bn=True): the phase-'train' outputs computed from the module's own fp32 parameters
through the library's differentiable ops (the 5x5 heads of multihead through networks.conv5x5), so that loss.backward() fills their
.grad: train.py's RefineDet loop.

Cases: use_refine with multihead (train.py's defaults --refine True --multihead True; a 4-tuple) and neither (a 2-tuple).

References.  Eval mode: oracle.net_ref.refinedet_vgg_forward(phase='train'), atol 1e-3 on every element (no deformable op, so no
exception).  Training mode: tests/_train_refinedet_ref.py on the CPU in float64.  Inputs, the gradient rule (relative L2 per tensor,
bound 10 x the float32 yardstick's worst tensor under a cap of 0.1) and the rule for the cancelling biases are
test_gpu_train_trn.py's: 192 px (pyramid 24 / 12 / 6 / 3, P = 2295; the dense 5x5 heads run on the 3 x 3 map, the kernel larger than
the image), one image of frame seed 5 for the float64 tests (worst float32 yardstick over torch's two evaluations, measured on the CPU:
7.4e-3 with refine and multihead, 5.6e-3 without), two for eval mode and the drop-in steps.  Train-mode outputs: 1e-4 max(1, max|ref|).
"""
import functools

import numpy as np
import pytest
import torch

import _train_refinedet_ref as T
from oracle import net_ref
from tdrn_amd.layers import MultiBoxLoss, RefineMultiBoxLoss
from tdrn_amd.model.refinedet_vgg import build_net
from tdrn_amd.utils import synth
from test_gpu_train_trn import DEV, LR, MAPS, P, SIZE, _buffers, _gradient_check, _priors, _train_atol

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

SEED = 5
CASES = [(True, True), (False, False)]                   # (use_refine, multihead)
CASE = pytest.mark.parametrize("use_refine,multihead", CASES, ids=["refine-multihead", "plain"])


def _build(use_refine, multihead):
    return build_net("train", 320, 21, use_refine, 1024, True, multihead)


@functools.lru_cache(maxsize=None)
def _state(use_refine, multihead):
    return synth.synth_state_dict({k: tuple(v.shape) for k, v in _build(use_refine, multihead).state_dict().items()}, 0)


def _net(use_refine, multihead):
    net = _build(use_refine, multihead)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in _state(use_refine, multihead).items()})
    return net.to(DEV)


@functools.lru_cache(maxsize=None)
def _frames(B):
    return synth.synth_frames(B, SIZE, seed=SEED)


@functools.lru_cache(maxsize=None)
def _targets(use_refine):
    gen = torch.Generator().manual_seed(77)
    return tuple(torch.randn(1, P, w, generator=gen) for w in ((4, 4, 21) if use_refine else (4, 21)))


@functools.lru_cache(maxsize=None)
def _reference(use_refine, multihead, dtype, onednn=True):
    """one training step of the restatement on the CPU, computed once and never changed.  onednn=False: torch's other float32
    evaluation of the same ops"""
    with torch.backends.mkldnn.flags(enabled=onednn):
        return T.sgd_run(_state(use_refine, multihead), _frames(1), _targets(use_refine), use_refine, multihead, dtype, 1, LR)[0][0]


def _tensors(out):
    return tuple(t for t in out if t is not None)


def _ours(net, use_refine, compute="fp32"):
    out = net.forward_train(torch.from_numpy(_frames(1)).to(DEV), compute)
    return out, T.smooth_loss(_tensors(out), _targets(use_refine))


@CASE
def test_eval_mode_matches_the_oracle(use_refine, multihead):
    B = 2
    net = _net(use_refine, multihead).eval()
    before = _buffers(net)
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
    after = _buffers(net)
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
    bounds = [_train_atol(r) for r in ref["outs"]]
    print("train refine=%s multihead=%s: max|d| %r, bounds 1e-4 max(1, max|ref|) %r" % (use_refine, multihead, d, bounds))
    assert len(d) == len(ref["outs"]) and all(v <= b for v, b in zip(d, bounds))
    worst = 0.0
    for k, v in _buffers(net).items():
        r = ref["buffers"][k]
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1 and int(r) == 1, k
            continue
        dd, bound = float((v.cpu().double() - r).abs().max()), 1e-4 * max(1.0, float(r.abs().max()))
        worst = max(worst, dd / bound)
        assert dd <= bound, (k, dd, bound)
    print("train refine=%s multihead=%s: running statistics, worst |d| / bound %.3e" % (use_refine, multihead, worst))


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
    _gradient_check("refinedet refine=%s multihead=%s" % (use_refine, multihead), grads, ref, yards)


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
    priors = _priors()
    targets = [torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in R.synth_targets(synth._rng("train_refinedet_dropin", 0), B, 3, 20, 21)]
    x = torch.from_numpy(_frames(B)).to(DEV)
    with torch.no_grad():
        before = [t.clone() for t in _tensors(net(x))]
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    out32, losses = _drop_in_step(net, use_refine, x, targets, priors, "fp32", opt)
    assert all(np.isfinite(l) for l in losses), losses
    for n, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    opt.step()
    with torch.no_grad():
        after = [t.clone() for t in _tensors(net(x))]
    # the engine re-packed by itself: no repack() call between the step and net(x)
    assert all(float((a - b).abs().max()) > 0 for a, b in zip(before, after))
    # the 16-bit compute types: the same pass is finite; their drift against fp32 is reported, not gated
    with torch.no_grad():
        ref = _tensors(_net(use_refine, multihead).forward_train(x))
    for compute in ("bf16", "fp16"):
        fresh = _net(use_refine, multihead)
        out, losses = _drop_in_step(fresh, use_refine, x, targets, priors, compute, torch.optim.SGD(fresh.parameters(), lr=1e-3))
        assert all(np.isfinite(l) for l in losses), (compute, losses)
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in fresh.parameters()), compute
        print("drop-in refine=%s multihead=%s %s: losses %r, output drift against fp32 %r" % (
            use_refine, multihead, compute, losses, [float((a.detach() - b).abs().max()) for a, b in zip(_tensors(out), ref)]))


def test_cpu_input_raises_and_the_engine_is_left_alone():
    net = _build(True, True)
    with pytest.raises(NotImplementedError):
        net.forward_train(torch.zeros(1, 3, SIZE, SIZE))
    assert net._engine is None                                  # forward_train builds no engine
    with pytest.raises(ValueError):
        net.to(DEV).forward_train(torch.zeros(3, SIZE, SIZE, device=DEV))
    assert MAPS[-1] < 5                                         # the 5x5 heads' kernel is larger than the last map
