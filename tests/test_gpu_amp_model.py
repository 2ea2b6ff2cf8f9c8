"""One fp16 training step of dualrefinedet_vggbn with the scaler in it, train.py's protocol:
forward_train(x, "fp16", resident=True) -> RefineMultiBoxLoss (ARM only_loc + ODM) -> scaler.scale(loss).backward() ->
scaler.step(SGD) -> scaler.update(), at the smallest input and batch of the model-level training tests (192 px, one frame, single
head; tests/test_gpu_train_resident.py).  No tolerance: the parameters are finite and have moved and nothing was skipped; or, with
one inf in the frame, every parameter keeps every byte and one skipped step is counted."""
import numpy as np
import pytest
import torch

import _loss_ref
import _train_model_harness as H
from tdrn_amd.amp import GradScaler
from tdrn_amd.layers import RefineMultiBoxLoss
from tdrn_amd.optim import SGD
from tdrn_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = H.DEV
SIZE, MAPS = 192, (24, 12, 6, 3)
SEED, STATE_SEED = 5, 0


def _step(poison):
    """-> (net, the parameters before the step, scaler)"""
    net = H.net(H.drn_vgg(True, False), STATE_SEED)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    priors = H.priors(SIZE, MAPS)
    targets = [torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in _loss_ref.synth_targets(synth._rng("amp_model", 0), 1, 3, 20, 21)]
    x = torch.from_numpy(H.frames(1, SIZE, SEED)).to(DEV)
    if poison:
        x[0, 1, SIZE // 2, SIZE // 3] = float("inf")
    arm_criterion = RefineMultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, device=DEV, only_loc=True)
    criterion = RefineMultiBoxLoss(21, 0.5, True, 0, True, 3, 0.5, False, device=DEV)
    opt = SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    scaler = GradScaler()
    opt.zero_grad()
    out = net.forward_train(x, "fp16", resident=True)
    loss_arm_l = arm_criterion(out[0], priors, targets)
    loss_l, loss_c = criterion(out[2:], priors, targets, arm_data=out[:2])
    scaler.scale(loss_arm_l + loss_l + loss_c).backward()
    worst = max(float(p.grad.abs().max()) for p in net.parameters() if p.grad is not None)
    print("amp model step (poison=%s): scale %g, largest |scaled gradient| %.3e" % (poison, scaler.get_scale(), worst))
    scaler.step(opt)
    state_after_step = scaler._state.tolist()
    scaler.update()
    return net, before, scaler, state_after_step


def test_a_scaled_fp16_step_moves_the_net_and_skips_nothing():
    net, before, scaler, after_step = _step(False)
    assert after_step == [65536.0, 0.0, 0.0, 0.0], "found_inf after the step"
    assert scaler._state.tolist() == [65536.0, 1.0, 0.0, 0.0] and scaler.skipped_steps() == 0
    for n, p in net.named_parameters():
        assert bool(torch.isfinite(p).all()), n
    first = next(n for n, p in net.named_parameters() if p.dim() == 4)     # the first trunk conv's weight
    assert not torch.equal(dict(net.named_parameters())[first].detach(), before[first]), first + " did not move"


def test_an_inf_in_the_frame_leaves_every_parameter_alone_and_counts_one_skip():
    net, before, scaler, after_step = _step(True)
    assert after_step == [65536.0, 0.0, 1.0, 0.0], "found_inf after the step"
    for n, p in net.named_parameters():
        assert torch.equal(p.detach().reshape(-1).view(torch.uint8), before[n].reshape(-1).view(torch.uint8)), n
    assert scaler._state.tolist() == [32768.0, 0.0, 0.0, 1.0] and scaler.skipped_steps() == 1 and scaler.get_scale() == 32768.0
