"""The resident training path end to end: a conv-BN-ReLU-conv-BN-ReLU-pool chain through the Python ops against the same sequence entry
by entry through the C ABI, bit for bit; forward_train(x, compute, resident=True) of dualrefinedet_vggbn; and one captured training
step.

Net test.  The yardstick is the existing path, not the code under test: with the float64 restatement of tests/_train_model_ref.py,
the relative L2 distance of arm_loc to float64 under resident=True is at most 2 x that of resident=False at the same compute type, both
computed here, with BatchNorm and without (that module's arm_loc restates the part of the net in front of the heads for both).
Why 2: the resident path rounds twice per layer (the conv output and the BatchNorm output) where the existing path
rounds once (the conv's input); two independent errors of equal size give sqrt(2), and 2 leaves room.  arm_loc is gated because it sits
in front of the discontinuous deformable sampling; odm_loc and conf, behind it, are printed.  Frame seed 5 at 192 px: the test
computes the float32 restatement on the CPU beside the float64 one and asserts that its arm_loc distance (5.7e-6 with BatchNorm, 6.8e-7
without) is at most a hundredth of the existing 16-bit path's, so no ReLU or max-pool decision flip dominates that distance.
"""
import functools

import numpy as np
import pytest
import torch

import _train_model_harness as H
import _train_model_ref as T
from tdrn_amd.layers import RefineMultiBoxLoss
from tdrn_amd.layers.box_utils import PackedTargets
from tdrn_amd.model import networks
from tdrn_amd.model.dualrefinedet_mobilenet import build_net as build_mobilenet
from tdrn_amd.optim import SGD
from tdrn_amd.utils import synth

from _conv_train_harness import DEV
from _nhwc_harness import (ConvAbi, TYPES, bn_backward, bn_forward, exact, pool_backward, pool_forward, raw_equal, resident)

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
SIZE, MAPS = 192, (24, 12, 6, 3)
PRIORS = H.priors_count(MAPS)
SEED, STATE_SEED, TARGET_SEED = 5, 0, 77


# ---- chain ---------------------------------------------------------------------------------------------------------------------------
def test_chain_python_ops_equal_the_entries_bit_for_bit():
    mode, eps, mom = "bf16", 1e-5, 0.1
    g = torch.Generator().manual_seed(17)
    x = exact(torch.randn(2, 64, 12, 10, generator=g), mode)
    w1, b1 = torch.randn(128, 64, 3, 3, generator=g) / 24, torch.randn(128, generator=g)
    w2, b2 = torch.randn(64, 128, 3, 3, generator=g) / 34, torch.randn(64, generator=g)
    g1, be1, g2, be2 = (0.5 + torch.rand(128, generator=g), 0.1 * torch.randn(128, generator=g), 0.5 + torch.rand(64, generator=g),
                        0.1 * torch.randn(64, generator=g))
    go = exact(torch.randn(2, 64, 6, 5, generator=g), mode)
    dev = lambda *ts: [t.to(DEV) for t in ts]

    # the Python ops under autograd
    xr = resident(x, mode).requires_grad_(True)
    P = [t.requires_grad_(True) for t in dev(w1, b1, g1, be1, w2, b2, g2, be2)]
    rm1, rv1, rm2, rv2 = torch.zeros(128, device=DEV), torch.ones(128, device=DEV), torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
    t = networks.conv2d_nhwc(xr, P[0], P[1], 1, 1)
    t = networks.batch_norm_nhwc(t, rm1, rv1, P[2], P[3], True, mom, eps, relu=True)
    t = networks.conv2d_nhwc(t, P[4], P[5], 1, 1)
    t = networks.batch_norm_nhwc(t, rm2, rv2, P[6], P[7], True, mom, eps, relu=True)
    y = networks.max_pool2d_nhwc(t, 2, 2, 0, False)
    y.backward(resident(go, mode))

    # entry by entry
    w1d, b1d, g1d, be1d, w2d, b2d, g2d, be2d = dev(w1, b1, g1, be1, w2, b2, g2, be2)
    xa, goa = resident(x, mode), resident(go, mode)
    cl = lambda n, c, h, w: torch.empty((n, c, h, w), dtype=TYPES[mode], device=DEV).contiguous(memory_format=torch.channels_last)
    c1 = ConvAbi((2, 64, 12, 10, 128, 3, 3, 1, 1, 1, 1, 1, 1), mode)
    c2 = ConvAbi((2, 128, 12, 10, 64, 3, 3, 1, 1, 1, 1, 1, 1), mode)
    a1 = c1.forward(xa, w1d, b1d, cl(2, 128, 12, 10))
    n1, sm1, si1 = cl(2, 128, 12, 10), torch.empty(128, device=DEV), torch.empty(128, device=DEV)
    qm1, qv1 = torch.zeros(128, device=DEV), torch.ones(128, device=DEV)
    bn_forward(a1, g1d, be1d, qm1, qv1, n1, sm1, si1, True, mom, eps, True, mode)
    a2 = c2.forward(n1, w2d, b2d, cl(2, 64, 12, 10))
    n2, sm2, si2 = cl(2, 64, 12, 10), torch.empty(64, device=DEV), torch.empty(64, device=DEV)
    qm2, qv2 = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
    bn_forward(a2, g2d, be2d, qm2, qv2, n2, sm2, si2, True, mom, eps, True, mode)
    ya, code = cl(2, 64, 6, 5), torch.empty((2, 6, 5, 64), dtype=torch.uint8, device=DEV)
    pool_forward(n2, ya, code, (2, 2, 0, 0), mode)
    d_n2 = cl(2, 64, 12, 10)
    pool_backward(goa, code, d_n2, (2, 2, 0, 0), mode)
    z = lambda t: torch.zeros_like(t)
    d_a2, gg2, gbe2 = cl(2, 64, 12, 10), z(g2d), z(be2d)
    bn_backward(a2, d_n2, g2d, be2d, sm2, si2, d_a2, gg2, gbe2, True, True, 1.0, mode)
    d_n1 = c2.backward_input(d_a2, w2d, cl(2, 128, 12, 10))
    gw2, gb2 = c2.backward_parameters(n1, d_a2, z(w2d), z(b2d))
    d_a1, gg1, gbe1 = cl(2, 128, 12, 10), z(g1d), z(be1d)
    bn_backward(a1, d_n1, g1d, be1d, sm1, si1, d_a1, gg1, gbe1, True, True, 1.0, mode)
    d_x = c1.backward_input(d_a1, w1d, cl(2, 64, 12, 10))
    gw1, gb1 = c1.backward_parameters(xa, d_a1, z(w1d), z(b1d))
    torch.cuda.synchronize()

    assert raw_equal(y.detach(), ya), "output"
    assert raw_equal(xr.grad, d_x), "grad_input"
    for name, p, want in zip(("w1", "b1", "gamma1", "beta1", "w2", "b2", "gamma2", "beta2"), P, (gw1, gb1, gg1, gbe1, gw2, gb2, gg2, gbe2)):
        assert p.grad is not None and torch.equal(p.grad, want), name
    for got, want in ((rm1, qm1), (rv1, qv1), (rm2, qm2), (rv2, qv2)):
        assert torch.equal(got, want)


# ---- net -----------------------------------------------------------------------------------------------------------------------------
def _state(bn):
    return H.state(H.drn_vgg(bn, False), STATE_SEED)


def _net(bn=True):
    return H.net(H.drn_vgg(bn, False), STATE_SEED)


def _frames(B=1):
    return H.frames(B, SIZE, SEED)


def _float64_outputs():
    """the float64 restatement's training-mode forward on the CPU, computed once (and shared with test_gpu_train_deform_ts.py)"""
    return H.forward_outputs(H.drn_vgg(True, False), STATE_SEED, SEED, SIZE, torch.float64)


def _targets():
    return H.targets(PRIORS, (4, 4, 21), TARGET_SEED)


def _step(net, compute, resident_path):
    """forward_train, the smooth loss, backward -> the outputs"""
    x = torch.from_numpy(_frames()).to(DEV)
    out = net.forward_train(x, compute, resident=resident_path)
    T.smooth_loss((out[0], out[2], out[3]), _targets()).backward()
    return out


@functools.lru_cache(maxsize=None)
def _arm_loc_reference(bn):
    """arm_loc of the CPU restatement (T.arm_loc: the trunk and the ARM loc heads alone) in float64 and float32, computed once ->
    (float64 arm_loc, the float32 one's relative L2 distance to it)"""
    a64 = T.arm_loc(_state(bn), _frames(), bn, torch.float64)
    a32 = T.arm_loc(_state(bn), _frames(), bn, torch.float32)
    return a64, float((a32.double() - a64).norm() / a64.norm())


def test_bn_restatement_is_the_existing_one():
    """(no device work) with bn=True the no_grad walk of the trunk and the ARM loc heads alone gives the full forward's arm_loc, exactly"""
    assert torch.equal(_arm_loc_reference(True)[0], _float64_outputs()[0])


@pytest.mark.parametrize("bn,compute", [(True, "bf16"), (True, "fp16"), (False, "bf16"), (False, "fp16")],
                         ids=["bn-bf16", "bn-fp16", "plain-bf16", "plain-fp16"])
def test_net_resident_against_the_existing_path(bn, compute):
    """shapes, None, finite gradients, num_batches_tracked, net(x) after a step: every variant.  The arm_loc gate: bf16 with and
    without BatchNorm (what the issue sets); fp16 is printed."""
    rel = lambda got, ref: float((got.detach().cpu().double() - ref).norm() / ref.norm())
    a64, d32 = _arm_loc_reference(bn)
    plain, res = _net(bn), _net(bn)
    assert res.training
    x = torch.from_numpy(_frames()).to(DEV)
    with torch.no_grad():
        before = [t.clone() for t in res(x) if t is not None]
    out_plain = _step(plain, compute, False)
    out_res = _step(res, compute, True)
    H.plumbing(res, out_res, plain, PRIORS, counters=True, exact=False)
    d_plain, d_res = rel(out_plain[0], a64), rel(out_res[0], a64)
    print("bn=%s %s, arm_loc relative L2 to float64: resident=False %.4e, resident=True %.4e (ratio %.3f); float32 restatement %.3e"
          % (bn, compute, d_plain, d_res, d_res / d_plain, d32))
    if bn:
        ref = _float64_outputs()
        print("  behind the deformable heads (not gated), odm_loc / conf: resident=False %.4e / %.4e, resident=True %.4e / %.4e"
              % (rel(out_plain[2], ref[1]), rel(out_plain[3], ref[2]), rel(out_res[2], ref[1]), rel(out_res[3], ref[2])))
    # the precondition of the gate: this frame seed puts no ReLU / max-pool decision flip into the existing path's own distance --
    # float32 arithmetic on the same walk stays a hundred times closer to float64 than the 16-bit path is
    assert d32 <= 0.01 * d_plain, (d32, d_plain)
    if compute == "bf16":
        assert d_res <= 2 * d_plain, (d_res, d_plain)
    H.moves_after_a_step(res, before, x)


def test_resident_switch_refusals_and_default():
    net = _net()
    x = torch.from_numpy(_frames()).to(DEV)
    with pytest.raises(ValueError):
        net.forward_train(x, "fp32", resident=True)
    with pytest.raises(ValueError):
        net.forward_train(x, resident=True)
    # a refused call has no side effect: the engine's packed weights are not marked stale
    with torch.no_grad():
        net(x)
    assert not net._dirty
    with pytest.raises(ValueError):
        net.forward_train(x, "fp32", resident=True)
    assert not net._dirty
    mob = build_mobilenet("train", 320, 21)
    with pytest.raises(NotImplementedError):
        mob.to(DEV).forward_train(x, "bf16", resident=True)
    # resident=False is the call that omits the argument, bit for bit
    a, b = _net().eval(), _net().eval()
    with torch.no_grad():
        oa, ob = a.forward_train(x, "bf16"), b.forward_train(x, "bf16", resident=False)
    assert all(torch.equal(p, q) for p, q in zip((oa[0], oa[2], oa[3]), (ob[0], ob[2], ob[3])))


# ---- graph ---------------------------------------------------------------------------------------------------------------------------
class Run(object):
    """one net from the fixed initial state, tdrn_amd.optim.SGD, static buffers and the step: forward_train resident,
    RefineMultiBoxLoss (ARM only_loc + ODM), backward, the optimizer (tests/test_gpu_sgd_graph.py's shape).  The net is
    refinedet_vgg (bn, use_refine): the same VGG-BN trunk, extras and TCB with DENSE heads.  dualrefinedet_vggbn's deformable heads
    accumulate their input gradient with float atomics (tdrn_hip.h section i-b says so), so no two steps of that net are bit-equal
    behind the heads, eager or replayed; every kernel of this net sums in a fixed order."""

    def __init__(self):
        import _loss_ref as R
        self.net = H.net(H.refinedet(True, False), STATE_SEED)
        self.start = {k: v.clone() for k, v in self.net.state_dict().items()}
        self.params = list(self.net.parameters())
        self.opt = SGD(self.params, lr=1e-3, momentum=0.9, weight_decay=5e-4)
        for p in self.params:
            p.grad = torch.zeros_like(p)
            self.opt.state[p]["momentum_buffer"] = torch.zeros_like(p)
        self.x = torch.from_numpy(_frames()).to(DEV)
        self.priors = H.priors(SIZE, MAPS)
        rows = [torch.from_numpy(np.ascontiguousarray(t)).float() for t in R.synth_targets(synth._rng("train_resident", 0), 1, 3, 20, 21)]
        # already on the device in tdrn_match's layout: nothing goes up from the host inside the captured step
        self.targets = PackedTargets(torch.cat(rows).to(DEV), torch.tensor([0, rows[0].size(0)], dtype=torch.int32, device=DEV),
                                     rows[0].size(0), rows[0].size(0))
        self.arm_criterion = RefineMultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, device=DEV, only_loc=True)
        self.criterion = RefineMultiBoxLoss(21, 0.5, True, 0, True, 3, 0.5, False, device=DEV)
        self.loss = torch.zeros(3, device=DEV)

    def restart(self):
        with torch.no_grad():
            for k, v in self.net.state_dict().items():
                v.copy_(self.start[k])
            for p in self.params:
                self.opt.state[p]["momentum_buffer"].zero_()
                p.grad.zero_()
            self.loss.zero_()

    def step(self):
        def closure():
            out = self.net.forward_train(self.x, "bf16", resident=True)
            loss_arm = self.arm_criterion(out[0], self.priors, self.targets)
            loss_l, loss_c = self.criterion(out[2:], self.priors, self.targets, arm_data=out[:2])
            loss = loss_arm + loss_l + loss_c
            grads = torch.autograd.grad(loss, self.params, allow_unused=True)
            with torch.no_grad():
                for p, g in zip(self.params, grads):
                    if g is not None:
                        p.grad.copy_(g)
                self.loss.copy_(torch.stack([loss_arm, loss_l, loss_c]))
            return loss
        self.opt.step(closure)

    def snapshot(self):
        torch.cuda.synchronize()
        s = {"loss": self.loss.clone()}
        s.update({"state." + k: v.clone() for k, v in self.net.state_dict().items()})
        s.update({"momentum.%d" % i: self.opt.state[p]["momentum_buffer"].clone() for i, p in enumerate(self.params)})
        return s


def test_captured_resident_step_replayed_twice_equals_two_eager_steps():
    eager = Run()
    want = []
    for _ in range(2):
        eager.step()
        want.append(eager.snapshot())
    assert bool(torch.isfinite(want[1]["loss"]).all()) and not torch.equal(want[0]["loss"], want[1]["loss"])
    r = Run()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        r.step()                                   # warm-up: every lazy initialisation happens outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    r.restart()
    r.opt.sync_hyper()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r.step()
    r.restart()
    for k in range(2):
        graph.replay()
        got = r.snapshot()
        assert sorted(got) == sorted(want[k])
        for key, ref in want[k].items():
            assert torch.equal(got[key].reshape(-1).view(torch.uint8), ref.reshape(-1).view(torch.uint8)), \
                "graph replay: %s differs from the eager run after step %d" % (key, k)
    del graph
