"""forward_train of the two SSD4Scale models (ssd4scale_vgg with bn=True, ssd4scale_mobile), static (deform=False) and temporal
(deform=True, 8 deformable groups): the phase-'train' outputs computed from the module's own fp32 parameters through the library's
differentiable ops, so that loss.backward() fills their .grad: train_trn.py's loop.

References.  Eval mode: oracle.net_ref.ssd4scale_*_forward(phase='train') under test_gpu_net.py's rule for these models (atol 1e-3;
behind the deformable heads every prior row but those net_ref.border_rows finds on a sampling discontinuity).  Training mode:
ssd4scale_forward of tests/_train_model_ref.py, the same walks on torch's functional ops with F.batch_norm(training=True), on the CPU in
float64.  ref_loc of the temporal nets is a constant of the test: the loc maps of the static net of the same architecture (synthetic
weights of seed 1) on the same frames, from oracle.net_ref.ssd4scale_*_forward(ret_loc=True).  Fixtures and checks:
tests/_train_model_harness.py.

Inputs: 192 px, the smallest frame the 3x3 deformable heads accept (pyramid 24 / 12 / 6 / 3, P = 2295).  The float64 tests run ONE
image, eval mode and the drop-in steps two.

Gradients are compared per tensor by relative L2 against float64 (test_gpu_train_net.py says why never elementwise).  Yardstick:
torch's own float32 run of the restatement, evaluated both ways torch offers on the CPU (with oneDNN and with it switched off:
two correct float32 implementations of the same ops); a tensor's yardstick is the larger of its two distances from float64.  The two
differ by up to five times on these nets (temporal MobileNet, seed 1: 8.1e-4 and 3.9e-3), which is why one evaluation alone is no
measure of what correct fp32 implementations differ by.  Bound: 10 x the worst tensor's yardstick, under the condition that it stays
below 0.1 (else the input must change, not the factor).  Frame seeds, decided on the CPU by that condition alone: seed 5, the
project's, where it holds (VGG: worst yardstick 5.6e-3 static, 1.2e-3 temporal); otherwise the smallest seed from 1 up at which it
holds: the temporal MobileNet net 1 (3.9e-3), the static one 15 (7.5e-3; seeds 1 to 14 give 1.0e-2 to 4.3e-2).  A conv bias in front
of a training-mode BatchNorm has a float64 gradient of 1e-17: it is judged by |g| <= 2e-6 sum|grad_output| of its conv, per channel,
as test_gpu_train_mobilenet.py does.

Train-mode outputs against float64: |d| <= 1e-4 max(1, max|ref|) per output, on every prior row but those on a sampling
discontinuity behind the deformable heads; eval mode against the oracle keeps test_gpu_net.py's atol 1e-3.
"""
import numpy as np
import pytest
import torch

import _augment_ref as A
import _train_model_harness as H
import _train_model_ref as T
from oracle import net_ref
from tdrn_amd.layers import RefineMultiBoxLoss
from tdrn_amd.utils import synth
from tdrn_amd.utils.augmentations import PairSSDAugmentation

pytestmark = pytest.mark.gpu
DEV = H.DEV
torch.set_num_threads(min(16, torch.get_num_threads()))

SIZE, MAPS = 192, (24, 12, 6, 3)
P = 3 * sum(f * f for f in MAPS)
LR, STEPS = 0.01, 3
SEED64 = {("vgg", False): 5, ("vgg", True): 5, ("mobile", False): 15, ("mobile", True): 1}   # the float64 tests' one image (header)
SEED = 5                               # eval mode's and the drop-in steps' two images
STATE_SEED, STATIC_SEED, TARGET_SEED = 0, 1, 77      # the nets' synthetic weights; those of the static net behind ref_loc; the targets
CAP = 0.1                              # on 10 x yardstick, inclusive (header)
CASES = [("vgg", False), ("vgg", True), ("mobile", False), ("mobile", True)]
CASE = pytest.mark.parametrize("arch,deform", CASES, ids=["%s-%s" % (a, "temporal" if d else "static") for a, d in CASES])


def _build(arch, deform):
    return H.build(H.ssd4scale(arch, deform))


def _state(arch, deform, seed=STATE_SEED):
    return H.state(H.ssd4scale(arch, deform), seed)


def _net(arch, deform, seed=STATE_SEED):
    return H.net(H.ssd4scale(arch, deform), seed)


def _frames(B, seed):
    return H.frames(B, SIZE, seed)


def _ref_loc(arch, B, seed):
    return H.ref_loc(arch, B, seed, SIZE, MAPS, STATIC_SEED)


def _ref_loc_dev(arch, deform, B, seed):
    return [torch.from_numpy(m).to(DEV) for m in _ref_loc(arch, B, seed)] if deform else ()


def _targets():
    return H.targets(P, (4, 21), TARGET_SEED)


def _reference(arch, deform, dtype, ref_loc_grad=False, onednn=True):
    """the restatement's SGD run on the CPU, computed once and never changed: STEPS steps for the temporal VGG net (the short run;
    its first step serves the forward and gradient tests), one step for the others.  onednn=False: torch's other float32
    evaluation of the same ops, one step"""
    steps = STEPS if (arch, deform, ref_loc_grad, onednn) == ("vgg", True, False, True) else 1
    seed = SEED64[arch, deform]
    return H.reference(H.ssd4scale(arch, deform), STATE_SEED, seed, SIZE, MAPS, TARGET_SEED, dtype, steps, LR, onednn,
                       (arch, 1, seed, SIZE, MAPS, STATIC_SEED) if deform else None, ref_loc_grad)


def _yardsticks(arch, deform, ref_loc_grad=False):
    """step 0 of torch's two float32 evaluations of the restatement: with oneDNN and without"""
    return [_reference(arch, deform, torch.float32, ref_loc_grad, onednn)[0][0] for onednn in (True, False)]


def _ours(net, arch, deform, compute="fp32", ref_loc=None):
    seed = SEED64[arch, deform]
    x = torch.from_numpy(_frames(1, seed)).to(DEV)
    out = net.forward_train(x, _ref_loc_dev(arch, deform, 1, seed) if ref_loc is None else ref_loc, compute)
    return out, T.smooth_loss(out, _targets())


def _gradient_check(label, grads, ref, yards, extra=()):
    """the cancelling biases are those whose conv's grad_output the float64 run recorded: every conv bias in front of a BatchNorm"""
    H.gradient_check(label, grads, ref, yards, extra, CAP, True, H.AbsGoRule(sorted(ref["abs_go"]), each=False))


def _allowed(deform, offsets, B):
    """no exception without a deformable head"""
    if not deform:
        return np.zeros(B * P, bool)
    return net_ref.border_rows({"offset.%d" % s: torch.as_tensor(np.asarray(o)) for s, o in enumerate(offsets)}, False, def_groups=T.G)


@CASE
def test_eval_mode_matches_the_oracle(arch, deform):
    B = 2
    net = _net(arch, deform).eval()
    before = H.buffers(net)
    x = _frames(B, SEED)
    ref_loc = _ref_loc(arch, B, SEED) if deform else None
    with torch.no_grad():
        out = net.forward_train(torch.from_numpy(x).to(DEV), _ref_loc_dev(arch, deform, B, SEED), ret_loc=True)
    assert len(out) == 3 and tuple(out[0].shape) == (B, P, 4) and tuple(out[1].shape) == (B, P, 21)
    want = H.ORACLE[arch](_state(arch, deform), x, 21, "train", deform_on=deform, ref_loc=ref_loc, ret_loc=True, ret_off=True)
    allowed = _allowed(deform, want[3], B)
    bad_loc, d_loc = H.rows_off(out[0], want[0], allowed, 1e-3)
    bad_conf, d_conf = H.rows_off(out[1], want[1], allowed, 1e-3)
    print("eval %s deform=%s: max|d| loc %.3e conf %.3e (atol 1e-3), rows on a discontinuity %d" % (arch, deform, d_loc, d_conf, int(allowed.sum())))
    assert bad_loc == 0 and bad_conf == 0
    if deform:
        assert out[2] == []                          # as the reference: the temporal net hands back no loc maps
    else:
        assert [tuple(m.shape) for m in out[2]] == [(B, 12, f, f) for f in MAPS]
        for m, r in zip(out[2], want[2]):
            assert float((m.cpu() - torch.as_tensor(r)).abs().max()) <= 1e-3
    after = H.buffers(net)
    assert all(torch.equal(before[k], after[k]) for k in before), "eval mode changed a running buffer"
    # with an autograd graph when asked for one, in eval mode too; the loc maps carry it; self.phase does not matter
    net.phase = "test"
    out = net.forward_train(torch.from_numpy(x).to(DEV), _ref_loc_dev(arch, deform, B, SEED), ret_loc=True)
    assert out[0].requires_grad and out[1].requires_grad and all(m.requires_grad for m in out[2])
    assert tuple(out[1].shape) == (B, P, 21)
    assert len(net.forward_train(torch.from_numpy(x).to(DEV), _ref_loc_dev(arch, deform, B, SEED))) == 2


@CASE
def test_train_mode_forward_and_running_statistics(arch, deform):
    net = _net(arch, deform)
    assert net.training
    with torch.no_grad():
        out, _ = _ours(net, arch, deform)
    ref = _reference(arch, deform, torch.float64)[0][0]
    allowed = _allowed(deform, [ref["taps"]["offset.%d" % s] for s in range(4)] if deform else None, 1)
    a_loc, a_conf = H.train_atol(ref["outs"][0]), H.train_atol(ref["outs"][1])
    bad_loc, d_loc = H.rows_off(out[0], ref["outs"][0], allowed, a_loc)
    bad_conf, d_conf = H.rows_off(out[1], ref["outs"][1], allowed, a_conf)
    print("train %s deform=%s: max|d| loc %.3e (bound %.3e) conf %.3e (bound %.3e), rows on a discontinuity %d, rows over the bound %d + %d"
          % (arch, deform, d_loc, a_loc, d_conf, a_conf, int(allowed.sum()), bad_loc, bad_conf))
    assert bad_loc == 0 and bad_conf == 0
    H.running_statistics_check("%s deform=%s" % (arch, deform), H.buffers(net), ref["buffers"])


@CASE
def test_train_mode_gradients(arch, deform):
    net = _net(arch, deform)
    _, loss = _ours(net, arch, deform)
    loss.backward()
    ref, yards = _reference(arch, deform, torch.float64)[0][0], _yardsticks(arch, deform)
    grads = {n: p.grad for n, p in net.named_parameters()}
    assert set(grads) == set(ref["grads"])
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"]))
    _gradient_check("%s deform=%s" % (arch, deform), grads, ref, yards)


def test_a_ref_loc_that_requires_grad_gets_its_gradient():
    arch, deform = "vgg", True
    net = _net(arch, deform)
    ref_loc = [t.requires_grad_(True) for t in _ref_loc_dev(arch, deform, 1, SEED64[arch, deform])]
    _, loss = _ours(net, arch, deform, ref_loc=ref_loc)
    loss.backward()
    ref, yards = _reference(arch, deform, torch.float64, True)[0][0], _yardsticks(arch, deform, True)
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0 for t in ref_loc)
    extra = [("ref_loc[%d]" % s, ref_loc[s].grad, ref["extra_grads"][s], [y["extra_grads"][s] for y in yards]) for s in range(4)]
    _gradient_check("vgg temporal, ref_loc requires grad", {n: p.grad for n, p in net.named_parameters()}, ref, yards, extra)
    # a constant ref_loc gets none, and costs nothing: needs_input_grad gates the launch
    const = _ref_loc_dev(arch, deform, 1, SEED64[arch, deform])
    _ours(_net(arch, deform), arch, deform, ref_loc=const)[1].backward()
    assert all(t.grad is None for t in const)


def test_short_sgd_run_follows_float64():
    """Three plain-SGD steps of the temporal VGG net on the smooth loss.  Losses only (test_gpu_train_net.py says why no parameter
    comparison can hold): the losses fall, in ours and in float64, and ours stays within 10 x the float32 yardstick's own distance from
    float64 at every step (floor: 1e-5 of the loss, the float32 evaluation of its means)."""
    arch, deform = "vgg", True
    want = [l["loss"] for l in _reference(arch, deform, torch.float64)[0]]
    yard = [l["loss"] for l in _reference(arch, deform, torch.float32)[0]]
    losses = H.short_run(_net(arch, deform), lambda net: _ours(net, arch, deform)[1], STEPS, LR)
    H.short_run_check(losses, want, yard, STEPS)


def _priors():
    return H.priors(SIZE, MAPS)


def _criterion():
    return RefineMultiBoxLoss(21, 0.5, True, 0, True, 3, 0.5, False, device=DEV)


def _trn_step(static, net, x, targets, priors, compute, opt, loose=0.5):
    """train_trn.py:209-221: the static net on the engine, the temporal net through forward_train, the refine loss on the static
    net's ARM output, backward"""
    deform = net.deform
    with torch.no_grad():
        static_out = list(static(x, ret_loc=deform))
    static_out[0] *= loose
    opt.zero_grad()
    out = net.forward_train(x, static_out[2] if deform else (), compute)
    loss_l, loss_c = _criterion()(out, priors, targets, arm_data=static_out[:2])
    (loss_l + loss_c).backward()
    return out, (float(loss_l.detach()), float(loss_c.detach()))


@pytest.mark.parametrize("arch", ["vgg", "mobile"])
def test_drop_in_trn_step(arch):
    """train_trn.py's default path with --deform: two images, one SGD step with momentum and weight decay"""
    import _loss_ref as R
    B = 2
    static, net = _net(arch, False, 1).eval(), _net(arch, True)
    priors = _priors()
    targets = [torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in R.synth_targets(synth._rng("train_trn_dropin", 0), B, 3, 20, 21)]
    x = torch.from_numpy(_frames(B, SEED)).to(DEV)
    with torch.no_grad():
        ref_loc = static(x, ret_loc=True)[2]
    step = lambda n, compute, opt: _trn_step(static, n, x, targets, priors, compute, opt)
    H.drop_in_fp32(net, lambda n: n(x, ref_loc=ref_loc), step, torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4))
    assert all(p.grad is None for p in static.parameters())
    with torch.no_grad():
        ref = _net(arch, True).forward_train(x, ref_loc)
    H.drop_in_16bit(lambda: _net(arch, True), step, ref, lambda compute, losses, drift: print(
        "drop-in %s %s: losses %r, output drift against fp32: loc %.3e conf %.3e" % (arch, compute, losses, *drift)))


def test_pair_path_step():
    """train_trn.py:196-203 (--augm_type pairssd) with deform=False: PairSSDAugmentation.batch -> the static net on images_ori ->
    forward_train(images_trans) -> the refine loss with packed_trans"""
    B, arch = 2, "vgg"
    static, net = _net(arch, False, 1).eval(), _net(arch, False)
    rs = np.random.RandomState(11)
    frames, targets = [], []
    for b in range(B):
        H, W = int(rs.randint(300, 401)), int(rs.randint(300, 401))
        frames.append(torch.from_numpy(np.ascontiguousarray(A.case_image(H, W, 11000 + b))).to(DEV))
        targets.append(torch.from_numpy(A.case_boxes(H, W, 3, 11000 + b)))
    aug = PairSSDAugmentation(SIZE, (104, 117, 123), seed=3)
    images_ori, images_trans, packed_ori, packed_trans = aug.batch(frames, targets, list(range(B)), seed=0)
    assert tuple(images_trans.shape) == (B, 3, SIZE, SIZE)
    with torch.no_grad():
        static_out = static(images_ori)
    out = net.forward_train(images_trans)
    loss_l, loss_c = _criterion()(out, _priors(), packed_trans, arm_data=static_out[:2])
    (loss_l + loss_c).backward()
    assert np.isfinite(float(loss_l.detach())) and np.isfinite(float(loss_c.detach()))
    for n, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n


def test_paired_and_separate_heads_agree():
    """the loc and conf heads of a level as one conv_offset2d over the concatenated weights (the default), or as two calls: the same
    function.  Outputs and the heads' own gradients differ by fp32 summation order only (tile shapes and split counts follow Cout):
    |d| <= 1e-4 max(1, max|ref|), the fp32 bound of the conv tests.  The separate form also meets the float64 reference under the
    gradient test's rule."""
    arch = "vgg"
    runs = []
    for paired in (True, False):
        net = _net(arch, True)
        net._paired_heads = paired
        out, loss = _ours(net, arch, True)
        loss.backward()
        runs.append((out, {n: p.grad for n, p in net.named_parameters()}))
    (o1, g1), (o2, g2) = runs
    close = lambda a, b: float((a - b).detach().abs().max()) <= 1e-4 * max(1.0, float(b.detach().abs().max()))
    assert close(o1[0], o2[0]) and close(o1[1], o2[1])
    for n in g1:
        if n.startswith("arm_loc") or n.startswith("arm_conf") or n.startswith("offset"):
            assert close(g1[n], g2[n]), n
    _gradient_check("vgg temporal, separate heads", g2, _reference(arch, True, torch.float64)[0][0], _yardsticks(arch, True))


def test_bad_inputs_raise_and_the_engine_is_left_alone():
    for arch in ("vgg", "mobile"):
        net = _build(arch, True)
        with pytest.raises(NotImplementedError):
            net.forward_train(torch.zeros(1, 3, SIZE, SIZE), [torch.zeros(1, 12, f, f) for f in MAPS])
        assert net._engine is None                                  # forward_train builds no engine
        net = net.to(DEV)
        with pytest.raises(ValueError):
            net.forward_train(torch.zeros(3, SIZE, SIZE, device=DEV))
        x = torch.zeros(1, 3, SIZE, SIZE, device=DEV)
        with pytest.raises(ValueError, match="needs ref_loc"):
            net.forward_train(x)
        with pytest.raises(ValueError, match="ref_loc"):
            net.forward_train(x, [torch.zeros(1, 12, f, f, device=DEV) for f in MAPS[:3]])
        with pytest.raises(ValueError, match="ref_loc"):
            net.forward_train(x, [torch.zeros(1, 12, f + 1, f, device=DEV) for f in MAPS])
        with pytest.raises(NotImplementedError):
            net.forward_train(x, [torch.zeros(1, 12, f, f) for f in MAPS])
