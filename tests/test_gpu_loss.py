"""MultiBoxLoss / RefineMultiBoxLoss on the GPU (tdrn_hip.h section ii-b): against the reference's fixtures
(tests/golden/loss_*.npz), against the numpy restatement (tests/_loss_ref.py) at training sizes, the per-image wrappers,
the zero-truth rule, run-to-run determinism, autograd, the absence of host synchronisation, the drop-in protocol of
train.py on the engine's phase='train' outputs, and a short training run."""
import os

import numpy as np
import pytest
import torch

import _loss_ref as R
from tdrn_amd.layers import MultiBoxLoss, RefineMultiBoxLoss
from tdrn_amd.layers.box_utils import match, match_targets, refine_match
from tdrn_amd.layers.modules.multibox_loss import multibox_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VAR = (0.1, 0.2)


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(priors, loc, conf, arm, targets, C, g=(1.0, 1.0)):
    """(loc_t, conf_t, loss, sel, grad_loc, grad_conf) through the kernels, upstream gradients g."""
    pri = _cu(priors)
    tg = [_cu(t) for t in targets]
    loc_t, conf_t = match_targets(tg, pri, 0.5, VAR, _cu(arm))
    lg = _cu(loc).requires_grad_(True)
    cg = None if conf is None else _cu(conf).requires_grad_(True)
    loss, sel = multibox_loss(lg, cg, loc_t, conf_t, C, 3)
    (loss * torch.tensor(g, device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return (loc_t.cpu().numpy(), conf_t.cpu().numpy(), loss.detach().cpu().numpy(), sel.cpu().numpy(),
            lg.grad.cpu().numpy(), None if cg is None else cg.grad.cpu().numpy())


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_matches_reference_fixture(name):
    cfg, B, C, refine, only_loc, counts, seed = R.CASES[name]
    priors = R.priors_of(cfg, GOLDEN)
    P = priors.shape[0]
    loc, conf, arm, targets = R.case_inputs(name, P)
    g = np.load(os.path.join(GOLDEN, "loss_%s.npz" % name))
    loc_t, conf_t, loss, sel, gl, gc = _run(priors, loc, conf, arm, targets, C)
    np.testing.assert_array_equal(conf_t, g["conf_t"])
    np.testing.assert_array_equal(sel, g["sel"])
    rtol, atol = R.loc_t_tolerance(refine)
    np.testing.assert_allclose(loc_t, g["loc_t"], rtol=rtol, atol=atol)
    np.testing.assert_allclose(loss[0], g["loss_l"], rtol=1e-5)
    gl = gl.reshape(B * P, 4)
    np.testing.assert_allclose(gl[g["gloc_rows"]], g["gloc"], atol=1e-6)
    off = np.ones(B * P, bool)
    off[g["gloc_rows"]] = False
    assert (gl[off] == 0).all()
    if conf is not None:
        np.testing.assert_allclose(loss[1], g["loss_c"], rtol=1e-5)
        gc = gc.reshape(B * P, C)
        np.testing.assert_allclose(gc[g["gconf_rows"]], g["gconf"], atol=1e-6)
        off = (sel == 0).reshape(-1)
        assert (gc[off] == 0).all()


def _training_batch(B, seed, C=21, refine=True, cfg="VOC_320", lo=1, hi=40):
    from tdrn_amd.utils import synth
    priors = R.priors_of(cfg, GOLDEN)
    P = priors.shape[0]
    rng = synth._rng("loss_train", seed)
    targets = R.synth_targets(rng, B, lo, hi, C)
    loc = (0.5 * rng.standard_normal((B, P, 4))).astype(np.float32)
    conf = (1.5 * rng.standard_normal((B, P, C))).astype(np.float32)
    arm = (0.3 * rng.standard_normal((B, P, 4))).astype(np.float32) if refine else None
    return priors, loc, conf, arm, targets


@pytest.mark.parametrize("refine", [True, False])
def test_restatement_at_training_size(refine):
    B, C = 32, 21
    priors, loc, conf, arm, targets = _training_batch(B, 3 if refine else 4, C, refine)
    loc_t, conf_t, loss, sel, gl, gc = _run(priors, loc, conf, arm, targets, C, g=(0.7, 1.3))
    r_lt, r_ct = R.match_batch(0.5, targets, priors, VAR, arm)
    np.testing.assert_array_equal(conf_t, r_ct)
    rtol, atol = R.loc_t_tolerance(refine)
    np.testing.assert_allclose(loc_t, r_lt, rtol=rtol, atol=atol)
    r_sel, gaps = R.select(conf, r_ct)
    clear = gaps > 1e-5                          # images whose num_neg boundary is not a near-tie of the scores
    assert clear.sum() >= B - 4
    np.testing.assert_array_equal(sel[clear], r_sel[clear])
    ll, lc, N = R.losses(loc, conf, r_lt, r_ct, sel)      # the device's own selection: the sums alone are compared
    np.testing.assert_allclose(loss, [ll, lc], rtol=1e-5)
    rgl, rgc = R.grads(loc, conf, r_lt, r_ct, sel, 0.7, 1.3)
    np.testing.assert_allclose(gl, rgl, atol=1e-6)
    np.testing.assert_allclose(gc, rgc, atol=1e-6)


def test_per_image_wrappers_match_the_batched_path():
    B, C = 3, 21
    priors, loc, conf, arm, targets = _training_batch(B, 5, C)
    pri = _cu(priors)
    for use_arm in (False, True):
        lt, ct = match_targets([_cu(t) for t in targets], pri, 0.5, VAR, _cu(arm) if use_arm else None)
        loc_t = torch.empty(B, pri.size(0), 4)                  # the reference's CPU buffers
        conf_t = torch.empty(B, pri.size(0), dtype=torch.long)
        for b, t in enumerate(targets):
            tt = _cu(t)
            if use_arm:
                refine_match(0.5, tt[:, :4], pri, list(VAR), tt[:, 4], loc_t, conf_t, b, _cu(arm[b]))
            else:
                match(0.5, tt[:, :4], pri, list(VAR), tt[:, 4], loc_t, conf_t, b)
        assert torch.equal(loc_t, lt.cpu())
        assert torch.equal(conf_t, ct.cpu().long())


def test_zero_truth_image_is_background_and_adds_nothing():
    B, C = 3, 21
    priors, loc, conf, arm, targets = _training_batch(B, 6, C)
    crit = RefineMultiBoxLoss(C, 0.5, True, 0, True, 3, 0.5, False, device=DEV)
    pri = _cu(priors)
    full = crit((_cu(loc[:2]), _cu(conf[:2])), pri, [_cu(t) for t in targets[:2]], arm_data=(_cu(arm[:2]), None))
    tg = [_cu(t) for t in targets[:2]] + [torch.zeros(0, 5, device=DEV)]
    loc3, conf3, arm3 = (np.concatenate([a[:2], a[2:3]]) for a in (loc, conf, arm))
    lt, ct = match_targets(tg, pri, 0.5, VAR, _cu(arm3))
    assert (ct[2] == 0).all() and (lt[2] == 0).all()
    with_empty = crit((_cu(loc3), _cu(conf3)), pri, tg, arm_data=(_cu(arm3), None))
    for a, b in zip(full, with_empty):
        assert float(a) == float(b)
    _, sel = multibox_loss(_cu(loc3), _cu(conf3), lt, ct, C)
    assert (sel[2] == 0).all()
    # N = 0: the reference's arithmetic, 0/0
    l0 = crit((_cu(loc3[:1]), _cu(conf3[:1])), pri, [torch.zeros(0, 5, device=DEV)], arm_data=(_cu(arm3[:1]), None))
    assert all(bool(torch.isnan(v)) for v in l0)


def test_bitwise_deterministic():
    priors, loc, conf, arm, targets = _training_batch(8, 7)
    a = _run(priors, loc, conf, arm, targets, 21)
    b = _run(priors, loc, conf, arm, targets, 21)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_autograd_matches_torch_on_the_restatement_and_arm_loc_gets_none():
    B, C = 4, 21
    priors, loc, conf, arm, targets = _training_batch(B, 8, C)
    pri = _cu(priors)
    lg, cg, ag = _cu(loc).requires_grad_(True), _cu(conf).requires_grad_(True), _cu(arm).requires_grad_(True)
    crit = RefineMultiBoxLoss(C, 0.5, True, 0, True, 3, 0.5, False, device=DEV)
    arm_crit = RefineMultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, device=DEV, only_loc=True)
    tg = [_cu(t) for t in targets]
    l_arm = arm_crit(ag, pri, tg)
    l_l, l_c = crit((lg, cg), pri, tg, arm_data=(ag, None))
    (0.5 * l_arm + l_l + 2.0 * l_c).backward()
    # torch autograd of the restatement's losses on the same targets and selection
    lt, ct = match_targets(tg, pri, 0.5, VAR, ag)
    _, sel = multibox_loss(lg.detach(), cg.detach(), lt, ct, C)
    l2, c2 = lg.detach().clone().requires_grad_(True), cg.detach().clone().requires_grad_(True)
    pos, used = sel == 1, sel > 0
    N = (ct > 0).sum().float()
    ref = torch.nn.functional.smooth_l1_loss(l2[pos], lt[pos], reduction="sum") / N
    ref = ref + 2.0 * torch.nn.functional.cross_entropy(c2[used], ct[used].long(), reduction="sum") / N
    ref.backward()
    assert torch.allclose(lg.grad, l2.grad, atol=1e-6, rtol=0)
    assert torch.allclose(cg.grad, c2.grad, atol=1e-6, rtol=0)
    assert ag.grad is not None                                   # the ARM criterion's own loc gradient ...
    lt0, ct0 = match_targets(tg, pri, 0.5, VAR)
    a2 = ag.detach().clone().requires_grad_(True)
    (0.5 * torch.nn.functional.smooth_l1_loss(a2[ct0 > 0], lt0[ct0 > 0], reduction="sum") / (ct0 > 0).sum().float()).backward()
    assert torch.allclose(ag.grad, a2.grad, atol=1e-6, rtol=0)   # ... and nothing through refine_match's targets
    a3 = _cu(arm).requires_grad_(True)
    l_l3, l_c3 = crit((lg.detach(), cg.detach().requires_grad_(True)), pri, tg, arm_data=(a3, None))
    (l_l3 + l_c3).backward()
    assert a3.grad is None


def test_no_host_synchronisation():
    B, C = 4, 21
    priors, loc, conf, arm, targets = _training_batch(B, 9, C)
    pri, tg = _cu(priors), [torch.from_numpy(t) for t in targets]          # targets on the host, as the collate gives them
    lg, cg, ag = _cu(loc).requires_grad_(True), _cu(conf).requires_grad_(True), _cu(arm)
    crit = RefineMultiBoxLoss(C, 0.5, True, 0, True, 3, 0.5, False, device=DEV)
    arm_crit = RefineMultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, device=DEV, only_loc=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        l_arm = arm_crit(ag, pri, tg)
        l_l, l_c = crit((lg, cg), pri, tg, arm_data=(ag, None))
        (l_arm + l_l + l_c).backward()
        honoured = True
        try:
            _ = torch.ones(2, device=DEV).nonzero()
            honoured = False
        except RuntimeError:
            pass
    finally:
        torch.cuda.set_sync_debug_mode(0)
    print("sync debug mode honoured by this build: %s" % honoured)
    assert torch.isfinite(l_l) and torch.isfinite(l_c) and torch.isfinite(lg.grad).all()


def test_drop_in_protocol_on_engine_train_outputs():
    """train.py:185-186, :261-262 on build_net('train', 320, 21) outputs: a validation-loss pass."""
    from tdrn_amd.data import mb_cfg
    from tdrn_amd.layers import PriorBox
    from tdrn_amd.model.dualrefinedet_vggbn import build_net
    from tdrn_amd.utils import synth
    net = build_net("train", 320, 21, 1024, 1, True, False)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(DEV)
    x = torch.from_numpy(synth.synth_frames(2, 320, seed=4)).to(DEV)
    with torch.no_grad():
        out = net(x)
        priors = PriorBox(mb_cfg["VOC_320"]).forward().to(DEV)
    assert out[1] is None
    rng = synth._rng("loss_dropin", 0)
    targets_np = R.synth_targets(rng, 2, 3, 20, 21)
    targets = [_cu(t) for t in targets_np]
    arm_criterion = RefineMultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, device=DEV, only_loc=True)
    criterion = RefineMultiBoxLoss(21, 0.5, True, 0, True, 3, 0.5, False, device=DEV)
    loss_arm_l = arm_criterion(out[0], priors, targets)
    loss_l, loss_c = criterion(out[2:], priors, targets, arm_data=out[:2])
    assert loss_arm_l.dim() == 0 and loss_l.dim() == 0 and loss_c.dim() == 0 and loss_l.device.type == "cuda"
    pr = priors.cpu().numpy()
    arm, odm, conf = (t.cpu().numpy() for t in (out[0], out[2], out[3]))
    lt0, ct0 = R.match_batch(0.5, targets_np, pr, VAR)
    s0, _ = R.select(None, ct0)
    np.testing.assert_allclose(float(loss_arm_l), R.losses(arm, None, lt0, ct0, s0)[0], rtol=1e-5)
    lt, ct = R.match_batch(0.5, targets_np, pr, VAR, arm)
    s, gaps = R.select(conf, ct)
    d_lt, d_ct = match_targets(targets, priors, 0.5, VAR, out[0])
    _, d_sel = multibox_loss(out[2], out[3], d_lt, d_ct, 21)
    d_sel = d_sel.cpu().numpy()
    np.testing.assert_array_equal(d_sel[gaps > 1e-5], s[gaps > 1e-5])
    ll, lc, _ = R.losses(odm, conf, lt, ct, d_sel)
    np.testing.assert_allclose([float(loss_l), float(loss_c)], [ll, lc], rtol=1e-5)


def test_short_training_loss_falls():
    """Torch conv heads + ConvOffset2d + RefineMultiBoxLoss on one fixed batch: 20 SGD steps."""
    from tdrn_amd.model.networks import ConvOffset2d
    torch.manual_seed(0)
    B, C, Cf, S = 2, 21, 16, 10
    P = S * S * 3
    feat = torch.randn(B, Cf, S, S, device=DEV)
    arm_head = torch.nn.Conv2d(Cf, 3 * 4, 3, padding=1).to(DEV)
    off_head = torch.nn.Conv2d(Cf, 18, 3, padding=1).to(DEV)
    torch.nn.init.normal_(off_head.weight, std=0.01)
    dcn = ConvOffset2d(Cf, 3 * (4 + C), 3, padding=1).to(DEV)
    params = list(arm_head.parameters()) + list(off_head.parameters()) + list(dcn.parameters())
    opt = torch.optim.SGD(params, lr=0.02, momentum=0.9)
    ys, xs = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    c = torch.stack([(xs + 0.5) / S, (ys + 0.5) / S], -1).reshape(-1, 1, 2).expand(-1, 3, 2).reshape(-1, 2)
    wh = torch.tensor([[0.2, 0.2], [0.28, 0.14], [0.14, 0.28]]).repeat(S * S, 1)
    priors = torch.cat([c, wh], 1).float().to(DEV)
    from tdrn_amd.utils import synth
    targets = [_cu(t) for t in R.synth_targets(synth._rng("loss_sgd", 1), B, 2, 6, C)]
    arm_crit = RefineMultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, device=DEV, only_loc=True)
    crit = RefineMultiBoxLoss(C, 0.5, True, 0, True, 3, 0.5, False, device=DEV)
    hist = []
    for _ in range(20):
        arm = arm_head(feat).permute(0, 2, 3, 1).reshape(B, P, 4)
        y = dcn(feat, off_head(feat)).permute(0, 2, 3, 1).reshape(B, S * S, 3, 4 + C)
        odm_loc, odm_conf = y[..., :4].reshape(B, P, 4), y[..., 4:].reshape(B, P, C)
        loss = arm_crit(arm, priors, targets)
        ll, lc = crit((odm_loc, odm_conf), priors, targets, arm_data=(arm, None))
        loss = loss + ll + lc
        opt.zero_grad()
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in params if p.grad is not None)
        assert dcn.weight.grad is not None and off_head.weight.grad is not None
        opt.step()
        hist.append(float(loss))
    assert hist[-1] < 0.8 * hist[0], hist


def test_multibox_loss_module_on_the_plain_fixture():
    name = "voc320_plain"
    cfg, B, C, refine, only_loc, counts, seed = R.CASES[name]
    priors = R.priors_of(cfg, GOLDEN)
    loc, conf, arm, targets = R.case_inputs(name, priors.shape[0])
    g = np.load(os.path.join(GOLDEN, "loss_%s.npz" % name))
    crit = MultiBoxLoss(C, 0.5, True, 0, True, 3, 0.5, False, device=DEV)
    loss_l, loss_c = crit((_cu(loc), _cu(conf)), _cu(priors), [torch.from_numpy(t) for t in targets])
    np.testing.assert_allclose([float(loss_l), float(loss_c)], [g["loss_l"], g["loss_c"]], rtol=1e-5)
