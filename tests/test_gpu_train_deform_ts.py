"""forward_train(..., deform_algo="transform") of the two dual-refinement models: the deformable ODM heads through
networks.conv_offset2d_ts, the loc and conf heads of a level as one call.

dualrefinedet_vggbn at 192 px (320 px with multihead: CONFIG), one image, bf16, the synth state and frame seed 5 of
tests/test_gpu_train_resident.py.
  * plumbing with and without multihead, resident or not: shapes and the None, finite fp32 .grad on exactly the parameters the default
    path fills, net(x) moves after an SGD step;
  * arm_loc sits in front of the heads: it equals the default path's bit for bit;
  * the yardstick of odm_loc and conf is the existing path: their relative L2 distance to the float64 restatement
    (tests/_train_model_ref.py) under "transform" is at most 2 x that under "gather", both computed here (the 192 px layout).  The
    transform rounds X and Y where the gather path rounds the sampled columns: one more rounding, sqrt(2) expected, 2 leaves room
    (as in DESIGN.md section 22); measured: odm_loc 1.2797e-1 -> 1.2798e-1, conf 1.1879e-1 -> 1.1879e-1, ratio 1.000;
    both distances are dominated by the 16-bit trunk in front of the discontinuous sampling;
  * the relative L2 difference between the two paths of the head weights' gradients and of the gradient at the ODM sources is printed,
    not gated: the op-level test (tests/test_gpu_deform_ts.py) is the gate.
dualrefinedet_mobilenet: plumbing only.  In eval mode deform_algo="gather" and the omitted argument give equal bits."""
import pytest
import torch

import _train_model_harness as H
import _train_model_ref as T
from tdrn_amd.model.dualrefinedet_mobilenet import build_net as build_mobilenet
from tdrn_amd.utils import synth

from _conv_train_harness import DEV

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
# multihead: the 5 x 5 heads need maps of at least 5 x 5 on the gather path (its "input image is smaller than kernel" rule), so that
# layout runs at 320 px, as in tests/test_gpu_train_mobilenet.py; its float64 restatement would take several times as long and is left out
CONFIG = {False: (192, (24, 12, 6, 3)), True: (320, (40, 20, 10, 5))}
COMPUTE = "bf16"
SEED, STATE_SEED, TARGET_SEED = 5, 0, 77


def _priors(multihead):
    return H.priors_count(CONFIG[multihead][1])


def _net(multihead):
    return H.net(H.drn_vgg(True, multihead), STATE_SEED)


def _frames(multihead=False):
    return H.frames(1, CONFIG[multihead][0], SEED)


def _float64_outputs():
    """the float64 restatement's training-mode forward of the single-head net on the CPU, computed once (and shared with
    test_gpu_train_resident.py)"""
    return H.forward_outputs(H.drn_vgg(True, False), STATE_SEED, SEED, CONFIG[False][0], torch.float64)


def _targets(priors):
    return H.targets(priors, (4, 4, 21), TARGET_SEED)


def _keep_odm_sources(net):
    """the ODM sources of the next forward_train, with their gradients retained (the wrapper changes no arithmetic)"""
    kept, inner = [], net._tcb_train

    def tcb(arm_sources, x, compute):
        sources = inner(arm_sources, x, compute)
        for s in sources:
            s.retain_grad()
        kept.extend(sources)
        return sources

    net._tcb_train = tcb
    return kept


def _step(net, resident, **kw):
    """forward_train, the smooth loss, backward -> the outputs"""
    x = torch.from_numpy(_frames(net.multihead)).to(DEV)
    out = net.forward_train(x, COMPUTE, resident, **kw)
    T.smooth_loss((out[0], out[2], out[3]), _targets(out[0].size(1))).backward()
    return out


@pytest.mark.parametrize("resident", [False, True], ids=["nchw", "resident"])
@pytest.mark.parametrize("multihead", [False, True], ids=["one-head", "multihead"])
def test_transform_against_the_gather_path(multihead, resident):
    rel = lambda got, ref: float((got.detach().cpu().double() - ref.detach().cpu().double()).norm() / ref.detach().cpu().double().norm())
    gather, transform = _net(multihead), _net(multihead)
    assert transform.training
    x = torch.from_numpy(_frames(multihead)).to(DEV)
    with torch.no_grad():
        before = [t.clone() for t in transform(x) if t is not None]
    src_g, src_t = _keep_odm_sources(gather), _keep_odm_sources(transform)
    out_g = _step(gather, resident)
    out_t = _step(transform, resident, deform_algo="transform")
    H.plumbing(transform, out_t, gather, _priors(multihead), counters=False, exact=True)
    assert torch.equal(out_g[0], out_t[0]), "arm_loc sits in front of the heads"
    what = "multihead=%s resident=%s %s" % (multihead, resident, COMPUTE)
    if not resident and not multihead:
        ref = _float64_outputs()
        for name, i, j in (("odm_loc", 2, 1), ("conf", 3, 2)):
            d_g, d_t = rel(out_g[i], ref[j]), rel(out_t[i], ref[j])
            print("%s, %s relative L2 to float64: gather %.4e, transform %.4e (ratio %.3f)" % (what, name, d_g, d_t, d_t / d_g))
            assert d_t <= 2 * d_g, (name, d_t, d_g)
    # printed, not gated: the two paths' gradients
    pg, pt = dict(gather.named_parameters()), dict(transform.named_parameters())
    for prefix in ("odm_loc.", "odm_conf.", "odm_loc_2.", "odm_conf_2.", "offset.", "offset2."):
        names = [n for n in pg if n.startswith(prefix) and pg[n].grad is not None]
        if names:
            print("%s, gradients of %s* transform vs gather, relative L2: %s"
                  % (what, prefix, " ".join("%.3e" % rel(pt[n].grad, pg[n].grad) for n in names)))
    assert len(src_g) == len(src_t) == 4
    print("%s, gradient at the ODM sources transform vs gather, relative L2: %s"
          % (what, " ".join("%.3e" % rel(a.grad, b.grad) for a, b in zip(src_t, src_g))))
    H.moves_after_a_step(transform, before, x)


def test_mobilenet_plumbing():
    def net():
        m = build_mobilenet("train", 320, 21)
        sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 0)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return m.to(DEV)

    gather, transform = net(), net()
    x = torch.from_numpy(_frames()).to(DEV)
    with torch.no_grad():
        before = [t.clone() for t in transform(x) if t is not None]
    out_g = _step(gather, False)
    out_t = _step(transform, False, deform_algo="transform")
    H.plumbing(transform, out_t, gather, _priors(False), counters=False, exact=True)       # the same four maps at 192 px: 24, 12, 6, 3
    assert torch.equal(out_g[0], out_t[0])
    H.moves_after_a_step(transform, before, x)


def test_gather_is_the_default_bit_for_bit():
    x = torch.from_numpy(_frames(True)).to(DEV)
    a, b = _net(True).eval(), _net(True).eval()
    with torch.no_grad():
        oa, ob = a.forward_train(x, COMPUTE), b.forward_train(x, COMPUTE, deform_algo="gather")
    assert all(torch.equal(p, q) for p, q in zip((oa[0], oa[2], oa[3]), (ob[0], ob[2], ob[3])))
    # the switch is checked before the engine is marked stale
    with torch.no_grad():
        a(x)
    assert not a._dirty
    with pytest.raises(ValueError):
        a.forward_train(x, "fp32", deform_algo="transform")
    with pytest.raises(ValueError):
        a.forward_train(x, COMPUTE, deform_algo="nonsense")
    assert not a._dirty
