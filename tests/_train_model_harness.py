"""What the forward_train tests of the five trainable models share (test helper; product code never imports it): the fixtures (a
model's synthetic state, a loaded net, frames, smooth-loss targets, priors, the oracle-made ref_loc), the cached CPU references
(tests/_train_model_ref.py), and the checks.

The checks are functions of tensors and dicts, so tests/test_train_model_harness.py runs each of them on the CPU against a correct and
a doctored input.  They carry no cap, seed or bias rule of their own: a test file passes its own and keeps the docstring that
justifies them.  Two constants are the same wherever they are used and live here: a gradient's bound is FACTOR x the float32
yardstick's worst tensor, and a running statistic may differ from float64 by STAT_TOL max(1, max|ref|).
"""
import collections
import functools

import numpy as np
import torch

import _train_model_ref as M
from oracle import net_ref
from tdrn_amd.data import mb_cfg
from tdrn_amd.layers import PriorBox
from tdrn_amd.model import dualrefinedet_mobilenet, dualrefinedet_vggbn, refinedet_vgg, ssd4scale_mobile, ssd4scale_vgg
from tdrn_amd.optim import SGD
from tdrn_amd.utils import synth

DEV = "cuda:0"
FACTOR, STAT_TOL = 10, 1e-4
ORACLE = {"vgg": functools.partial(net_ref.ssd4scale_vgg_forward, bn=True), "mobile": net_ref.ssd4scale_mobile_forward}


# ---- the models ------------------------------------------------------------------------------------------------------------------------
class Model(collections.namedtuple("Model", "build args forward kwargs widths")):
    """build(*args): the module; forward(o, x, taps, ..., **dict(kwargs)): its restatement; widths: the last dimension of each output.
    Hashable, so that it keys the caches below: two test files that name the same model share its state and its references"""

    def restatement(self):
        return functools.partial(self.forward, **dict(self.kwargs))


def drn_vgg(bn, multihead):
    return Model(dualrefinedet_vggbn.build_net, ("train", 320, 21, 1024, 1, bn, multihead), M.drn_forward,
                 (("arch", "vgg"), ("multihead", multihead)), (4, 4, 21))


def drn_mobilenet(multihead):
    return Model(dualrefinedet_mobilenet.build_net, ("train", 320, 21, 1, multihead), M.drn_forward,
                 (("arch", "mobile"), ("multihead", multihead)), (4, 4, 21))


def refinedet(use_refine, multihead):
    return Model(refinedet_vgg.build_net, ("train", 320, 21, use_refine, 1024, True, multihead), M.refinedet_forward,
                 (("use_refine", use_refine), ("multihead", multihead)), (4, 4, 21) if use_refine else (4, 21))


def ssd4scale(arch, deform):
    build, args = ((ssd4scale_vgg.build_net, ("train", 320, 21, 1024, True, deform)) if arch == "vgg" else
                   (ssd4scale_mobile.build_net, ("train", 320, 21, 1024, deform)))
    return Model(build, args, M.ssd4scale_forward, (("arch", arch), ("deform", deform)), (4, 21))


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------
def build(model):
    return model.build(*model.args)


@functools.lru_cache(maxsize=None)
def state(model, seed):
    return synth.synth_state_dict({k: tuple(v.shape) for k, v in build(model).state_dict().items()}, seed)


def net(model, seed):
    """a fresh module with the synthetic weights on the device, in training mode as build_net leaves it"""
    n = build(model)
    n.load_state_dict({k: torch.from_numpy(v) for k, v in state(model, seed).items()})
    return n.to(DEV)


@functools.lru_cache(maxsize=None)
def frames(B, size, seed):
    return synth.synth_frames(B, size, seed=seed)


def priors_count(maps):
    return 3 * sum(f * f for f in maps)


@functools.lru_cache(maxsize=None)
def targets(count, widths, seed):
    """the smooth loss's fixed targets, one per output"""
    gen = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(1, count, w, generator=gen) for w in widths)


def priors(size, maps):
    cfg = dict(mb_cfg["VOC_320"], min_dim=size, feature_maps=list(maps), name="VOC_%d" % size)
    boxes = PriorBox(cfg).forward().to(DEV)
    assert boxes.shape[0] == priors_count(maps)
    return boxes


@functools.lru_cache(maxsize=None)
def ref_loc(arch, B, frame_seed, size, maps, state_seed):
    """ref_loc of a temporal SSD4Scale net, a constant of the tests: the loc maps of the static net of the same architecture (synthetic
    weights of `state_seed`) on the same frames, from the oracle"""
    got = ORACLE[arch](state(ssd4scale(arch, False), state_seed), frames(B, size, frame_seed), 21, "train", ret_loc=True)[2]
    assert [tuple(m.shape) for m in got] == [(B, 12, f, f) for f in maps]
    return tuple(np.ascontiguousarray(np.asarray(m, dtype=np.float32)) for m in got)


# ---- the CPU references, each computed once per process and never changed ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(model, state_seed, frame_seed, size, maps, target_seed, dtype, steps, lr, onednn, ref_loc_args=None, ref_loc_grad=False):
    """M.sgd_run of the model's restatement on one frame -> (the log, the final parameters).  onednn=False: torch's other float32
    evaluation of the same ops.  ref_loc_args: the arguments of ref_loc() for a temporal net"""
    extra = ref_loc(*ref_loc_args) if ref_loc_args is not None else None
    with torch.backends.mkldnn.flags(enabled=onednn):
        return M.sgd_run(model.restatement(), state(model, state_seed), frames(1, size, frame_seed),
                         targets(priors_count(maps), model.widths, target_seed), dtype, steps, lr, extra, ref_loc_grad)


@functools.lru_cache(maxsize=None)
def forward_outputs(model, state_seed, frame_seed, size, dtype):
    """the restatement's training-mode outputs on one frame, no gradients"""
    return M.run(model.restatement(), state(model, state_seed), frames(1, size, frame_seed), dtype, True)


# ---- checks ----------------------------------------------------------------------------------------------------------------------------
def tensors(out):
    return tuple(t for t in out if t is not None)


def buffers(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")}


def rows_off(got, ref, allowed, atol):
    """test_gpu_net.py's rule for outputs behind the deformable heads: (rows over atol that are on no discontinuity, max |d| over the
    rows inside atol); at most 30 rows may be on a discontinuity"""
    d = (got.detach().cpu().double() - torch.as_tensor(ref).double()).abs().reshape(-1, got.shape[-1]).numpy()
    bad = (d > atol).any(1)
    assert int(allowed.sum()) <= 30, "suspiciously many pixels on a discontinuity: %d rows" % int(allowed.sum())
    return int((bad & ~allowed).sum()), float(d[~bad].max())


def train_atol(ref):
    """train mode against float64: 1e-4 max(1, max|ref|)"""
    return 1e-4 * max(1.0, float(torch.as_tensor(ref).abs().max()))


def running_statistics_check(label, got, ref):
    """after one training-mode forward: every counter is 1, in ours and in the reference, and every running statistic is within
    STAT_TOL max(1, max|ref|) of float64"""
    worst = 0.0
    for k, v in got.items():
        r = ref[k]
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1 and int(r) == 1, k
            continue
        d, bound = float((v.cpu().double() - r).abs().max()), STAT_TOL * max(1.0, float(r.abs().max()))
        worst = max(worst, d / bound)
        assert d <= bound, (k, d, bound)
    print("train %s: running statistics, worst |d| / bound %.3e" % (label, worst))


class BnBiasRule(object):
    """a conv that feeds a training-mode BatchNorm has an exactly zero bias gradient (the batch mean removes the bias): ours is judged
    by |g| <= 1e-4 max(1, max|g64(the BatchNorm's bias)|).  zero_bias: M.bn_after_conv's {conv bias: BatchNorm prefix}"""

    def __init__(self, zero_bias):
        self.names = self.zero_bias = zero_bias

    def check(self, head, grads, ref):
        worst = 0.0
        for n, bn in self.zero_bias.items():
            g, scale = float(grads[n].abs().max()), max(1.0, float(ref["grads"][bn + ".bias"].abs().max()))
            worst = max(worst, g / scale)
            assert g <= 1e-4 * scale, (n, g, scale)
        print("%s: zero-gradient biases, worst |g| / max(1, |g(bn.bias)|) %.3e (bound 1e-4)" % (head, worst))


class AbsGoRule(object):
    """the cancelling biases: the batch mean removes the bias, what is left is the fp32 noise of a sum of grad_output.  Their float64
    gradient is at most 1e-12; ours is judged by |g| <= 2e-6 sum|grad_output| of the conv, per channel (ref["abs_go"]).  each: one
    line per bias, else one for the worst"""

    def __init__(self, names, each):
        self.names, self.each = names, each

    def check(self, head, grads, ref):
        worst = 0.0
        for n in self.names:
            g, s = grads[n].cpu().double().abs(), ref["abs_go"][n]
            assert float(ref["grads"][n].abs().max()) <= 1e-12, n
            ratio = float((g / (2e-6 * s)).max())
            worst = max(worst, ratio)
            if self.each:
                print("%s: %s worst |g| / (2e-6 sum|grad_output|) %.3e" % (head, n, ratio))
            assert bool((g <= 2e-6 * s).all()), (n, ratio)
        if not self.each:
            print("%s: %d cancelling biases, worst |g| / (2e-6 sum|grad_output|) %.3e" % (head, len(self.names), worst))


def gradient_check(label, grads, ref, yards, extra, cap, cap_inclusive, bias_rule):
    """Per tensor, the relative L2 distance to float64 is at most FACTOR x the worst tensor's float32 yardstick, and that bound is
    informative: at most `cap` (below it unless cap_inclusive).  grads {name: ours}; ref: one log entry of the float64 run; yards: the
    log entries of torch's float32 evaluations (a tensor's yardstick is the larger of them); extra: [(name, ours, float64, [float32,
    ...])], further tensors under the same rule; bias_rule: how the biases in bias_rule.names, left out above, are judged"""
    rel = lambda g, r: float((g.double() - r).norm() / r.norm())
    head = "gradients %s" % label if label else "gradients"
    names = [n for n in ref["grads"] if n not in bias_rule.names]
    yardstick = {n: max(rel(y["grads"][n], ref["grads"][n]) for y in yards) for n in names}
    ours = {}
    for n in names:
        assert grads.get(n) is not None and bool(torch.isfinite(grads[n]).all()), n
        ours[n] = rel(grads[n].cpu(), ref["grads"][n])
    for n, g, r, ys in extra:
        yardstick[n], ours[n] = max(rel(y, r) for y in ys), rel(g.cpu(), r)
    y_name, o_name = max(yardstick, key=yardstick.get), max(ours, key=ours.get)
    bound = FACTOR * yardstick[y_name]
    print("%s: ours worst %.3e (%s), float32 yardstick worst %.3e (%s), bound %.3e"
          % (head, ours[o_name], o_name, yardstick[y_name], y_name, bound))
    assert bound <= cap if cap_inclusive else bound < cap, \
        "uninformative: the float32 yardstick itself is at %.3e; change the input, not the factor" % yardstick[y_name]
    bad = {n: v for n, v in ours.items() if not v <= bound}
    assert not bad, bad
    bias_rule.check(head, grads, ref)


def short_run(net, loss_of, steps, lr):
    """`steps` plain-SGD steps of the module on loss_of(net) -> the losses"""
    losses = []
    for _ in range(steps):
        net.zero_grad()
        loss = loss_of(net)
        loss.backward()
        losses.append(float(loss.detach()))
        with torch.no_grad():
            for p in net.parameters():
                p -= lr * p.grad
    return losses


def short_run_check(losses, want, yard, steps):
    """the losses fall, in ours and in float64 (want), and ours stays within FACTOR x the float32 yardstick's own distance from float64
    at every step (floor: 1e-5 of the loss, the float32 evaluation of its means)"""
    print("short run: losses ours %r, float64 %r, float32 yardstick %r" % (losses, want, yard))
    assert len(losses) == len(want) == len(yard) == steps
    assert all(b < a for a, b in zip(want, want[1:])) and all(b < a for a, b in zip(losses, losses[1:]))
    for k, (a, b, y) in enumerate(zip(losses, want, yard)):
        bound = max(FACTOR * abs(y - b), 1e-5 * max(1.0, abs(b)))
        print("short run: step %d |ours - float64| %.3e, yardstick %.3e, bound %.3e" % (k, abs(a - b), abs(y - b), bound))
        assert abs(a - b) <= bound, (k, a, b, bound)


def finite_gradients(net, what=None):
    for n, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), what or n


def drop_in_fp32(net, evaluate, step, opt):
    """step(net, "fp32", opt) -> (outputs, losses): finite losses, a finite gradient on every parameter, and after opt.step() the
    engine re-packed by itself: evaluate(net) moved with no repack() call in between"""
    with torch.no_grad():
        before = [t.clone() for t in tensors(evaluate(net))]
    _, losses = step(net, "fp32", opt)
    assert all(np.isfinite(l) for l in losses), losses
    finite_gradients(net)
    opt.step()
    with torch.no_grad():
        after = [t.clone() for t in tensors(evaluate(net))]
    assert all(float((a - b).abs().max()) > 0 for a, b in zip(before, after))


def drop_in_16bit(make_net, step, ref, report):
    """the 16-bit compute types: the same pass is finite; report(compute, losses, the outputs' drift against the fp32 outputs `ref`):
    printed, not gated"""
    for compute in ("bf16", "fp16"):
        fresh = make_net()
        out, losses = step(fresh, compute, torch.optim.SGD(fresh.parameters(), lr=1e-3))
        assert all(np.isfinite(l) for l in losses), (compute, losses)
        finite_gradients(fresh, compute)
        report(compute, losses, [float((a.detach() - b.detach()).abs().max()) for a, b in zip(tensors(out), tensors(ref))])


def plumbing(net, out, reference_net, count, counters, exact):
    """a dual-refinement step's outputs and gradients: shapes and the None, finite fp32 outputs, a finite fp32 .grad on the parameters
    reference_net filled (with exact: on no other), and with counters every num_batches_tracked at 1"""
    assert len(out) == 4 and out[1] is None
    assert tuple(out[0].shape) == (1, count, 4) and tuple(out[2].shape) == (1, count, 4) and tuple(out[3].shape) == (1, count, 21)
    assert all(o.dtype == torch.float32 and bool(torch.isfinite(o).all()) for o in (out[0], out[2], out[3]))
    want = {n for n, p in reference_net.named_parameters() if p.grad is not None}
    assert want
    for n, p in net.named_parameters():
        if n in want:
            assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), n
        elif exact:
            assert p.grad is None, n
    if counters:
        for k, v in net.state_dict().items():
            if k.endswith("num_batches_tracked"):
                assert int(v) == 1, k


def moves_after_a_step(net, before, x):
    """the engine re-packs by itself: net(x) differs after a tdrn_amd.optim.SGD step on the gradients the net holds"""
    SGD(net.parameters(), lr=1e-3, momentum=0.9).step()
    with torch.no_grad():
        after = [t.clone() for t in net(x) if t is not None]
    assert all(float((a - b).abs().max()) > 0 for a, b in zip(before, after))
