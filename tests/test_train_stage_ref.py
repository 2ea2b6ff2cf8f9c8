"""tests/_train_stage_ref.py proved on the CPU before it judges the kernels (no GPU): the six ops of tdrn_amd.model.networks are
replaced by float32 torch stand-ins of the same signatures, RefineSSD.forward_train + smooth_loss.backward() run on the CPU (single
head, 192 px, batch 1, synthetic weights seed 0, frames seed 5), and

  (a) the recorder is exact: for three stages of different kinds, two of them with an output that has two consumers (conv4_3 behind
      its BatchNorm: L2Norm and the next pool; an arm_loc conv: the output and the offset conv), the recorded grad_output and
      grad_input equal torch.autograd.grad taken directly on the same graph, bit for bit;
  (b) a correct fp32 implementation passes every stage (the worst share per kind is printed: the yardstick of DESIGN.md);
  (c) nine mutations, each in one op of ONE run (a stage is judged from its own inputs, so they do not disturb each other): every
      mutated stage fails, at the tensor the mutation breaks, and no other stage of the part of the net that is re-checked fails --
      none upstream of a mutation, none downstream;
  (d) a stand-in that writes into its input trips the recorder's immutability check.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import _deform_grad_ref as D
import _train_model_ref as T
import _train_stage_ref as R
from tdrn_amd import _lib
from tdrn_amd.model import networks
from tdrn_amd.model.dualrefinedet_vggbn import build_net
from tdrn_amd.utils import synth

torch.set_num_threads(min(16, torch.get_num_threads()))
SIZE, MAPS = 192, (24, 12, 6, 3)


# ---- float32 stand-ins with the signatures of the six ops ------------------------------------------------------------------------
def conv2d(input, weight, bias=None, padding=0, dilation=1, compute="fp32", stride=1):
    return F.conv2d(input, weight, bias, stride, padding, dilation)


def batch_norm(input, running_mean, running_var, weight, bias, training, momentum=0.1, eps=1e-5, relu=False):
    z = F.batch_norm(input, running_mean, running_var, weight, bias, training, momentum, eps)
    return F.relu(z) if relu else z


def max_pool2d(input, kernel_size, stride=None, padding=0, ceil_mode=False):
    return F.max_pool2d(input, kernel_size, stride, padding, ceil_mode=ceil_mode)


def l2norm(input, weight, eps=1e-10):
    return weight.view(1, -1, 1, 1) * (input / (input.pow(2).sum(dim=1, keepdim=True).sqrt() + eps))


def conv_transpose2d(input, weight, bias=None, stride=2, compute="fp32"):
    return F.conv_transpose2d(input, weight, bias, stride)


def conv_offset2d(input, offset, weight, stride=1, padding=0, dilation=1, deform_groups=1, compute="fp32"):
    return D.deform_conv(input.double(), offset.double(), weight.double(), stride, padding, dilation, deform_groups).float()


STAND_INS = dict(conv2d=conv2d, batch_norm=batch_norm, max_pool2d=max_pool2d, l2norm=l2norm, conv_transpose2d=conv_transpose2d,
                 conv_offset2d=conv_offset2d)


class _WrongGradient(torch.autograd.Function):
    """fn(*tensors) with autograd's own gradients passed through `spoil(gradients, tensors, grad_output) -> gradients`"""

    @staticmethod
    def forward(ctx, fn, spoil, *tensors):
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_(t.requires_grad) for t in tensors]
            out = fn(*leaves)
        ctx.leaves, ctx.out, ctx.spoil = leaves, out, spoil
        return out.detach()

    @staticmethod
    def backward(ctx, go):
        need = [i for i, t in enumerate(ctx.leaves) if t.requires_grad]
        grads = [None] * len(ctx.leaves)
        for i, g in zip(need, torch.autograd.grad(ctx.out, [ctx.leaves[i] for i in need], go, retain_graph=True)):
            grads[i] = g
        return (None, None) + tuple(ctx.spoil(grads, ctx.leaves, go))


def _only(name, weight):
    """the mutation of the stage whose weight is the parameter `name` of the net under test"""
    return MUTATED_NET[0] is not None and weight is dict(MUTATED_NET[0].named_parameters())[name]


MUTATED_NET = [None]
# stage -> (the tensor whose check must fail, what is wrong)
MUTATIONS = {
    "trans_layers.1.2": ("grad_weight", "one tap of the weight gradient dropped"),
    "latent_layers.0": ("grad_input", "grad_input shifted by one column"),
    "extras.1": ("ReLU decisions differ", "BatchNorm on the running statistics in training mode"),
    "extras.4": ("grad_input", "BatchNorm's gradient without the mean(go xhat) term"),
    "max_pool2d.4": ("grad_input", "pool gradient routed to the last maximum of a tie"),
    "up_layers.1": ("output", "two phases of the ConvTranspose swapped"),
    "L2Norm_5_3": ("grad_input", "L2Norm's gradient without the projection term"),
    "arm_loc.2": ("no gradient arrived", "missing bias gradient"),
    "odm_loc.1": ("grad_offset", "grad_offset with the h and w components swapped"),
}


def m_conv2d(input, weight, bias=None, padding=0, dilation=1, compute="fp32", stride=1):
    fn = lambda x, w, b: F.conv2d(x, w, b, stride, padding, dilation)
    if _only("trans_layers.1.2.weight", weight):
        def spoil(g, leaves, go):
            g[1] = g[1].clone()
            g[1][:, :, 0, 2] = 0
            return g
        return _WrongGradient.apply(fn, spoil, input, weight, bias)
    if _only("latent_layers.0.weight", weight):
        return _WrongGradient.apply(fn, lambda g, leaves, go: [torch.roll(g[0], 1, 3), g[1], g[2]], input, weight, bias)
    if _only("arm_loc.2.weight", weight):
        return fn(input, weight, bias.detach())
    return fn(input, weight, bias)


def m_batch_norm(input, running_mean, running_var, weight, bias, training, momentum=0.1, eps=1e-5, relu=False):
    if _only("extras.1.weight", weight):
        return F.relu(F.batch_norm(input, running_mean, running_var, weight, bias, False, momentum, eps))
    if _only("extras.4.weight", weight):
        def fn(x, w, b):
            mean, var = x.mean((0, 2, 3), keepdim=True), x.var((0, 2, 3), unbiased=False, keepdim=True)
            # xhat's statistics detached in the variance: autograd then drops the mean(go xhat) xhat term, and only that
            xhat = (x - mean) / torch.sqrt(var.detach() + eps)
            return F.relu(w.view(1, -1, 1, 1) * xhat + b.view(1, -1, 1, 1))
        return fn(input, weight, bias)
    return batch_norm(input, running_mean, running_var, weight, bias, training, momentum, eps, relu)


POOLS = [0]


def m_max_pool2d(input, kernel_size, stride=None, padding=0, ceil_mode=False):
    POOLS[0] += 1
    if MUTATED_NET[0] is not None and POOLS[0] == 5:          # pool5: 12 x 12 -> 6 x 6, 2 x 2 / 2, no padding
        def fn(x):
            N, C, H, W = x.shape
            win = x.view(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
            last = 3 - torch.flip(win == win.max(-1, keepdim=True)[0], (-1,)).float().argmax(-1, keepdim=True)
            return win.gather(-1, last)[..., 0]
        return fn(input)
    return max_pool2d(input, kernel_size, stride, padding, ceil_mode)


def m_l2norm(input, weight, eps=1e-10):
    if _only("L2Norm_5_3.weight", weight):
        return weight.view(1, -1, 1, 1) * (input / (input.pow(2).sum(dim=1, keepdim=True).sqrt().detach() + eps))
    return l2norm(input, weight, eps)


def m_conv_transpose2d(input, weight, bias=None, stride=2, compute="fp32"):
    if _only("up_layers.1.weight", weight):
        return F.conv_transpose2d(input, weight.transpose(2, 3), bias, stride)      # phases (0, 1) and (1, 0) swapped
    return F.conv_transpose2d(input, weight, bias, stride)


def m_conv_offset2d(input, offset, weight, stride=1, padding=0, dilation=1, deform_groups=1, compute="fp32"):
    fn = lambda x, o, w: conv_offset2d(x, o, w, stride, padding, dilation, deform_groups)
    if _only("odm_loc.1.weight", weight):
        def spoil(g, leaves, go):
            N, Ch, H, W = g[1].shape
            return [g[0], g[1].view(N, Ch // 2, 2, H, W).flip(2).reshape(N, Ch, H, W), g[2]]
        return _WrongGradient.apply(fn, spoil, input, offset, weight)
    return fn(input, offset, weight)


MUTANTS = dict(conv2d=m_conv2d, batch_norm=m_batch_norm, max_pool2d=m_max_pool2d, l2norm=m_l2norm,
               conv_transpose2d=m_conv_transpose2d, conv_offset2d=m_conv_offset2d)


# ---- one recorded step -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _state():
    net = build_net("train", 320, 21, 1024, 1, True, False)
    return synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)


def _step(ops, mutated=False):
    """one recorded forward_train + backward on the CPU with `ops` in place of the six -> (recorder, net, loss); the graph is kept"""
    mp = pytest.MonkeyPatch()
    try:
        for kind, fn in ops.items():
            mp.setattr(networks, kind, fn)
        mp.setattr(_lib, "require_cuda", lambda t, name="tensor": None)
        net = build_net("train", 320, 21, 1024, 1, True, False)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in _state().items()})
        assert net.training
        MUTATED_NET[0], POOLS[0] = (net if mutated else None), 0
        gen = torch.Generator().manual_seed(77)
        P = 3 * sum(f * f for f in MAPS)
        targets = tuple(torch.randn(1, P, w, generator=gen) for w in (4, 4, 21))
        with R.Recorder(net) as rec:
            out = net.forward_train(torch.from_numpy(synth.synth_frames(1, SIZE, seed=5)))
            loss = T.smooth_loss((out[0], out[2], out[3]), targets)
            loss.backward(retain_graph=True)
        assert networks.conv2d is ops["conv2d"], "the recorder did not restore the ops"
        return rec, net, loss
    finally:
        MUTATED_NET[0] = None
        mp.undo()


@functools.lru_cache(maxsize=None)
def _clean():
    rec, net, loss = _step(STAND_INS)
    rec.finish()
    return rec, net, loss


@functools.lru_cache(maxsize=None)
def _mutated():
    rec, net, loss = _step(MUTANTS, mutated=True)
    rec.finish()
    return rec


@pytest.fixture(scope="module", autouse=True)
def _release_the_recordings():
    """the two recorded steps keep their autograd graphs: given back when this file is done"""
    yield
    _mutated_failures.cache_clear()
    _mutated.cache_clear()
    _clean.cache_clear()


def _cancelling():
    zero_bias = T.bn_after_conv(_state().keys())
    assert len(zero_bias) == 17
    return set(zero_bias)


def _stage(stages, name):
    found = [st for st in stages if st.name == name]
    assert len(found) == 1, (name, found)
    return found[0]


def test_the_ops_are_restored_and_the_stages_are_the_modules_children():
    rec, net, _ = _clean()
    assert all(getattr(networks, k) is not STAND_INS[k] for k in R.KINDS)                 # monkeypatch undone as well
    kinds = [st.kind for st in rec.stages]
    assert {k: kinds.count(k) for k in R.KINDS} == dict(conv2d=37, batch_norm=17, max_pool2d=5, l2norm=2, conv_transpose2d=3,
                                                        conv_offset2d=8)
    assert [st.index for st in rec.stages] == list(range(len(rec.stages)))
    first = rec.stages[0]
    assert first.name == "backbone.0" and "input" not in first.grad_input and "grad_input.input" not in first.fired   # the image


@pytest.mark.parametrize("name", ["backbone.31", "arm_loc.1", "odm_conf.1"])
def test_recorder_is_exact(name):
    """(a): conv4_3's BatchNorm + ReLU output feeds L2Norm_4_3 and the next pool; arm_loc.1's output is an output of the net and the
    input of offset.1; odm_conf.1 has two activation inputs, one of them (the offset) shared with odm_loc.1"""
    rec, _, loss = _clean()
    st = _stage(rec.stages, name)
    roles = [r for r in R.ACTIVATIONS if r in st.live]
    assert roles == (["input", "offset"] if name == "odm_conf.1" else ["input"]) and set(st.grad_input) == set(roles)
    direct = torch.autograd.grad(loss, [st.output] + [st.live[r] for r in roles], retain_graph=True)
    assert R.bits_equal(direct[0], st.grad_output), "%s: grad_output" % name
    for r, g in zip(roles, direct[1:]):
        assert R.bits_equal(g, st.grad_input[r]), "%s: grad_input of %s" % (name, r)
    assert st.fired == dict({"grad_input." + r: 1 for r in roles}, grad_output=1)          # the direct pass recorded nothing
    # the two-consumer property the stage was chosen for: the op's grad_output is not what any single consumer sent
    if name == "backbone.31":
        consumers = [s for s in rec.stages if s.name in ("L2Norm_4_3", "max_pool2d.3")]
        assert len(consumers) == 2 and all(s.inputs["input"].shape == st.output.shape for s in consumers)
        assert all(not R.bits_equal(s.grad_input["input"], st.grad_output) for s in consumers)
        assert torch.allclose(sum(s.grad_input["input"] for s in consumers), st.grad_output, rtol=1e-5, atol=0)


def test_correct_fp32_ops_pass_every_stage():
    """(b): torch's own float32 ops on the CPU, judged by the checker; the worst share of a bound per op kind is the yardstick"""
    rec, _, _ = _clean()
    worst = R.check_stages(rec.stages, _cancelling())
    assert set(worst) == set(R.KINDS)
    assert all(share < 1.0 for share, _, _ in worst.values())


def _deep(stages):
    """the part of the net the mutated run re-checks: conv5_1 and everything behind it (maps of 12 x 12 and smaller, and the 24 x 24
    heads): every mutated stage, and every stage next to one"""
    first = _stage(stages, "backbone.34").index
    return lambda st: st.index >= first


@functools.lru_cache(maxsize=None)
def _mutated_failures():
    rec = _mutated()
    failures = {}
    R.check_stages(rec.stages, _cancelling(), select=_deep(rec.stages), failures=failures)
    return failures


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_fails_at_its_stage(name):
    """(c)"""
    failures = _mutated_failures()
    tensor, what = MUTATIONS[name]
    print("%s (%s): %s" % (name, what, failures.get(name)))
    assert name in failures, "%s passed the checker: %s" % (name, what)
    assert tensor in failures[name], "%s failed, but not at %s: %s" % (name, tensor, failures[name])


def test_mutations_fail_nowhere_else():
    """(c): every other stage of the re-checked part passes, in front of a mutated stage and behind it"""
    failures = _mutated_failures()
    checked = [st.name for st in R.select_stages(_mutated().stages, _deep(_mutated().stages))]
    assert set(MUTATIONS) <= set(checked) and len(checked) > 4 * len(MUTATIONS)
    assert set(failures) == set(MUTATIONS), {k: v for k, v in failures.items() if k not in MUTATIONS}


def test_a_written_input_trips_the_immutability_check():
    """(d)"""
    def scribbling(input, weight, bias=None, padding=0, dilation=1, compute="fp32", stride=1):
        out = F.conv2d(input, weight, bias, stride, padding, dilation)
        if weight.shape[:2] == (12, 512) and input.shape[2] == 3:           # arm_loc.3, the smallest map
            input.data[0, 0, 0, 0] += 1.0
        return out
    rec, _, _ = _step(dict(STAND_INS, conv2d=scribbling))
    with pytest.raises(AssertionError, match="arm_loc.3.*input was written to"):
        rec.finish()
