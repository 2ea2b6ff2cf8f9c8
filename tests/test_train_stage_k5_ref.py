"""tests/_train_stage_k5.py proved on the CPU before it judges the kernels (no GPU): the ops of tdrn_amd.model.networks are replaced by
float32 torch stand-ins of the same signatures (test_train_stage_mobilenet_ref.py's seven and F.conv2d(padding=2) for conv5x5), one
training step of refinedet_vgg (bn, use_refine, multihead) and one of the temporal ssd4scale_vgg (bn, deform, separate heads) run on
the CPU (192 px, batch 1, synthetic weights seed 0, frames seed 5; ref_loc: test_gpu_train_trn.py's constant), and

  (a) the stages are the module's holders, the counts derived from the module (refinedet_vgg: 8 conv5x5 among them; ssd4scale_vgg:
      8 conv_offset2d and the four 1x1 offset convs); every parameter in exactly one stage, every hook fired once (Recorder.finish);
  (b) a correct fp32 implementation passes every stage, so the references alone stay inside the checker's caps at this input (ReLU
      kink <= 1 % of a stage, near_decision <= max(2, numel // 1000)); the worst share per kind is printed: the yardstick of DESIGN.md;
  (c) two planted mutations each fail at their own stage and nowhere else: a 5x5 stand-in whose weight gradient lacks kernel row 2
      (odm_conf_2.1: what a row pass of the HIP kernel that wrote no slab rows would give), and a deformable stand-in that samples
      with the offsets of the level before it (arm_conf.1 with level 0's, cropped to its map).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import _train_model_harness as H
import _train_model_ref as N
import _train_stage_k5 as K
import _train_stage_ref as R
import test_train_stage_mobilenet_ref as M
import test_train_stage_ref as V
from tdrn_amd import _lib
from tdrn_amd.model import networks, refinedet_vgg, ssd4scale_vgg
from tdrn_amd.utils import synth

torch.set_num_threads(min(16, torch.get_num_threads()))
SIZE, MAPS, SEED = 192, (24, 12, 6, 3), 5
P = 3 * sum(f * f for f in MAPS)
NETS = ("refinedet", "trn")


def conv5x5(input, weight, bias=None, compute="fp32"):
    return F.conv2d(input, weight, bias, 1, 2)


STAND_INS = dict(M.STAND_INS, conv5x5=conv5x5)
MUTATED = [None]
LAST_OFFSET = [None]
MUTATIONS = {"refinedet": {"odm_conf_2.1": ("grad_weight", "kernel row 2 of the 5x5 weight gradient dropped")},
             "trn": {"arm_conf.1": ("output", "a head sampling with the offsets of the level before it")}}
NEAR = {"refinedet": {"odm_loc.1", "odm_conf.1", "odm_loc_2.1", "odm_conf_2.1", "odm_conf_2.0", "odm_conf_2.2", "latent_layers.1"},
        "trn": {"arm_loc.0", "arm_conf.0", "offset.0", "offset.1", "arm_loc.1", "arm_conf.1", "arm_loc.2", "arm_conf.2"}}


def _is(name, weight):
    return MUTATED[0] is not None and weight is dict(MUTATED[0].named_parameters())[name]


def m_conv5x5(input, weight, bias=None, compute="fp32"):
    if _is("odm_conf_2.1.weight", weight):
        def spoil(g, leaves, go):
            g[1] = g[1].clone()
            g[1][:, :, 2, :] = 0
            return g
        return V._WrongGradient.apply(lambda x, w, b: F.conv2d(x, w, b, 1, 2), spoil, input, weight, bias)
    return conv5x5(input, weight, bias, compute)


def m_conv_offset2d(input, offset, weight, stride=1, padding=0, dilation=1, deform_groups=1, compute="fp32"):
    used = offset
    if _is("arm_conf.1.weight", weight):
        H, W = offset.shape[2:]
        used = LAST_OFFSET[0][:, :, :H, :W] + 0 * offset          # (the given offsets still get a gradient: zeros)
    elif _is("arm_conf.0.weight", weight):
        LAST_OFFSET[0] = offset.detach().clone()
    return V.conv_offset2d(input, used, weight, stride, padding, dilation, deform_groups)


MUTANTS = dict(STAND_INS, conv5x5=m_conv5x5, conv_offset2d=m_conv_offset2d)


def _build(which):
    if which == "refinedet":
        return refinedet_vgg.build_net("train", 320, 21, True, 1024, True, True)
    net = ssd4scale_vgg.build_net("train", 320, 21, 1024, True, True)
    net._paired_heads = False          # _train_stage_k5.py says why
    return net


@functools.lru_cache(maxsize=None)
def _state(which):
    return synth.synth_state_dict({k: tuple(v.shape) for k, v in _build(which).state_dict().items()}, 0)


@functools.lru_cache(maxsize=None)
def _step(which, mutated=False):
    """one recorded forward_train + backward on the CPU with the stand-ins in place of the ops -> (finished recorder, net)"""
    ops = MUTANTS if mutated else STAND_INS
    mp = pytest.MonkeyPatch()
    try:
        for kind, fn in ops.items():
            mp.setattr(networks, kind, fn)
        mp.setattr(_lib, "require_cuda", lambda t, name="tensor": None)
        net = _build(which)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in _state(which).items()})
        assert net.training
        MUTATED[0] = net if mutated else None
        gen = torch.Generator().manual_seed(77)
        x = torch.from_numpy(synth.synth_frames(1, SIZE, seed=SEED))
        with K.Recorder(net) as rec:
            if which == "refinedet":
                out = net.forward_train(x)
                out = (out[0], out[2], out[3])
                widths = (4, 4, 21)
            else:
                out = net.forward_train(x, [torch.from_numpy(m) for m in H.ref_loc("vgg", 1, SEED, SIZE, MAPS, 1)])
                widths = (4, 21)
            targets = tuple(torch.randn(1, P, w, generator=gen) for w in widths)
            N.smooth_loss(out, targets).backward()
        assert networks.conv5x5 is ops["conv5x5"], "the recorder did not restore the ops"
        rec.finish()
        return rec, net
    finally:
        MUTATED[0] = LAST_OFFSET[0] = None
        mp.undo()


@pytest.fixture(scope="module", autouse=True)
def _release_the_recordings():
    yield
    _step.cache_clear()


def _cancelling(which):
    return set(N.bn_after_conv(_state(which).keys()))


@pytest.mark.parametrize("which", NETS)
def test_the_ops_are_restored_and_the_stages_are_the_modules_holders(which):
    rec, net = _step(which)
    assert all(getattr(networks, k) is not STAND_INS[k] for k in K.KINDS)
    kinds = [st.kind for st in rec.stages]
    want = K.holder_counts(net)
    assert {k: kinds.count(k) for k in K.KINDS if kinds.count(k)} == want
    assert [st.index for st in rec.stages] == list(range(sum(want.values())))
    assert len(_cancelling(which)) == 17
    if which == "refinedet":
        # 15 trunk + 2 extras + 4 arm_loc + 3 last_layer_trans + 6 trans + 3 latent + 8 ODM 3x3 convs; 8 ODM 5x5 convs
        assert want == dict(conv2d=41, conv5x5=8, batch_norm=17, max_pool2d=5, l2norm=2, conv_transpose2d=3)
        k5 = [st for st in rec.stages if st.kind == K.CONV5X5]
        assert [st.name for st in k5] == [n % s for s in range(4) for n in ("odm_loc_2.%d", "odm_conf_2.%d")]
        assert all(set(st.grad_input) == {"input"} and "bias" in st.inputs and st.args["compute"] == "fp32" for st in k5)
        assert [tuple(st.inputs["input"].shape[2:]) for st in k5] == [(f, f) for f in MAPS for _ in range(2)]
    else:
        # 15 trunk + 2 extras + the four 1x1 offset convs; 8 deformable heads with 8 groups
        assert want == dict(conv2d=21, conv_offset2d=8, batch_norm=17, max_pool2d=5, l2norm=2)
        heads = [st for st in rec.stages if st.kind == "conv_offset2d"]
        assert [st.name for st in heads] == [n % s for s in range(4) for n in ("arm_loc.%d", "arm_conf.%d")]
        assert all(st.args["deform_groups"] == 8 and set(st.grad_input) == {"input", "offset"} for st in heads)
        offs = [st for st in rec.stages if st.name.startswith("offset.")]
        assert len(offs) == 4 and all("input" not in st.grad_input for st in offs)          # ref_loc is a constant


@pytest.mark.parametrize("which", NETS)
def test_correct_fp32_ops_pass_every_stage(which):
    rec, net = _step(which)
    worst = K.check_stages(rec.stages, _cancelling(which))
    assert set(worst) == set(K.holder_counts(net))
    assert all(share < 1.0 for share, _, _ in worst.values())


@pytest.mark.parametrize("which", NETS)
def test_mutations_fail_at_their_stage_and_nowhere_else(which):
    rec, _ = _step(which, True)
    near, failures = NEAR[which], {}
    chosen = R.select_stages(rec.stages, lambda st: st.name in near)
    assert len(chosen) == len(near)
    K.check_stages(rec.stages, _cancelling(which), select=lambda st: st.name in near, failures=failures)
    for name, (tensor, what) in MUTATIONS[which].items():
        print("%s (%s): %s" % (name, what, failures.get(name)))
        assert name in failures and tensor in failures[name], (name, what, failures.get(name))
    assert set(failures) == set(MUTATIONS[which]), failures
