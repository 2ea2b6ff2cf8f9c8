"""One training step of the temporal ssd4scale_vgg (bn, deform, 8 deformable groups; fp32 and bf16) and of refinedet_vgg (bn,
use_refine, multihead; fp32) pinned op by op on the device: tests/_train_stage_ref.py's method through tests/_train_stage_k5.py, which
adds conv5x5 as a kind.  Every stage is judged from its OWN recorded inputs and grad_output against float64 on the CPU, elementwise;
tests/test_train_stage_k5_ref.py proves the checker on the CPU at this very input (192 px, batch 1, synthetic weights seed 0, frames
seed 5, ref_loc test_gpu_train_trn.py's constant, from tests/_train_model_harness.py) and shows that float32 torch ops stay inside its caps there.

The SSD4Scale net is recorded with separate loc / conf heads (_train_stage_k5.py says why).  In the bf16 step the conv-type and
deformable stages are checked; BatchNorm, pools and L2Norm run the same fp32 code as in the fp32 step.
"""
import functools

import pytest
import torch

import _train_model_harness as H
import _train_model_ref as N
import _train_stage_k5 as K
import _train_stage_ref as R
from tdrn_amd.model import refinedet_vgg, ssd4scale_vgg
from tdrn_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_num_threads(min(16, torch.get_num_threads()))

SIZE, MAPS, SEED = 192, (24, 12, 6, 3), 5
P = 3 * sum(f * f for f in MAPS)
SIXTEEN = R.CONV_TYPE + ("conv_offset2d", K.CONV5X5)
EXPECTED = {"refinedet": dict(conv2d=41, conv5x5=8, batch_norm=17, max_pool2d=5, l2norm=2, conv_transpose2d=3),
            "trn": dict(conv2d=21, conv_offset2d=8, batch_norm=17, max_pool2d=5, l2norm=2)}
GROUPS = ("conv1-4", "conv5-extras", "heads")


def _build(which):
    if which == "refinedet":
        return refinedet_vgg.build_net("train", 320, 21, True, 1024, True, True)
    net = ssd4scale_vgg.build_net("train", 320, 21, 1024, True, True)
    net._paired_heads = False
    return net


@functools.lru_cache(maxsize=None)
def _state(which):
    return synth.synth_state_dict({k: tuple(v.shape) for k, v in _build(which).state_dict().items()}, 0)


@functools.lru_cache(maxsize=None)
def _recorded(which, compute):
    """one recorded step on the device -> (the finished stages, the net's holder counts)"""
    net = _build(which)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in _state(which).items()})
    net = net.to(DEV)
    gen = torch.Generator().manual_seed(77)
    x = torch.from_numpy(synth.synth_frames(1, SIZE, seed=SEED)).to(DEV)
    with K.Recorder(net) as rec:
        if which == "refinedet":
            out = net.forward_train(x, compute)
            out, widths = (out[0], out[2], out[3]), (4, 4, 21)
        else:
            out = net.forward_train(x, [torch.from_numpy(m).to(DEV) for m in H.ref_loc("vgg", 1, SEED, SIZE, MAPS, 1)], compute)
            widths = (4, 21)
        N.smooth_loss(out, tuple(torch.randn(1, P, w, generator=gen) for w in widths)).backward()
    torch.cuda.synchronize()
    stages = rec.finish()
    assert all(st.output.is_cuda for st in stages)
    assert all(st.args["compute"] == compute for st in stages if "compute" in st.args)
    assert all(st.args["training"] is True for st in stages if st.kind == "batch_norm")
    return stages, K.holder_counts(net)


@pytest.fixture(scope="module", autouse=True)
def _release_the_recordings():
    yield
    _recorded.cache_clear()
    torch.cuda.empty_cache()


def _group(st):
    head = st.name.split(".")[0]
    if head in ("backbone", "max_pool2d"):
        return None                  # by position: see _groups
    return "conv5-extras" if head in ("extras", "L2Norm_4_3", "L2Norm_5_3") else "heads"


def _groups(stages):
    """stage name -> group; the trunk is cut behind conv4_3 (ten convs); a pool goes with the convs in front of it"""
    out, convs = {}, 0
    for st in stages:
        g = _group(st)
        if g is None:
            convs += st.kind == "conv2d"
            g = "conv1-4" if convs <= 10 else "conv5-extras"
        out[st.name] = g
    return out


CASES = [("trn", "fp32"), ("trn", "bf16"), ("refinedet", "fp32")]


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("which,compute", CASES)
def test_every_stage_of_a_training_step(which, compute, group):
    stages, _ = _recorded(which, compute)
    groups = _groups(stages)
    kinds = K.KINDS if compute == "fp32" else SIXTEEN
    select = lambda st: groups[st.name] == group and st.kind in kinds
    chosen = R.select_stages(stages, select)
    print("\n%s %s %s: %d stages" % (which, compute, group, len(chosen)))
    worst = K.check_stages(stages, set(N.bn_after_conv(_state(which).keys())), select)
    assert all(share < 1.0 for share, _, _ in worst.values())
    if group == "heads" and which == "refinedet":
        k5 = [st for st in chosen if st.kind == K.CONV5X5]
        assert len(k5) == 8 and all(set(st.grad_input) == {"input"} for st in k5)
    if group == "heads" and which == "trn":
        heads = [st for st in chosen if st.kind == "conv_offset2d"]
        assert len(heads) == 8 and all(st.args["deform_groups"] == 8 and set(st.grad_input) == {"input", "offset"} for st in heads)


@pytest.mark.parametrize("which", ["trn", "refinedet"])
def test_the_groups_cover_every_stage_and_the_counts_are_the_modules(which):
    stages, holders = _recorded(which, "fp32")
    kinds = [st.kind for st in stages]
    assert {k: kinds.count(k) for k in K.KINDS if kinds.count(k)} == holders == EXPECTED[which]
    groups = _groups(stages)
    assert len(groups) == len(stages) == sum(holders.values()) and set(groups.values()) == set(GROUPS)
