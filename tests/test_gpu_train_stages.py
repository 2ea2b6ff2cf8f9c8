"""One real training step of dualrefinedet_vggbn (net.forward_train(x, compute), smooth_loss, backward) pinned op by op: every call of
the six differentiable ops is recorded (tests/_train_stage_ref.py) and recomputed on the CPU in float64 from its own recorded inputs
and grad_output, elementwise, with the per-op files' bounds (the fp32 bound without its floor of 1: that module's docstring says
why).  tests/test_train_stage_ref.py proves the recorder and the checker on the CPU, mutations included.

What tests/test_gpu_train_net.py cannot see and this file does: gradients at batch 2 in training mode (batch statistics across
images, wgrad chunks that cross images) at the net's own shapes, elementwise; the bf16 and fp16 compute types, gated; the eval-mode
BatchNorm path under a real grad_output.

Cases.  Single head, 192 px (the smallest input the 3 x 3 deformable heads accept), batch 2, training mode, in fp32 (every stage),
bf16 and fp16 (the conv-type and deformable stages: BatchNorm, pools and L2Norm run the same fp32 code as in the fp32 run).
Multihead, 320 px (5 x 5 heads), batch 2, training mode, fp32 and bf16: the stages the single-head run does not contain, the
offset2 convs and the 5 x 5 heads, whose grad_output is shared with the 3 x 3 heads through the head sum.  Eval mode, single head,
192 px, batch 2, fp32: the BatchNorm stages (running statistics used and left untouched, gradients through fixed statistics).

A step is recorded once per (multihead, compute, mode) and kept; the checks are parametrised over groups of stages so that the
float64 work of one test stays at a few seconds.
"""
import functools

import pytest
import torch

import _train_model_ref as T
import _train_stage_ref as R
from tdrn_amd.model.dualrefinedet_vggbn import build_net
from tdrn_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_num_threads(min(16, torch.get_num_threads()))

CONFIG = {False: (192, (24, 12, 6, 3)), True: (320, (40, 20, 10, 5))}      # test_gpu_train_net.py's
B = 2


@functools.lru_cache(maxsize=None)
def _state(mh):
    net = build_net("train", 320, 21, 1024, 1, True, mh)
    return synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)


@functools.lru_cache(maxsize=None)
def _recorded(mh, compute, training=True):
    """one recorded step on the device -> the finished stages (the recorder's own four assertions have passed)"""
    net = build_net("train", 320, 21, 1024, 1, True, mh)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in _state(mh).items()})
    net = net.to(DEV).train(training)
    size, maps = CONFIG[mh]
    gen = torch.Generator().manual_seed(77)
    P = 3 * sum(f * f for f in maps)
    targets = tuple(torch.randn(1, P, w, generator=gen) for w in (4, 4, 21))
    x = torch.from_numpy(synth.synth_frames(B, size, seed=5)).to(DEV)
    with R.Recorder(net) as rec:
        out = net.forward_train(x, compute)
        loss = T.smooth_loss((out[0], out[2], out[3]), targets)
        loss.backward()
    torch.cuda.synchronize()
    stages = rec.finish()
    assert all(st.output.is_cuda for st in stages)
    assert all(st.args["compute"] == compute for st in stages if "compute" in st.args)
    assert all(st.args["training"] == training for st in stages if st.kind == "batch_norm")
    return stages


@pytest.fixture(scope="module", autouse=True)
def _release_the_recordings():
    """the recorded steps hold every activation and gradient of six steps on the device: given back when this file is done"""
    yield
    _recorded.cache_clear()
    torch.cuda.empty_cache()


def _cancelling(mh):
    zero_bias = T.bn_after_conv(_state(mh).keys())
    assert len(zero_bias) == 17
    return set(zero_bias)


def _groups(stages):
    """stage name -> group.  The backbone is cut at conv3_1 and conv5_1 (a pool goes with the convs in front of it)"""
    out, current = {}, "conv1-2"
    for st in stages:
        head = st.name.split(".")[0]
        if head == "backbone":
            i = int(st.name.split(".")[1])
            current = "conv1-2" if i < 14 else ("conv3-4" if i < 34 else "conv5-fc7")
        elif head in ("L2Norm_4_3", "L2Norm_5_3", "extras", "arm_loc", "offset", "offset2"):
            current = "arm"
        elif head in ("last_layer_trans", "trans_layers", "up_layers", "latent_layers"):
            current = "tcb"
        elif head in ("odm_loc", "odm_conf", "odm_loc_2", "odm_conf_2"):
            current = "heads"
        else:
            assert st.kind == "max_pool2d" and current in ("conv1-2", "conv3-4", "conv5-fc7"), st
        out[st.name] = current
    return out


GROUPS = ("conv1-2", "conv3-4", "conv5-fc7", "arm", "tcb", "heads")
SIXTEEN = R.CONV_TYPE + ("conv_offset2d",)


def _check(stages, cancelling, select, what):
    chosen = R.select_stages(stages, select)
    print("\n%s: %d stages" % (what, len(chosen)))
    worst = R.check_stages(stages, cancelling, select)
    assert all(share < 1.0 for share, _, _ in worst.values())
    return chosen


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("compute", ["fp32", "bf16", "fp16"])
def test_single_head_batch2_training(compute, group):
    stages = _recorded(False, compute)
    groups = _groups(stages)
    kinds = R.KINDS if compute == "fp32" else SIXTEEN
    chosen = _check(stages, _cancelling(False), lambda st: groups[st.name] == group and st.kind in kinds,
                    "single head %s %s" % (compute, group))
    if group == "heads":
        assert len(chosen) == 8 and all(st.kind == "conv_offset2d" and set(st.grad_input) == {"input", "offset"} for st in chosen)


def test_single_head_groups_cover_every_stage():
    stages = _recorded(False, "fp32")
    groups = _groups(stages)
    assert len(stages) == 72 and set(groups.values()) == set(GROUPS) and len(groups) == len(stages)
    assert sum(st.kind in SIXTEEN for st in stages) == 48


SECOND = {"offset2": ("offset2", (0, 1, 2, 3)), "odm_loc_2-level0": ("odm_loc_2", (0,)), "odm_loc_2-levels1-3": ("odm_loc_2", (1, 2, 3)),
          "odm_conf_2-level0": ("odm_conf_2", (0,)), "odm_conf_2-levels1-3": ("odm_conf_2", (1, 2, 3))}


@pytest.mark.parametrize("part", list(SECOND))
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_multihead_batch2_training_second_heads(compute, part):
    stages = _recorded(True, compute)
    head, levels = SECOND[part]
    chosen = _check(stages, _cancelling(True), lambda st: st.name in ["%s.%d" % (head, s) for s in levels], "multihead %s %s" % (compute, part))
    assert len(chosen) == len(levels)
    if head != "offset2":
        # the 5 x 5 head and the 3 x 3 head of a level were handed one grad_output: the head sum's
        for st in chosen:
            twin = [s for s in stages if s.name == st.name.replace("_2", "")]
            assert len(twin) == 1 and st.args["padding"] == (2, 2) and tuple(st.inputs["weight"].shape[2:]) == (5, 5)
            assert R.bits_equal(st.grad_output, twin[0].grad_output), st


def test_eval_mode_batch_norm_stages():
    stages = _recorded(False, "fp32", training=False)
    chosen = _check(stages, (), "batch_norm", "eval mode, single head fp32")
    assert len(chosen) == 17 and all(st.args["training"] is False for st in chosen)
