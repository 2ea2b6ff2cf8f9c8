"""One real training step of dualrefinedet_mobilenet (net.forward_train(x, compute), smooth_loss, backward) pinned op by op: every
call of the seven differentiable ops is recorded (tests/_train_stage_dw.py on tests/_train_stage_ref.py) and recomputed on the CPU
in float64 from its own recorded inputs and grad_output, elementwise, with the per-op bounds (the fp32 bound without its floor of 1).
tests/test_train_stage_mobilenet_ref.py proves the recorder and the depthwise check on the CPU, mutations included.

Cases.  Single head, 192 px, batch 2, frames seed 5.  Training mode in fp32: every stage.  Training mode in bf16: the dense
conv-type and deformable stages, and the depthwise stages, which compute in fp32 in every mode and so are held to the fp32 run's
rule.  Eval mode, fp32: the 33 BatchNorm stages (running statistics used and left untouched), on running statistics calibrated
on the input (_train_stage_dw.calibrate says why).

A step is recorded once per (compute, mode) and kept; the checks are parametrised over groups of stages so that the float64 work
of one test stays at a few seconds.
"""
import functools

import pytest
import torch

import _train_model_ref as T
import _train_stage_dw as W
import _train_stage_ref as R
from tdrn_amd.model.dualrefinedet_mobilenet import build_net
from tdrn_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_num_threads(min(16, torch.get_num_threads()))

SIZE, MAPS, B = 192, (24, 12, 6, 3), 2
EXPECTED = dict(conv2d=38, depthwise_conv2d=15, batch_norm=33, conv_transpose2d=3, l2norm=2, conv_offset2d=8)


@functools.lru_cache(maxsize=None)
def _state():
    net = build_net("train", 320, 21, 1, False)
    return synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)


@functools.lru_cache(maxsize=None)
def _recorded(compute, training=True):
    """one recorded step on the device -> the finished stages (the recorder's own four assertions have passed)"""
    net = build_net("train", 320, 21, 1, False)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in _state().items()})
    net = net.to(DEV)
    gen = torch.Generator().manual_seed(77)
    P = 3 * sum(f * f for f in MAPS)
    targets = tuple(torch.randn(1, P, w, generator=gen) for w in (4, 4, 21))
    x = torch.from_numpy(synth.synth_frames(B, SIZE, seed=5)).to(DEV)
    if not training:
        W.calibrate(net, x)          # running statistics under which the checker's ReLU-kink cap holds: see there
    with W.Recorder(net) as rec:
        out = net.forward_train(x, compute)
        loss = T.smooth_loss((out[0], out[2], out[3]), targets)
        loss.backward()
    torch.cuda.synchronize()
    stages = rec.finish()
    assert all(st.output.is_cuda for st in stages)
    assert all(st.args["compute"] == compute for st in stages if "compute" in st.args)
    assert all("compute" not in st.args for st in stages if st.kind == W.DEPTHWISE)
    assert all(st.args["training"] == training for st in stages if st.kind == "batch_norm")
    return stages


@pytest.fixture(scope="module", autouse=True)
def _release_the_recordings():
    """the recorded steps hold every activation and gradient of three steps on the device: given back when this file is done"""
    yield
    _recorded.cache_clear()
    torch.cuda.empty_cache()


def _groups(stages):
    """stage name -> group.  The trunk is cut behind backbone.3 and backbone.8"""
    out = {}
    for st in stages:
        head = st.name.split(".")[0]
        if head == "backbone":
            i = int(st.name.split(".")[1])
            out[st.name] = "trunk0-3" if i <= 3 else ("trunk4-8" if i <= 8 else "trunk9-13")
        elif head in ("L2Norm_4_3", "L2Norm_5_3", "extras", "arm_loc", "offset"):
            out[st.name] = "arm"
        elif head in ("last_layer_trans", "trans_layers", "up_layers", "latent_layers"):
            out[st.name] = "tcb"
        else:
            assert head in ("odm_loc", "odm_conf"), st
            out[st.name] = "heads"
    return out


GROUPS = ("trunk0-3", "trunk4-8", "trunk9-13", "arm", "tcb", "heads")
SIXTEEN = R.CONV_TYPE + ("conv_offset2d", W.DEPTHWISE)


def _check(stages, cancelling, select, what):
    chosen = R.select_stages(stages, select)
    print("\n%s: %d stages" % (what, len(chosen)))
    worst = W.check_stages(stages, cancelling, select)
    assert all(share < 1.0 for share, _, _ in worst.values())
    return chosen


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_single_head_batch2_training(compute, group):
    stages = _recorded(compute)
    groups = _groups(stages)
    kinds = W.KINDS if compute == "fp32" else SIXTEEN
    chosen = _check(stages, set(T.CANCELLING), lambda st: groups[st.name] == group and st.kind in kinds,
                    "single head %s %s" % (compute, group))
    if group == "heads":
        assert len(chosen) == 8 and all(st.kind == "conv_offset2d" and set(st.grad_input) == {"input", "offset"} for st in chosen)


def test_single_head_groups_cover_every_stage():
    stages = _recorded("fp32")
    groups = _groups(stages)
    kinds = [st.kind for st in stages]
    assert {k: kinds.count(k) for k in W.KINDS if kinds.count(k)} == EXPECTED
    assert len(stages) == 99 and set(groups.values()) == set(GROUPS) and len(groups) == len(stages)
    assert sum(st.kind in SIXTEEN for st in stages) == 64


def test_compute_does_not_reach_the_depthwise_op():
    """the op has no 16-bit mode: every depthwise stage of the bf16 step, run again through the fp32 op from its recorded inputs,
    gives the recorded output's bits"""
    from tdrn_amd.model import networks
    dw = [s for s in _recorded("bf16") if s.kind == W.DEPTHWISE]
    assert len(dw) == 15
    for st in dw:
        with torch.no_grad():
            y = networks.depthwise_conv2d(st.inputs["input"], st.inputs["weight"], None, st.args["stride"], st.args["padding"])
        assert R.bits_equal(y, st.output), st


def test_eval_mode_batch_norm_stages():
    stages = _recorded("fp32", training=False)
    chosen = _check(stages, (), "batch_norm", "eval mode, single head fp32")
    assert len(chosen) == 33 and all(st.args["training"] is False for st in chosen)
