"""The in-net launches of the fused gather kernel, deform_gemm_kernel<bf16_t | f16_t> (csrc/deform.hip), from their own inputs:
check (d) of tests/test_gpu_pin16.py (check_stages -> _check_gather) on every plan that keeps a deformable head off the
transform-then-sample path.

    dualrefinedet_vggbn under TDRN_PLAN_NO_DEFORM_TS   four pyramid levels in ONE launch; multihead: the 3x3 and the 5x5 branch as two
                                                       work items that add atomically into zeroed outputs; single head: one item
    ... at 81 classes                                  12 + 243 = 255 columns in two ranges of 128 (net_run.hip run_deform_gather), the
                                                       second range's conf pointer re-based
    ssd4scale_vgg / ssd4scale_mobile temporal nets     8 deformable groups in two halves of four ([g_begin, g_end) of every tap) that
                                                       add atomically; 21 and 31 classes (75 / 105 columns: NTL = 3 / 4)
    a TRN clip with fewer key frames than frames       the offsets of Bk key frames broadcast over F * Bk frames (off_rows)

Every case asserts that all four heads are on the gather kernel (op["y"] == -1), that a profiled forward names the kernel's launch
family (deform_gemm_mfma:<head>), that four heads were recomputed, and (in _check_gather) that `near` stays below HW // 4 at every
level.  Only the heads are recomputed here (stages=...): the other launches of these plans are pinned by the other files.
Bounds: C_ACC * S + extra of tests/test_gpu_pin16.py, unchanged."""
import pytest
import torch

from tdrn_amd import _lib
from tdrn_amd.utils import synth

import test_gpu_net as tgn
import test_gpu_pin16 as pin

pytestmark = pytest.mark.gpu
DEV = pin.DEV


def _heads(op, in_hw):
    return op["kind"] == "deform_heads"


def _families(net, x, forward):
    """the launch names '<kernel family>:<layer>' of one profiled forward (as tests/test_gpu_pin16_sizes.py _families, through `forward`)"""
    eng = net.engine_for(x)
    eng.set_profile(1)
    forward(x)
    torch.cuda.synchronize()
    fam = {o["name"] for o in eng.op_stats()}
    eng.set_profile(0)
    return fam


def _check_heads(title, net, sd, x, dtype, images, forward=None, key_frames=None):
    forward = forward or net
    fam = _families(net, x, forward)
    heads = [o for o in net.engine_for(x).op_infos() if o["kind"] == "deform_heads"]
    assert len(heads) == 4 and all(o["y"] == -1 for o in heads), [o["y"] for o in heads]
    assert any(n.startswith("deform_gemm_mfma:") for n in fam), fam
    report, checked = pin.check_stages(net, sd, x, dtype, images=images, forward=forward, stages=_heads, key_frames=key_frames)
    pin._print_report(title, report, checked)
    assert checked == {"deform_heads": 4}
    assert len(report) == 4 * len(images) and all(n.endswith(":gather") for n, _, _, _ in report)
    return heads


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("classes", [21, 81])
@pytest.mark.parametrize("multihead", [True, False], ids=["multihead", "single_head"])
def test_drn_heads_on_the_gather_kernel(multihead, classes, dtype):
    """dualrefinedet_vggbn under TDRN_PLAN_NO_DEFORM_TS, 320 px, batch 2, raw logits, image 1 recomputed"""
    net, sd = pin._build("dualrefinedet_vggbn", (320, classes, 1024, 1, True, multihead), phase="train", dtype=dtype, flags=_lib.PLAN_NO_DEFORM_TS)
    x = torch.from_numpy(synth.synth_frames(2, 320, seed=91)).to(DEV)
    heads = _check_heads("gather heads, %s, %d classes, %s" % ("multihead" if multihead else "single head", classes, dtype), net, sd, x, dtype, (1,))
    assert all(o["n_branches"] == (2 if multihead else 1) and o["groups"] == 1 for o in heads)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("classes", [21, 31])
@pytest.mark.parametrize("model,targs,sargs", [("ssd4scale_vgg", (1024, True, True), (1024, True, False)),
                                               ("ssd4scale_mobile", (1024, True), (1024, False))], ids=["vgg", "mobile"])
def test_trn_temporal_heads_on_the_gather_kernel(model, targs, sargs, classes, dtype):
    """the temporal nets' grouped heads (df_group = 8, two halves of four groups), ref_loc from the static net, batch 2, image 1"""
    net, sd = pin._build(model, (320, classes) + targs, phase="train", seed=1, dtype=dtype)
    stat, _ = tgn._build(model, (320, classes) + sargs, seed=0)
    x = torch.from_numpy(synth.synth_frames(2, 320, seed=92)).to(DEV)
    maps = stat(x, ret_loc=True)[2]
    heads = _check_heads("TRN heads, %s, %d classes, %s" % (model, classes, dtype), net, sd, x, dtype, (1,), forward=lambda xx: net(xx, ref_loc=maps))
    assert all(o["groups"] == 8 and o["n_branches"] == 1 for o in heads)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_trn_clip_heads_under_the_key_frame_broadcast(dtype):
    """one temporal forward over two clips of two frames (frame-major: frames 0, 1 are the key frames, frame i reads the offsets of key
    frame i % 2): the offset tensors hold two frames for a batch of four (off_rows).  Frames 1 and 2 recomputed: frame 2 must read
    key frame 0's offsets, frame 1 its own."""
    Bk, F = 2, 2
    net, sd = pin._build("ssd4scale_vgg", (320, 21, 1024, True, True), phase="train", seed=1, dtype=dtype)
    stat, _ = tgn._build("ssd4scale_vgg", (320, 21, 1024, True, False), seed=0)
    x = torch.from_numpy(synth.synth_frames(F * Bk, 320, seed=93)).to(DEV)
    maps = stat(x[:Bk], ret_loc=True)[2]
    assert maps[0].shape[0] == Bk
    _check_heads("TRN clip heads, %d key frames for %d frames, %s" % (Bk, F * Bk, dtype), net, sd, x, dtype, (1, 2),
                 forward=lambda xx: net(xx, ref_loc=maps), key_frames=Bk)
