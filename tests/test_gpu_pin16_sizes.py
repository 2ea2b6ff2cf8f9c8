"""The exact-input stage checks of test_gpu_pin16.py at the frame sizes of multi-scale testing (eval/tta.py: a 320-net also
runs 192, 384, 448, 512, 576 and 704 px frames, each size on a plan of its own: EngineModule.engine_for).

Which kernel a 3x3 layer gets depends on its map (conv_route.hip; conv3x3_tile_mode in kernels.h is the tile mode conv3x3_patch.hip,
conv3x3_pp.hip and conv3x3_ws.hip share); 320 and 512 px reach only a few of the geometries the kernels accept:

    tile mode         condition                       maps at 320 / 512 px       maps at the other sizes (checked below: *)
    8 x 32 tiles      W % 32 == 0, H % 8 == 0         320, 160 / 512 ... 32      96*, 192*, 224*, 448*, 288, 352, 576, 704
    16 x 16 tiles     W % 16 == 0, H % 16 == 0        80 (5 tiles per row)       48* (3 per row), 112* (7), 144 (9), 176 (11)
    flat 256-pixel    2 W + 258 <= 352 (W <= 47),     40, 20                     22*, 24*, 28*, 36, 44* (346 of the 352 patch rows)
      tiles           H W >= 400
    none: conv_igemm  any other 3x3 / s1 / p1 layer   10, 5 (below 400 pixels)   56*, 72, 88* (conv4_x, its TCB convs, unsplit);
                                                                                 3*, 6*, 7*, 11*, 12*, 14* (split-K 3 ... 16)

(144, 36 and 72 -- the 576 px plan -- are under the bit-for-bit plan equalities of test_gpu_pin16.py only.)  Every case proves
which family ran from the launch names of a profiled forward (conv3x3_patch_mfma:<layer> / conv_igemm_mfma:<layer>), asserts how
many stages were recomputed, and prints the worst error over tolerance per stage.  Bounds: those of test_gpu_pin16.py, unchanged.

The fp64 reference of every case was timed on the CPU (figures in the docstrings); the worst error over tolerance per stage is
printed by each case and has not been recorded for these sizes yet.
"""
import pytest
import torch

from tdrn_amd.utils import synth

import test_gpu_pin16 as pin

pytestmark = pytest.mark.gpu
DEV = pin.DEV
VGG_MH = ("dualrefinedet_vggbn", (320, 21, 1024, 1, True, True))
VGG_SH = ("dualrefinedet_vggbn", (320, 21, 1024, 1, True, False))
CONV3 = ("backbone.14", "backbone.17", "backbone.20")
CONV4 = ("backbone.24", "backbone.27", "backbone.30")
CONV5 = ("backbone.34", "backbone.37", "backbone.40")
PATCH, IGEMM = "conv3x3_patch_mfma", "conv_igemm_mfma"


def _families(net, x):
    """the launch names, '<kernel family>:<layer>', of one profiled forward of x, on a call of its own (not the one whose tensors are
    read back)"""
    eng = net.engine_for(x)
    eng.set_profile(1)
    net(x)
    torch.cuda.synchronize()
    fam = {o["name"] for o in eng.op_stats()}
    eng.set_profile(0)
    return fam


def _frames(batch, size, seed):
    return torch.from_numpy(synth.synth_frames(batch, size, seed=seed)).to(DEV)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_every_stage_192_batch3(dtype):
    """192 px, single head (the 5x5 branch refuses the 3x3 map), batch 3, every stage of image 1:
    conv1_2 on conv3x3_ws.hip with the first conv fused (SX = 6 tile columns, 216 units), conv2_x on 8 x 32 tiles at 96, conv3_x on
    16 x 16 tiles at 48 (3 per row), conv4_x and the 24 x 24 TCB convs on flat tiles (M = 3 * 576: 6.75 tiles, a tile spans 10.7
    rows), conv5_x at 12 / fc6, fc7 at 6 / the extras at 3 on conv_igemm with split-K 3 ... 16, heads on 24, 12, 6 and 3.
    fp64 reference: 1.8 s on 8 CPU threads."""
    net, sd = pin._build(VGG_SH[0], VGG_SH[1], phase="train", dtype=dtype)
    x = _frames(3, 192, seed=71)
    fam = _families(net, x)
    assert all(PATCH + ":" + n in fam for n in CONV3 + CONV4 + ("backbone.3", "backbone.7", "backbone.10")), fam
    assert all(IGEMM + ":" + n in fam for n in CONV5 + ("backbone.44", "extras.3", "last_layer_trans.0")), fam
    assert "first_conv:backbone.0" not in fam                        # (no launch of its own: computed by conv1_2's producers)
    report, checked = pin.check_stages(net, sd, x, dtype, images=(1,))
    pin._print_report("192 px %s batch 3" % dtype, report, checked)
    assert net.engine_for(x).fm == [24, 12, 6, 3]
    assert checked.get("conv", 0) >= 32 and checked.get("conv_transpose", 0) == 3 and checked.get("deform_heads", 0) == 4
    assert checked.get("l2norm", 0) == 2 and checked.get("maxpool", 0) >= 2


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_every_stage_448_batch2(dtype):
    """448 px, multihead, batch 2, every stage of image 1:
    8 x 32 tiles at 448 and 224, conv3_x on 16 x 16 tiles at 112 (7 per row), conv4_x and the 56 x 56 TCB convs on conv_igemm (no
    tile mode takes W = 56; unsplit: 49 blocks of 128 pixels x 4 cout tiles), conv5_x (Cin 512) and the 28 x 28 TCB convs on flat
    tiles, fc6 ... the 7 x 7 level on conv_igemm with split-K 4 ... 16, ConvTranspose 7 -> 14 -> 28 -> 56, heads on 56, 28, 14 and
    7 with the 5x5 branch on the odd 7 x 7 map.
    fp64 reference: 5.9 s on 8 CPU threads."""
    net, sd = pin._build(VGG_MH[0], VGG_MH[1], phase="train", dtype=dtype)
    x = _frames(2, 448, seed=73)
    fam = _families(net, x)
    assert all(IGEMM + ":" + n in fam for n in CONV4 + ("trans_layers.0.0", "trans_layers.0.2", "latent_layers.2")), fam
    assert all(PATCH + ":" + n in fam for n in CONV3 + CONV5 + ("trans_layers.1.0", "trans_layers.1.2", "latent_layers.1")), fam
    report, checked = pin.check_stages(net, sd, x, dtype, images=(1,))
    pin._print_report("448 px %s batch 2" % dtype, report, checked)
    assert net.engine_for(x).fm == [56, 28, 14, 7]
    assert checked.get("conv", 0) >= 32 and checked.get("conv_transpose", 0) == 3 and checked.get("deform_heads", 0) == 4
    assert checked.get("l2norm", 0) == 2 and checked.get("maxpool", 0) >= 2


def _from_conv4(op, in_hw):
    return in_hw[1] <= 88


def _from_conv5(op, in_hw):
    return in_hw[1] <= 44 or op["kind"] == "deform_heads"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_stages_behind_conv4_704_batch13(dtype):
    """704 px, multihead, batch 13, first and last image, the ops on maps of 44 and below plus all four heads:
    conv5_x at 44 x 44, the flat-mode limit (2 * 44 + 258 = 346 of the 352 patch rows), with ceil(13 * 1936 / 256) * 2 = 198 items:
    at or above the 192 of launch_conv3x3_pp, so conv3x3_pp.hip runs it in flat mode, the last image's tiles the ragged ones;
    fc6 (dilated, unsplit) and fc7 at 22 on conv_igemm, the 44 x 44 and 22 x 22 TCB convs on flat tiles, the 11 x 11 level with
    split-K 4 ... 13, heads on 88, 44, 22 and 11.  (conv4_x and its TCB convs at 88 are left to the batch-2 case below: with them
    the fp64 reference of two images takes 10 s on 8 CPU threads, without them 4.6 s.)"""
    net, sd = pin._build(VGG_MH[0], VGG_MH[1], phase="train", dtype=dtype)
    x = _frames(13, 704, seed=75)
    assert -(-13 * 44 * 44 // 256) * (512 // 256) == 198
    fam = _families(net, x)
    assert all(PATCH + ":" + n in fam for n in CONV5 + ("trans_layers.1.0", "trans_layers.2.0", "latent_layers.0")), fam
    assert all(IGEMM + ":" + n in fam for n in CONV4 + ("backbone.44", "backbone.47", "trans_layers.0.0")), fam
    report, checked = pin.check_stages(net, sd, x, dtype, images=(0, 12), stages=_from_conv5)
    pin._print_report("704 px %s batch 13, maps <= 44 + heads" % dtype, report, checked)
    assert net.engine_for(x).fm == [88, 44, 22, 11]
    assert checked == {"conv": 19, "l2norm": 1, "maxpool": 1, "conv_transpose": 3, "deform_heads": 4}


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_stages_behind_conv3_704_batch2(dtype):
    """704 px at batch 2, last image, the ops on maps of 88 and below: 16 pixel tiles x 2 cout tiles at 44 x 44 are far below
    conv3x3_pp's 192 items, so conv5_x stays on conv3x3_patch.hip in flat mode at W = 44, in 64-cout items (16 x 4 128-cout items would be fewer than
    160); the 16th tile is ragged and the 8th spans both images.  conv4_x (Cin 256 / 512, 7744 pixels per image) and its TCB convs
    at 88 on conv_igemm, unsplit.  fp64 reference: 5 s on 8 CPU threads."""
    net, sd = pin._build(VGG_MH[0], VGG_MH[1], phase="train", dtype=dtype)
    x = _frames(2, 704, seed=77)
    fam = _families(net, x)
    assert all(PATCH + ":" + n in fam for n in CONV5), fam
    assert all(IGEMM + ":" + n in fam for n in CONV4 + ("trans_layers.0.0", "trans_layers.0.2", "latent_layers.2")), fam
    report, checked = pin.check_stages(net, sd, x, dtype, images=(1,), stages=_from_conv4)
    pin._print_report("704 px %s batch 2, maps <= 88" % dtype, report, checked)
    assert checked == {"conv": 26, "l2norm": 2, "maxpool": 2, "conv_transpose": 3, "deform_heads": 4}


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_every_stage_mobilenet_448(dtype):
    """test_every_stage_mobilenet's default plan at 448 px, batch 2: the stride-2 first conv to 224, depthwise strips and the sliding
    window at 224, 112, 56 and 28, the stride-2 depthwise layers 224 -> 112 -> 56 -> 28 -> 14 -> 7 (even to odd at the last one), the
    1x1 GEMMs on pw1x1, the 28 x 28 TCB convs on flat tiles, the 56 x 56 ones on conv_igemm.  fp64 reference: 3.5 s on 8 CPU threads."""
    net, sd = pin._build("dualrefinedet_mobilenet", (320, 21, 1, True), phase="train", dtype=dtype)
    x = _frames(2, 448, seed=79)
    fam = _families(net, x)
    assert all(PATCH + ":" + n in fam for n in ("trans_layers.1.0", "trans_layers.1.2", "latent_layers.1")), fam
    assert all(IGEMM + ":" + n in fam for n in ("trans_layers.0.0", "trans_layers.0.2", "latent_layers.2")), fam
    report, checked = pin.check_stages(net, sd, x, dtype, images=(1,))
    pin._print_report("mobilenet 448 px %s" % dtype, report, checked)
    ops = net.engine_for(x).op_infos()
    assert sum(1 for o in ops if o["kind"] == "depthwise" and o["fused_dw"]) == 0
    assert sum(1 for o in ops if o["kind"] == "depthwise" and o["stride"] == 2) == 5
    assert checked.get("depthwise", 0) == 15 and checked.get("conv", 0) >= 30 and checked.get("first_conv", 0) == 1
    assert checked.get("conv_transpose", 0) == 3 and checked.get("deform_heads", 0) == 4
