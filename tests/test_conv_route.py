"""Which kernel runs each dense conv layer (csrc/conv_route.hip), asked of the library without a GPU: the `plan:` lines a net prints
under TDRN_PLAN_DUMP end in conv_kernel_name(conv_route) at batch 1 / at the planner's reference batch 32.

The expected pairs are worked out by hand from the kernels' criteria (and agree with the kernel names in a GPU trace of the commit
before conv_route existed, profiles/conv_route):
  * conv3x3_ws: pooled, 16-bit, Cin = 64, from 192 units; a unit is a run of 8 x 32 tiles of one tile column.  320 px: 10 columns of
    40 tiles, cheapest split 20 runs of 2 -> 200 units for ONE frame already: ws at every batch.  192 px: 6 columns of 24 tiles, at
    most 72 units for one frame -> patch; 768 units (runs of 6) at batch 32 -> ws.
  * conv3x3_pp: unpooled, 16-bit, Cin >= 256, Npad % 256 == 0, from 192 items of 256 pixels x 256 couts.  40 x 40 (flat tiles), 512
    couts: ceil(1600 B / 256) * 2 = 14 items at batch 1 -> patch, 400 at batch 32 -> pp.  Cin = 128 (conv3_1) and pooled layers never.
  * head3x3: 16-bit, fp32 output of <= 16 columns, levels of >= 400 pixels, at any batch; the 10 x 10 level stays on igemm (split-K).
  * pw1x1: 16-bit 1 x 1, Npad % 256 == 0, from 192 items: MobileNet's 512 -> 512 layers at 40 x 40 have 14 / 400 items.
  * a split layer, and every 3 x 3 layer below 400 pixels, runs on igemm; fp32 nets know igemm and patch only.
"""
import ctypes as C
import os
import re
import tempfile

import pytest

from tdrn_amd import _lib

DIRECT = {"patch", "pp", "ws"}


def routes(model, size, dtype, flags=0):
    """{layer: (kernel at batch 1, kernel at batch 32, splitk)} of one net, from the library's own plan lines (stderr)."""
    lib = _lib.lib()
    cfg = _lib.NetConfig(c7_channel=1024, model=model, size=size, num_classes=21, def_groups=1, bn=1, multihead=0, deform=0,
                         test_phase=1, dtype=dtype, use_refine=0, plan_flags=flags)
    net = C.c_void_p()
    old_env = os.environ.get("TDRN_PLAN_DUMP")
    os.environ["TDRN_PLAN_DUMP"] = "1"
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        try:
            os.dup2(tmp.fileno(), 2)
            rc = lib.tdrn_net_create(C.byref(cfg), C.byref(net))
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            if old_env is None:
                del os.environ["TDRN_PLAN_DUMP"]
            else:
                os.environ["TDRN_PLAN_DUMP"] = old_env
        assert rc == 0
        lib.tdrn_net_destroy(net)
        tmp.seek(0)
        text = tmp.read().decode()
    out = {}
    for m in re.finditer(r"^plan: (\S+) .* splitk (\d+)  (\w+)/(\w+)  chain", text, re.M):
        out[m.group(1)] = (m.group(3), m.group(4), int(m.group(2)))
    assert out
    return out


@pytest.fixture(scope="module")
def vgg():
    return routes(_lib.DRN_VGGBN, 320, _lib.BF16)


@pytest.fixture(scope="module")
def mobile():
    return routes(_lib.DRN_MOBILENET, 320, _lib.BF16)


def pair(r, name):
    return r[name][:2]


def moved(base, other):
    return {k for k in base if base[k][:2] != other[k][:2]}


def test_vgg_layers_on_each_side_of_every_rule(vgg):
    assert pair(vgg, "backbone.3") == ("ws", "ws")               # conv1_2: pooled, Cin 64, 200 units for one 320-px frame
    assert pair(vgg, "backbone.7") == ("patch", "patch")         # conv2_1: Cin 64 but a full-resolution output
    assert pair(vgg, "backbone.14") == ("patch", "patch")        # conv3_1: Cin 128 stays on patch
    assert pair(vgg, "backbone.17") == ("patch", "pp")           # conv3_2: 80 x 80, 25 items a frame
    assert pair(vgg, "backbone.20") == ("patch", "patch")        # conv3_3: Cin 256 but pooled
    assert pair(vgg, "backbone.27") == ("patch", "pp")           # conv4_2: Cin 512 at 40 x 40
    assert pair(vgg, "backbone.37") == ("patch", "patch")        # conv5_2: 20 x 20, 100 items at batch 32
    assert pair(vgg, "latent_layers.0") == ("igemm", "igemm")    # 3 x 3 at 10 x 10: below 400 pixels
    assert pair(vgg, "arm_loc.0") == ("head3x3", "head3x3")      # 40 x 40
    assert pair(vgg, "arm_loc.1") == ("head3x3", "head3x3")      # 20 x 20 = 400 pixels
    assert pair(vgg, "arm_loc.2") == ("igemm", "igemm")          # 10 x 10
    assert vgg["extras.0"] == ("igemm", "igemm", 4)              # a split-K layer
    assert all(v[:2] == ("igemm", "igemm") for v in vgg.values() if v[2] > 1)


def test_ws_threshold_at_a_smaller_frame():
    r = routes(_lib.DRN_VGGBN, 192, _lib.BF16)
    assert pair(r, "backbone.3") == ("patch", "ws")              # 72 units for one 192-px frame, 768 for 32


def test_mobilenet_pointwise_layers(mobile):
    assert pair(mobile, "backbone.7.3") == ("igemm", "pw1x1")    # 512 -> 512 at 40 x 40: 14 / 400 items
    assert pair(mobile, "backbone.3.3") == ("igemm", "igemm")    # 128 couts: no whole 256-group
    assert pair(mobile, "extras.0.0") == ("igemm", "igemm")      # 1024 -> 256 at 20 x 20: 50 items at batch 32
    assert pair(mobile, "trans_layers.0.0") == ("patch", "pp")
    assert pair(mobile, "arm_loc.1") == ("head3x3", "head3x3")
    assert mobile["extras.1.0"] == ("igemm", "igemm", 2)


@pytest.mark.parametrize("model", [_lib.DRN_VGGBN, _lib.DRN_MOBILENET])
def test_fp32_nets_know_igemm_and_patch_only(model):
    r = routes(model, 320, _lib.F32)
    assert {k for v in r.values() for k in v[:2]} <= {"igemm", "patch"}
    if model == _lib.DRN_VGGBN:
        assert pair(r, "backbone.3") == ("patch", "patch") and pair(r, "backbone.27") == ("patch", "patch")
        assert pair(r, "arm_loc.0") == ("igemm", "igemm")


def test_each_switch_moves_exactly_its_layers(vgg, mobile):
    r = routes(_lib.DRN_VGGBN, 320, _lib.BF16, _lib.PLAN_NO_CONV_PP)
    assert moved(vgg, r) == {k for k, v in vgg.items() if "pp" in v[:2]} and len(moved(vgg, r)) == 7
    assert all(pair(r, k) == ("patch", "patch") for k in moved(vgg, r))

    r = routes(_lib.DRN_VGGBN, 320, _lib.BF16, _lib.PLAN_NO_CONV_WS)
    assert moved(vgg, r) == {"backbone.3"} and pair(r, "backbone.3") == ("patch", "patch")

    r = routes(_lib.DRN_VGGBN, 320, _lib.BF16, _lib.PLAN_NO_CONV_PATCH)
    assert moved(vgg, r) == {k for k, v in vgg.items() if DIRECT & set(v[:2])}
    assert all(pair(r, k) == ("igemm", "igemm") for k in moved(vgg, r))

    r = routes(_lib.DRN_VGGBN, 320, _lib.BF16, _lib.PLAN_NO_HEAD3X3)
    assert moved(vgg, r) == {"arm_loc.0", "arm_loc.1"}
    assert all(pair(r, k) == ("igemm", "igemm") for k in moved(vgg, r))

    r = routes(_lib.DRN_MOBILENET, 320, _lib.BF16, _lib.PLAN_NO_PW1X1)
    assert moved(mobile, r) == {k for k, v in mobile.items() if "pw1x1" in v[:2]} and len(moved(mobile, r)) == 10
    assert all(pair(r, k) == ("igemm", "igemm") for k in moved(mobile, r))
