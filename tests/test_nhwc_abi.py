"""C ABI of the resident-tensor entries (tdrn_hip.h section i-k), no GPU needed: every entry decides every error before its first
launch, the BatchNorm split rule is the table of DESIGN.md section 22, and tdrn_conv2d_nhwc_route names the kernel each stride-1 3x3
layer of the 320-px VGG-BN trunk reaches.

The expected kernels are worked out by hand from patch_takes / pp_takes / conv3x3_tile_mode (the way tests/test_conv_route.py
documents its pairs).  Nothing is pooled on the training path, the result is 16-bit and gap-free, so every 3x3 / pad 1 / dilation 1
layer of >= 400 pixels is a direct-conv layer:
  * tiles: 320 and 160 px maps are 2-D (W % 32 == 0), 80 px maps 2-D (16 x 16), 40 and 20 px maps flat (256 consecutive pixels).
  * conv3x3_pp needs Cin >= 256 of the LAUNCH (the input gradient convolves grad_output: its Cin is the layer's Cout), Npad % 256 == 0
    (Npad pads the launch's Cout: the layer's Cin in the input gradient) and >= 192 items of 256 pixels x 256 couts:
      conv3_2 / conv3_3 (256 -> 256, 80 x 80): 25 tiles a frame, one cout tile: 200 items at batch 8, 800 at 32 -> pp / pp, both ways.
      conv4_1 (256 -> 512, 40 x 40): forward ceil(1600 B / 256) * 2 = 100 / 400 items -> patch / pp; the input gradient has 256 couts:
        50 / 200 items -> patch / pp.
      conv4_2 / conv4_3 (512 -> 512): 100 / 400 items -> patch / pp, both ways.
      conv5_x (512 -> 512, 20 x 20): ceil(400 B / 256) * 2 = 26 / 100 items -> patch / patch.
      conv3_1 (128 -> 256): forward Cin = 128 -> patch; its input gradient has Cin = 256 but 128 couts (Npad 128) -> patch.
      conv1_2, conv2_1, conv2_2: Cin (and the input gradient's Cin) <= 128 -> patch.
  * fc6 (dilation 6, on the 10 x 10 map behind pool5) is no such layer: igemm; fc7 (1x1, 10 x 10) has 16 / 52 items of the wide 1x1
    GEMM, below its 192: igemm.
"""
import ctypes as C
import os
import re

import pytest

from tdrn_amd import _lib

P = 256                     # a fake non-null pointer on a 16-byte boundary: only compared with NULL (and its low bits) before any launch
BF16, F16, F32 = _lib.BF16, _lib.F16, _lib.F32
CONV = (2, 64, 9, 7, 128, 3, 3, 1, 1, 1, 1, 1, 1)       # N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilH, dilW
BN = (2, 64, 5, 7)
ARG, SHAPE, WORKSPACE, UNSUPPORTED = -1, -2, -3, -4


def conv_fwd(lib, dims=CONV, dt=BF16, nb=1 << 30, ptrs=None, ws=P, flags=0):
    ptrs = [P] * 4 if ptrs is None else ptrs
    return lib.tdrn_conv2d_nhwc_forward(*ptrs, *dims, dt, ws, nb, None, flags)


def conv_dgrad(lib, dims=CONV, dt=BF16, nb=1 << 30, ptrs=None, ws=P, flags=0):
    ptrs = [P] * 3 if ptrs is None else ptrs
    return lib.tdrn_conv2d_nhwc_backward_input(*ptrs, *dims, dt, ws, nb, None, flags)


def conv_wgrad(lib, dims=CONV, dt=BF16, nb=1 << 30, ptrs=None, ws=P, flags=0):
    ptrs = [P] * 4 if ptrs is None else ptrs
    return lib.tdrn_conv2d_nhwc_backward_parameters(*ptrs, *dims, 1.0, dt, ws, nb, None, flags)


CONV_ENTRIES = (conv_fwd, conv_dgrad, conv_wgrad)


def bn_fwd(lib, dims=BN, dt=BF16, nb=1 << 30, training=1, momentum=0.1, eps=1e-5, ptrs=None, ws=P):
    ptrs = [P] * 8 if ptrs is None else ptrs
    return lib.tdrn_batch_norm_nhwc_forward(*ptrs, *dims, training, momentum, eps, 1, dt, ws, nb, None)


def bn_bwd(lib, dims=BN, dt=BF16, nb=1 << 30, training=1, ptrs=None, ws=P):
    ptrs = [P] * 9 if ptrs is None else ptrs
    return lib.tdrn_batch_norm_nhwc_backward(*ptrs, *dims, training, 1, 1.0, dt, ws, nb, None)


def pool_fwd(lib, dims=BN, geo=(2, 2, 0, 0), dt=BF16, ptrs=None):
    ptrs = [P] * 3 if ptrs is None else ptrs
    return lib.tdrn_max_pool_nhwc_forward(*ptrs, *dims, *geo, dt, None)


def pool_bwd(lib, dims=BN, geo=(2, 2, 0, 0), dt=BF16, ptrs=None):
    ptrs = [P] * 3 if ptrs is None else ptrs
    return lib.tdrn_max_pool_nhwc_backward(*ptrs, *dims, *geo, dt, None)


def with_dim(dims, i, v):
    d = list(dims)
    d[i] = v
    return tuple(d)


def test_conv_queries_and_short_workspace():
    lib = _lib.lib()
    for dt in (BF16, F16):
        for flags in (0, _lib.CONV_NHWC_IGEMM_ONLY):
            nb = lib.tdrn_conv2d_nhwc_workspace_bytes(*CONV, dt, flags)
            assert nb > 0
            for entry in CONV_ENTRIES:
                assert entry(lib, dt=dt, nb=nb - 1, flags=flags) == WORKSPACE       # one byte short
                assert entry(lib, dt=dt, nb=nb, ws=None, flags=flags) == WORKSPACE
    # the resident workspace holds no copy of an activation: smaller than the fp32 NCHW entry's
    big = (8, 256, 80, 80, 256, 3, 3, 1, 1, 1, 1, 1, 1)
    assert 0 < lib.tdrn_conv2d_nhwc_workspace_bytes(*big, BF16, 0) < lib.tdrn_conv2d_workspace_bytes(*big, BF16)


def test_conv_channel_blocks_type_and_family():
    lib = _lib.lib()
    cases = [(with_dim(CONV, 1, 3), BF16, UNSUPPORTED),                     # Cin % 64
             (with_dim(CONV, 1, 96), BF16, UNSUPPORTED),
             (with_dim(CONV, 4, 100), F16, UNSUPPORTED),                    # Cout % 64
             (CONV, F32, ARG),                                              # TDRN_F32 is a bad dtype here
             (CONV, 3, ARG),
             (CONV[:7] + (2, 2) + CONV[9:], BF16, UNSUPPORTED),             # stride 2
             (CONV[:5] + (5, 5, 1, 1, 2, 2, 1, 1), BF16, UNSUPPORTED),      # k = 5
             (CONV[:9] + (3, 3, 1, 1), BF16, UNSUPPORTED),                  # pad > dil (k - 1)
             (CONV[:9] + (1, 2, 1, 1), BF16, UNSUPPORTED),                  # two pads
             (with_dim(CONV, 0, 0), BF16, SHAPE),
             (with_dim(CONV, 2, -1), BF16, SHAPE),
             ((1, 64, 2, 2, 64, 3, 3, 1, 1, 0, 0, 1, 1), BF16, SHAPE),      # the window does not fit
             ((1 << 10, 64, 1 << 8, 1 << 7, 64, 1, 1, 1, 1, 0, 0, 1, 1), BF16, UNSUPPORTED)]        # 2^31 elements
    for dims, dt, want in cases:
        assert lib.tdrn_conv2d_nhwc_workspace_bytes(*dims, dt, 0) == 0, dims
        assert lib.tdrn_conv2d_nhwc_route(*dims, dt, 0, 0) is None, dims
        for entry in CONV_ENTRIES:
            assert entry(lib, dims=dims, dt=dt) == want, (entry.__name__, dims, dt)
    for entry in CONV_ENTRIES:
        assert entry(lib, flags=2) == ARG                                   # an unknown flag bit
    assert lib.tdrn_conv2d_nhwc_workspace_bytes(*CONV, BF16, 2) == 0


def test_conv_splits_query():
    lib = _lib.lib()
    f, d, w = C.c_int(), C.c_int(), C.c_int()
    ptrs = (C.byref(f), C.byref(d), C.byref(w))
    assert lib.tdrn_conv2d_nhwc_splits(*CONV, BF16, 0, *ptrs) == 0 and (f.value, d.value, w.value) == (2, 4, 1)
    # conv3_2 at batch 8: a direct-conv layer is never split; its weight gradient has min(ceil(512 / 16 tiles), ceil(51200 / 256)) = 32 splits
    big = (8, 256, 80, 80, 256, 3, 3, 1, 1, 1, 1, 1, 1)
    for flags in (0, _lib.CONV_NHWC_IGEMM_ONLY):            # the flag changes no split
        assert lib.tdrn_conv2d_nhwc_splits(*big, BF16, flags, *ptrs) == 0 and (f.value, d.value, w.value) == (1, 1, 32)
    assert lib.tdrn_conv2d_nhwc_splits(*CONV, BF16, 0, None, C.byref(d), C.byref(w)) == ARG
    assert lib.tdrn_conv2d_nhwc_splits(*CONV, F32, 0, *ptrs) == ARG
    assert lib.tdrn_conv2d_nhwc_splits(*with_dim(CONV, 1, 96), BF16, 0, *ptrs) == UNSUPPORTED


def test_conv_pointers():
    lib = _lib.lib()
    # forward: input, weight, bias (optional), output
    for i, bad in ((0, None), (1, None), (3, None), (0, P + 2), (3, P + 2), (0, P + 8), (1, P + 2), (2, P + 2)):
        ptrs = [P] * 4
        ptrs[i] = bad
        assert conv_fwd(lib, ptrs=ptrs) == ARG, (i, bad)
    assert conv_fwd(lib, ptrs=[P, P, None, P], nb=0) == WORKSPACE           # no bias is legal
    assert conv_fwd(lib, ptrs=[P, P + 4, P + 4, P], nb=0) == WORKSPACE      # fp32 tensors on any 4-byte boundary
    # backward_input: grad_output, weight, grad_input
    for i, bad in ((0, None), (1, None), (2, None), (0, P + 2), (2, P + 2), (1, P + 1)):
        ptrs = [P] * 3
        ptrs[i] = bad
        assert conv_dgrad(lib, ptrs=ptrs) == ARG, (i, bad)
    # backward_parameters: input, grad_output, grad_weight, grad_bias (optional)
    for i, bad in ((0, None), (1, None), (2, None), (0, P + 2), (1, P + 2), (2, P + 2), (3, P + 2)):
        ptrs = [P] * 4
        ptrs[i] = bad
        assert conv_wgrad(lib, ptrs=ptrs) == ARG, (i, bad)
    assert conv_wgrad(lib, ptrs=[P, P, P, None], nb=0) == WORKSPACE


def test_layout_entries():
    lib = _lib.lib()
    for fn, act in ((lib.tdrn_nhwc16_from_nchw, 1), (lib.tdrn_nchw_from_nhwc16, 0)):
        for ptrs in ([None, P], [P, None]):
            assert fn(*ptrs, *BN, BF16, None) == ARG
        ptrs = [P, P]
        ptrs[act] = P + 2
        assert fn(*ptrs, *BN, BF16, None) == ARG                            # the resident side off a 16-byte boundary
        ptrs[act] = P + 4
        assert fn(*ptrs, *BN, F16, None) == ARG
        ptrs = [P, P]
        ptrs[1 - act] = P + 2
        assert fn(*ptrs, *BN, BF16, None) == ARG                            # the fp32 side off a 4-byte boundary
        assert fn(P, P, *BN, F32, None) == ARG
        assert fn(P, P, *with_dim(BN, 1, 70), BF16, None) == UNSUPPORTED
        assert fn(P, P, *with_dim(BN, 2, 0), BF16, None) == SHAPE
        assert fn(P, P, 1 << 10, 64, 1 << 8, 1 << 7, BF16, None) == UNSUPPORTED


def test_batch_norm_errors():
    lib = _lib.lib()
    nb = lib.tdrn_batch_norm_nhwc_workspace_bytes(*BN)
    assert nb > 0
    for training in (0, 1):
        assert bn_fwd(lib, nb=nb - 1, training=training) == WORKSPACE and bn_bwd(lib, nb=nb - 1, training=training) == WORKSPACE
        assert bn_fwd(lib, nb=nb, ws=None, training=training) == WORKSPACE and bn_bwd(lib, nb=nb, ws=None, training=training) == WORKSPACE
    for dims, want in ((with_dim(BN, 1, 70), UNSUPPORTED), (with_dim(BN, 1, 32), UNSUPPORTED), (with_dim(BN, 0, 0), SHAPE),
                       (with_dim(BN, 3, -2), SHAPE), ((1 << 10, 64, 1 << 8, 1 << 7), UNSUPPORTED)):
        assert lib.tdrn_batch_norm_nhwc_workspace_bytes(*dims) == 0
        assert bn_fwd(lib, dims=dims) == want and bn_bwd(lib, dims=dims) == want, dims
    assert bn_fwd(lib, dt=F32) == ARG and bn_bwd(lib, dt=F32) == ARG
    # one value per channel: refused in training only
    one = (1, 64, 1, 1)
    assert bn_fwd(lib, dims=one) == SHAPE and bn_bwd(lib, dims=one) == SHAPE
    assert bn_fwd(lib, dims=one, training=0, nb=0) == WORKSPACE and bn_bwd(lib, dims=one, training=0, nb=0) == WORKSPACE
    assert bn_fwd(lib, eps=0.0, nb=0) == ARG and bn_fwd(lib, momentum=1.5, nb=0) == ARG
    # forward: input, weight, bias, running_mean, running_var, output, save_mean, save_invstd
    for i in (0, 1, 2, 5, 6, 7):
        ptrs = [P] * 8
        ptrs[i] = None
        assert bn_fwd(lib, ptrs=ptrs) == ARG, i
    assert bn_fwd(lib, ptrs=[P, P, P, None, P, P, P, P]) == ARG
    assert bn_fwd(lib, training=0, ptrs=[P, P, P, None, None, P, P, P]) == ARG
    assert bn_fwd(lib, nb=0, ptrs=[P, P, P, None, None, P, P, P]) == WORKSPACE
    assert bn_fwd(lib, ptrs=[P + 2] + [P] * 7) == ARG and bn_fwd(lib, ptrs=[P] * 5 + [P + 2, P, P]) == ARG
    assert bn_fwd(lib, ptrs=[P + 4] + [P] * 7) == ARG                       # a 4-byte boundary is not enough for an activation
    assert bn_fwd(lib, ptrs=[P, P + 2] + [P] * 6) == ARG
    assert bn_fwd(lib, nb=0, ptrs=[P, P + 4, P + 4, P + 4, P + 4, P, P + 4, P + 4]) == WORKSPACE
    # backward: input, grad_output, weight, bias, save_mean, save_invstd, grad_input, grad_weight, grad_bias
    for i in range(6):
        ptrs = [P] * 9
        ptrs[i] = None
        assert bn_bwd(lib, ptrs=ptrs) == ARG, i
    assert bn_bwd(lib, ptrs=[P] * 7 + [P, None]) == ARG and bn_bwd(lib, ptrs=[P] * 6 + [None, None, None]) == ARG
    assert bn_bwd(lib, nb=0, ptrs=[P] * 6 + [None, P, P]) == WORKSPACE and bn_bwd(lib, nb=0, ptrs=[P] * 6 + [P, None, None]) == WORKSPACE
    for i in (0, 1, 6):
        ptrs = [P] * 9
        ptrs[i] = P + 2
        assert bn_bwd(lib, ptrs=ptrs) == ARG, i


def test_max_pool_errors():
    lib = _lib.lib()
    for fn in (pool_fwd, pool_bwd):
        assert fn(lib, dims=with_dim(BN, 1, 70)) == UNSUPPORTED
        assert fn(lib, dims=with_dim(BN, 1, 8)) == UNSUPPORTED
        assert fn(lib, dt=F32) == ARG
        assert fn(lib, geo=(3, 2, 1, 0)) == UNSUPPORTED and fn(lib, geo=(2, 2, 1, 0)) == UNSUPPORTED
        assert fn(lib, dims=with_dim(BN, 0, 0)) == SHAPE
        assert fn(lib, dims=(1, 64, 1, 1), geo=(2, 2, 0, 0)) == SHAPE        # nothing fits
        assert fn(lib, ptrs=[None, P, P]) == ARG and fn(lib, ptrs=[P, P, None] if fn is pool_bwd else [P, None, P]) == ARG
        assert fn(lib, ptrs=[P + 2, P, P]) == ARG
    assert pool_fwd(lib, ptrs=[P, P + 2, P]) == ARG and pool_bwd(lib, ptrs=[P, P, P + 2]) == ARG
    assert pool_bwd(lib, ptrs=[P, None, P]) == ARG                          # the backward needs its codes


def nhwc_splits(lib, dims):
    s, per = C.c_int(), C.c_int()
    assert lib.tdrn_batch_norm_nhwc_splits(*dims, C.byref(s), C.byref(per)) == 0
    return s.value, per.value


def test_batch_norm_split_rule_is_the_design_table():
    """DESIGN.md section 22 lists `| nhwc ... | (N, C, H, W) | M | per_split | splits |` rows: they are the library's, and the rule is
    S = clamp(floor(2048 / (C / 64)), 1, ceil(M / 256)), per_split = ceil(M / S) rounded up to 32, splits = ceil(M / per_split)"""
    lib = _lib.lib()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    rows = re.findall(r"^\| nhwc ([\w ]+?) \| \((\d+), (\d+), (\d+), (\d+)\) \| (\d+) \| (\d+) \| (\d+) \|", text, re.M)
    seen = set()
    for name, N, Cc, H, W, M, per, splits in rows:
        N, Cc, H, W, M, per, splits = (int(v) for v in (N, Cc, H, W, M, per, splits))
        assert M == N * H * W, name
        assert nhwc_splits(lib, (N, Cc, H, W)) == (splits, per), name
        assert lib.tdrn_batch_norm_nhwc_workspace_bytes(N, Cc, H, W) == 12 * Cc * splits + 8 * Cc, name
        S = max(1, min(2048 // (Cc // 64), -(-M // 256)))
        want_per = -(-(-(-M // S)) // 32) * 32
        assert (per, splits) == (want_per, -(-M // want_per)), name
        assert per % 32 == 0 and (splits - 1) * per < M <= splits * per, name
        seen.add((N, Cc, H, W))
    trunk = {(b, c, s, s) for b in (8, 32) for c, s in ((64, 320), (128, 160), (256, 80), (512, 40), (512, 20), (1024, 10))}
    tests = {(1, 64, 1, 2), (1, 64, 31, 1), (1, 64, 32, 1), (1, 64, 33, 1), (2, 192, 5, 5), (1, 128, 80, 80), (3, 1024, 10, 10), (1, 64, 1, 1),
             (1, 64, 16, 16), (1, 64, 1, 257)}
    assert trunk | tests <= seen, (trunk | tests) - seen
    assert nhwc_splits(lib, (1, 64, 16, 16))[0] == 1 and nhwc_splits(lib, (1, 64, 1, 257))[0] == 2          # the first shape with two splits


VGG_3X3 = [  # layer, Cin, Cout, map; (forward, input gradient) at batch 8 and at batch 32
    ("conv1_2", 64, 64, 320, ("patch", "patch"), ("patch", "patch")),
    ("conv2_1", 64, 128, 160, ("patch", "patch"), ("patch", "patch")),
    ("conv2_2", 128, 128, 160, ("patch", "patch"), ("patch", "patch")),
    ("conv3_1", 128, 256, 80, ("patch", "patch"), ("patch", "patch")),
    ("conv3_2", 256, 256, 80, ("pp", "pp"), ("pp", "pp")),
    ("conv3_3", 256, 256, 80, ("pp", "pp"), ("pp", "pp")),
    ("conv4_1", 256, 512, 40, ("patch", "patch"), ("pp", "pp")),
    ("conv4_2", 512, 512, 40, ("patch", "patch"), ("pp", "pp")),
    ("conv4_3", 512, 512, 40, ("patch", "patch"), ("pp", "pp")),
    ("conv5_1", 512, 512, 20, ("patch", "patch"), ("patch", "patch")),
    ("conv5_2", 512, 512, 20, ("patch", "patch"), ("patch", "patch")),
    ("conv5_3", 512, 512, 20, ("patch", "patch"), ("patch", "patch")),
]


def route(lib, B, cin, cout, size, flags, dgrad, k=3, pad=1, dil=1):
    r = lib.tdrn_conv2d_nhwc_route(B, cin, size, size, cout, k, k, 1, 1, pad, pad, dil, dil, BF16, flags, dgrad)
    assert r is not None
    return r.decode()


@pytest.mark.parametrize("layer", VGG_3X3, ids=[l[0] for l in VGG_3X3])
def test_route_of_the_vgg_trunk(layer):
    lib = _lib.lib()
    name, cin, cout, size, at8, at32 = layer
    for B, want in ((8, at8), (32, at32)):
        got = (route(lib, B, cin, cout, size, 0, 0), route(lib, B, cin, cout, size, 0, 1))
        assert got == want, (name, B, got, want)
        assert size * size < 400 or "igemm" not in got, name            # no pad-1, dil-1 layer of >= 400 pixels is on igemm
        only = (route(lib, B, cin, cout, size, _lib.CONV_NHWC_IGEMM_ONLY, 0), route(lib, B, cin, cout, size, _lib.CONV_NHWC_IGEMM_ONLY, 1))
        assert only == ("igemm", "igemm"), (name, B, only)


def test_route_outside_the_direct_conv_layers():
    lib = _lib.lib()
    for B in (8, 32):
        assert route(lib, B, 512, 1024, 10, 0, 0, pad=6, dil=6) == "igemm" and route(lib, B, 512, 1024, 10, 0, 1, pad=6, dil=6) == "igemm"   # fc6
        assert route(lib, B, 1024, 1024, 10, 0, 0, k=1, pad=0) == "igemm"   # fc7 on its 10 x 10 map: 16 / 52 items of the wide 1x1 GEMM
        assert route(lib, B, 512, 512, 10, 0, 0) == "igemm"                 # 100 pixels: below the direct-conv kernels' 400
        for dgrad in (0, 1):
            assert route(lib, B, 1024, 1024, 20, _lib.CONV_NHWC_IGEMM_ONLY, dgrad, k=1, pad=0) == "igemm"   # a wide 1x1 layer with the switch
    assert route(lib, 8, 1024, 1024, 20, 0, 0, k=1, pad=0) == "igemm"       # a 1024 -> 1024 1x1 layer on 20 x 20: 13 x 4 = 52 items at batch 8 ...
    assert route(lib, 32, 1024, 1024, 20, 0, 0, k=1, pad=0) == "pw1x1"      # ... 200 at batch 32: the wide 1x1 GEMM
