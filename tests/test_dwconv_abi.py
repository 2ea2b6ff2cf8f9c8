"""C ABI of the depthwise 3x3 conv with gradients (tdrn_hip.h section i-h), no GPU needed: the workspace query and the entries decide
every error before any launch, and the plan behind the query -- the weight gradient's split rule and its partial sums -- is restated
here in plain Python, independently of api.hip and dwconv_train.hip.
"""
import pytest
import torch

import test_gpu_dwconv as G
from tdrn_amd import _lib
from tdrn_amd.model import networks

# N C H W kH kW dH dW padH padW dilH dilW
GOOD = (2, 6, 9, 7, 3, 3, 2, 2, 1, 1, 1, 1)
NAMES = "N C H W kH kW dH dW padH padW dilH dilW".split()
FAMILY = ("tdrn_dwconv2d_workspace_bytes", "tdrn_dwconv2d_forward", "tdrn_dwconv2d_backward_input", "tdrn_dwconv2d_backward_parameters")
# backbone.1 .. backbone.13 and the two extras blocks: (channels, stride, input size at 320 px)
MOBILENET_320 = [(32, 1, 160), (64, 2, 160), (128, 1, 80), (128, 1, 80), (256, 1, 80), (256, 2, 80)] + [(512, 1, 40)] * 5 + \
                [(512, 2, 40), (1024, 1, 20), (256, 2, 20), (256, 2, 10)]


def cdiv(a, b):
    return -(-a // b)


def wgrad_splits(N, C, H, W, stride):
    """the split rule of tdrn_hip.h section i-h -> (S, per_split, K)"""
    K = N * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
    per = cdiv(K, max(1, min(cdiv(2048, C), cdiv(K, 1024))))
    return cdiv(K, per), per, K


def workspace_bytes(N, C, H, W, stride):
    """C S 10 floats, rounded up to 256 bytes"""
    return cdiv(C * wgrad_splits(N, C, H, W, stride)[0] * 10 * 4, 256) * 256


def _entries(lib, dims, dt, nb, p=256):
    """all three entries on fake non-null pointers.  Pointers are only compared with NULL before any launch, so this is called
    only where a check ahead of the first launch fails (bad geometry or a short workspace): a fake pointer never reaches a kernel."""
    q = lib.tdrn_dwconv2d_workspace_bytes(*dims, dt)
    assert q == 0 or nb < q
    return (lib.tdrn_dwconv2d_forward(p, p, None, p, *dims, dt, p, nb, None),
            lib.tdrn_dwconv2d_backward_input(p, p, p, *dims, dt, p, nb, None),
            lib.tdrn_dwconv2d_backward_parameters(p, p, p, None, *dims, 1.0, dt, p, nb, None))


def _with(**kw):
    d = dict(zip(NAMES, GOOD))
    d.update(kw)
    return tuple(d[n] for n in NAMES)


def test_symbols_exist():
    lib = _lib.lib()
    for name in FAMILY:
        assert name in _lib.EXPORTS and getattr(lib, name) is not None


def test_query_positive_and_equal_to_the_restated_plan():
    lib = _lib.lib()
    for case, (N, C, H, W, s) in G.CASES.items():
        assert lib.tdrn_dwconv2d_workspace_bytes(*G._dims(case), _lib.F32) == workspace_bytes(N, C, H, W, s) > 0, case
    # the MobileNet layers at 320 and 512 px, batch 32 and 8
    for px in (320, 512):
        for C, s, hw in MOBILENET_320:
            hw = hw * px // 320
            for N in (8, 32):
                dims = _with(N=N, C=C, H=hw, W=hw, dH=s, dW=s)
                assert lib.tdrn_dwconv2d_workspace_bytes(*dims, _lib.F32) == workspace_bytes(N, C, hw, hw, s) > 0, dims


def test_the_split_rule_fills_the_chip_and_collapses_on_tiny_maps():
    # C = 32 with K in the hundreds of thousands: 2048 workgroups of 3200 elements
    assert wgrad_splits(8, 32, 160, 160, 1) == (64, 3200, 204800)
    assert wgrad_splits(32, 32, 160, 160, 1) == (64, 12800, 819200)
    # the 1024-channel layer: one split per channel already fills it twice over
    assert wgrad_splits(8, 1024, 10, 10, 1) == (1, 800, 800)
    assert wgrad_splits(1, 1, 1, 1, 1) == (1, 1, 1) and wgrad_splits(2, 256, 6, 6, 2) == (1, 18, 18)
    # a ragged last split, and no empty one: cdiv(K, 3) = 726 elements, the third split holds 724
    assert wgrad_splits(8, 64, 33, 31, 2) == (3, 726, 2176)
    # S' ranges that would be empty are dropped: K = 1025 asks for 2 splits of 513
    assert wgrad_splits(1, 1, 25, 41, 1) == (2, 513, 1025)


@pytest.mark.parametrize("dims", [_with(N=0), _with(C=0), _with(H=-1), _with(W=0), _with(kH=0), _with(kW=-2), _with(dH=0), _with(dW=-1),
                                  _with(dilH=0), _with(dilW=-1), _with(padH=-1), _with(padW=-1),
                                  _with(H=2, W=2, padH=0, padW=0),          # an output smaller than 1 x 1
                                  _with(H=1, W=9, padH=0, padW=0)])
def test_bad_sizes_are_shape_errors(dims):
    lib = _lib.lib()
    for dt in (_lib.F32, _lib.BF16, _lib.F16, 3):       # ahead of the compute check
        assert lib.tdrn_dwconv2d_workspace_bytes(*dims, dt) == 0
        assert _entries(lib, dims, dt, 1 << 20) == (-2, -2, -2)


def test_compute_outside_the_enum_is_an_argument_error():
    lib = _lib.lib()
    for dt in (-1, 3):
        assert lib.tdrn_dwconv2d_workspace_bytes(*GOOD, dt) == 0
        assert _entries(lib, GOOD, dt, 1 << 20) == (-1, -1, -1)
        # ... ahead of an uncovered geometry
        assert _entries(lib, _with(kH=5, kW=5), dt, 1 << 20) == (-1, -1, -1)


UNCOVERED = [
    _with(kH=1, kW=1),                                   # k = 1
    _with(kH=5, kW=5),                                   # k = 5
    _with(dH=3, dW=3),                                   # stride 3
    _with(dH=2, dW=1), _with(dH=1, dW=2),                # per-axis stride
    _with(padH=0, padW=0),                               # pad 0
    _with(padH=2, padW=2),                               # pad 2
    _with(padH=1, padW=0), _with(padH=0, padW=1),        # per-axis pad
    _with(dilH=2, dilW=2),                               # dilation 2
    _with(kH=3, kW=1),                                   # not square
    _with(N=128, C=256, H=256, W=256),                   # N C H W = 2^31
    _with(N=1, C=2 ** 31 - 1, H=2, W=1),                 # ... in the last factor
    _with(N=2 ** 20, C=2 ** 20, H=2 ** 20, W=2 ** 20),   # a product far past 64 bits
]


@pytest.mark.parametrize("dims", UNCOVERED)
def test_uncovered_geometry_is_unsupported(dims):
    lib = _lib.lib()
    assert lib.tdrn_dwconv2d_workspace_bytes(*dims, _lib.F32) == 0
    assert _entries(lib, dims, _lib.F32, 1 << 20) == (-4, -4, -4)


def test_the_16_bit_types_are_unsupported():
    lib = _lib.lib()
    for stride in (1, 2):
        dims = _with(dH=stride, dW=stride)
        assert lib.tdrn_dwconv2d_workspace_bytes(*dims, _lib.F32) > 0
        for dt in (_lib.BF16, _lib.F16):
            assert lib.tdrn_dwconv2d_workspace_bytes(*dims, dt) == 0
            assert _entries(lib, dims, dt, 1 << 20) == (-4, -4, -4)


def test_the_size_limit_is_where_the_header_says():
    lib = _lib.lib()
    assert 128 * 256 * 256 * 256 == 2 ** 31
    # the largest covered element count, 2^31 - 1 (a prime: one factor holds all of it), in either position
    for dims in (_with(N=1, C=2 ** 31 - 1, H=1, W=1), _with(N=2 ** 31 - 1, C=1, H=1, W=1, dH=1, dW=1), _with(N=1, C=1, H=1, W=2 ** 31 - 1)):
        d = dict(zip(NAMES, dims))
        assert lib.tdrn_dwconv2d_workspace_bytes(*dims, _lib.F32) == workspace_bytes(d["N"], d["C"], d["H"], d["W"], d["dH"]) > 0, dims
    assert lib.tdrn_dwconv2d_workspace_bytes(*_with(N=127, C=256, H=256, W=256), _lib.F32) > 0


def test_short_workspace_and_null_pointers():
    lib = _lib.lib()
    p, dt = 256, _lib.F32
    nb = lib.tdrn_dwconv2d_workspace_bytes(*GOOD, dt)
    assert _entries(lib, GOOD, dt, nb - 1) == (-3, -3, -3)
    assert lib.tdrn_dwconv2d_forward(p, p, None, p, *GOOD, dt, None, nb, None) == -3            # no workspace at all
    assert lib.tdrn_dwconv2d_backward_input(p, p, p, *GOOD, dt, None, nb, None) == -3
    assert lib.tdrn_dwconv2d_backward_parameters(p, p, p, None, *GOOD, 1.0, dt, None, nb, None) == -3
    # a null tensor pointer is refused first, whatever else is passed: every call below has one
    assert lib.tdrn_dwconv2d_forward(None, p, None, p, *GOOD, dt, p, nb, None) == -1
    assert lib.tdrn_dwconv2d_forward(p, None, None, p, *GOOD, dt, p, nb, None) == -1
    assert lib.tdrn_dwconv2d_forward(p, p, None, None, *GOOD, dt, p, nb, None) == -1
    assert lib.tdrn_dwconv2d_backward_input(None, p, p, *GOOD, dt, p, nb, None) == -1
    assert lib.tdrn_dwconv2d_backward_input(p, None, p, *GOOD, dt, p, nb, None) == -1
    assert lib.tdrn_dwconv2d_backward_input(p, p, None, *GOOD, dt, p, nb, None) == -1
    assert lib.tdrn_dwconv2d_backward_parameters(None, p, p, None, *GOOD, 1.0, dt, p, nb, None) == -1
    assert lib.tdrn_dwconv2d_backward_parameters(p, None, p, None, *GOOD, 1.0, dt, p, nb, None) == -1
    assert lib.tdrn_dwconv2d_backward_parameters(p, p, None, None, *GOOD, 1.0, dt, p, nb, None) == -1
    # ... also in front of a bad geometry, an uncovered one and a short workspace
    assert lib.tdrn_dwconv2d_forward(None, p, None, p, *_with(N=0), dt, None, 0, None) == -1
    assert lib.tdrn_dwconv2d_backward_input(p, p, None, *_with(dH=3, dW=3), dt, None, 0, None) == -1
    assert lib.tdrn_dwconv2d_backward_parameters(p, p, None, None, *GOOD, 1.0, _lib.BF16, None, 0, None) == -1
    # a shape error comes before an uncovered geometry, that before the workspace
    assert lib.tdrn_dwconv2d_forward(p, p, None, p, *_with(N=0, dH=3, dW=3), dt, None, 0, None) == -2
    assert lib.tdrn_dwconv2d_forward(p, p, None, p, *_with(dH=3, dW=3), dt, None, 0, None) == -4
    assert lib.tdrn_dwconv2d_forward(p, p, None, p, *GOOD, _lib.BF16, None, 0, None) == -4


def test_module_has_nn_conv2d_parameters():
    for stride, bias in ((1, False), (2, True)):
        m, r = networks.DepthwiseConv2d(5, stride=stride, bias=bias), torch.nn.Conv2d(5, 5, 3, stride, 1, groups=5, bias=bias)
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in r.state_dict().items()}
        assert m.stride == (stride, stride) and tuple(m.weight.shape) == (5, 1, 3, 3)
        m.load_state_dict(r.state_dict())
        torch.manual_seed(3)
        r.reset_parameters()
        torch.manual_seed(3)
        m.reset_parameters()
        assert torch.equal(m.weight, r.weight) and (not bias or torch.equal(m.bias, r.bias))
    assert networks.DepthwiseConv2d(5).bias is None and networks.DepthwiseConv2d(5).stride == (1, 1)


def test_cpu_tensors_are_rejected():
    x, w, b = torch.zeros(1, 4, 8, 8), torch.zeros(4, 1, 3, 3), torch.zeros(4)
    with pytest.raises(NotImplementedError):
        networks.depthwise_conv2d(x, w, b)
    with pytest.raises(NotImplementedError):
        networks.DepthwiseConv2dFunction.apply(x, w, None, 2, 1)
    with pytest.raises(NotImplementedError):
        networks.DepthwiseConv2d(4, stride=2)(x)
    with pytest.raises(ValueError):
        networks.depthwise_conv2d(x[0], w, b)


def test_the_walk_sends_only_the_depthwise_3x3_to_the_op():
    from tdrn_amd.model._base import _flatten, _is_depthwise3x3
    from tdrn_amd.model.dualrefinedet_mobilenet import build_net
    net = build_net("train", 320, 21, 1, False)
    convs = [m for m in _flatten(list(net.backbone) + list(net.extras)) if isinstance(m, torch.nn.Conv2d)]
    assert sum(_is_depthwise3x3(m) for m in convs) == 15 and sum(m.groups == 1 for m in convs) == 1 + 15 + 2
    assert [(m.in_channels, m.stride[0]) for m in convs if _is_depthwise3x3(m)] == [(c, s) for c, s, _ in MOBILENET_320]
    for m in (torch.nn.Conv2d(8, 8, 3, 1, 1, groups=4), torch.nn.Conv2d(8, 16, 3, 1, 1, groups=8), torch.nn.Conv2d(8, 8, 5, 1, 2, groups=8),
              torch.nn.Conv2d(8, 8, 3, 1, 0, groups=8), torch.nn.Conv2d(8, 8, 3, 1, 2, 2, groups=8)):
        assert not _is_depthwise3x3(m)
        with pytest.raises(NotImplementedError, match="no differentiable op"):
            net._walk([m], torch.zeros(1, 8, 8, 8), "fp32")
