"""C ABI and Python refusals of the transform-domain deformable conv (tdrn_hip.h section i-l), no GPU needed: both queries answer
inside the scope and return 0 outside it, every entry decides every refusal before its first launch, and the Python op and
forward_train(deform_algo=...) raise what they promise."""
import pytest
import torch

from tdrn_amd import _lib
from tdrn_amd.model import networks

P = 256                     # a fake non-null pointer on a 256-byte boundary: only compared with NULL (and its low bits) before any launch
BF16, F16, F32 = _lib.BF16, _lib.F16, _lib.F32
ARG, SHAPE, WORKSPACE, UNSUPPORTED = -1, -2, -3, -4
# N, Cin, H, W, Cout, kW, kH, dW, dH, padW, padH, dilationH, dilationW, G: the argument order of tdrn_deform_conv_forward
DIMS = (2, 64, 6, 5, 75, 3, 3, 1, 1, 1, 1, 1, 1, 1)
BIG = 1 << 30


def with_dim(dims, i, v):
    d = list(dims)
    d[i] = v
    return tuple(d)


def fwd(lib, dims=DIMS, dt=BF16, nb=BIG, ptrs=None, ws=P):
    ptrs = [P] * 5 if ptrs is None else ptrs            # input, weight, offset, output, y_save
    return lib.tdrn_deform_conv_ts_forward(*ptrs, *dims, dt, ws, nb, None)


def bwd(lib, dims=DIMS, dt=BF16, nb=BIG, ptrs=None, ws=P):
    ptrs = [P] * 8 if ptrs is None else ptrs            # input, weight, offset, grad_output, y_saved, grad_input, grad_offset, grad_weight
    return lib.tdrn_deform_conv_ts_backward(*ptrs, *dims, dt, ws, nb, None)


def test_queries_inside_the_scope():
    lib = _lib.lib()
    for dt, es in ((BF16, 2), (F16, 2)):
        assert lib.tdrn_deform_conv_ts_workspace_bytes(*DIMS, dt) > 0
        # Y: N H W pixels of kH kW ceil8(Cout) = 720 columns, padded to 768
        assert lib.tdrn_deform_conv_ts_y_bytes(*DIMS, dt) == 2 * 6 * 5 * 768 * es
    # a 1 x 1 map under a 3 x 3 kernel with pad 1, a 5 x 5 kernel, stride 2 (Y lives on input pixels), Cout at both ends of the scope
    for dims in ((1, 64, 1, 1, 12, 3, 3, 1, 1, 1, 1, 1, 1, 1), (2, 256, 6, 5, 12, 5, 5, 1, 1, 2, 2, 1, 1, 1),
                 (1, 128, 9, 8, 63, 3, 3, 2, 2, 1, 1, 1, 1, 1), with_dim(DIMS, 4, 1), with_dim(DIMS, 4, 256)):
        assert lib.tdrn_deform_conv_ts_workspace_bytes(*dims, BF16) > 0, dims
        assert lib.tdrn_deform_conv_ts_y_bytes(*dims, BF16) > 0, dims
    assert lib.tdrn_deform_conv_ts_y_bytes(2, 256, 6, 5, 12, 5, 5, 1, 1, 2, 2, 1, 1, 1, F16) == 2 * 6 * 5 * 448 * 2       # 25 * 16 = 400 -> 448


def test_refusals_launch_nothing():
    """the pointers are fake and the stream is the null stream: a launch would fault, a refusal returns its code"""
    lib = _lib.lib()
    cases = [(with_dim(DIMS, 13, 2), BF16, UNSUPPORTED),                    # G = 2
             (with_dim(with_dim(DIMS, 13, 8), 1, 512), F16, UNSUPPORTED),   # G = 8 (the SSD4Scale heads)
             (with_dim(DIMS, 1, 96), BF16, UNSUPPORTED),                    # Cin = 96
             (DIMS, F32, UNSUPPORTED),                                      # TDRN_F32
             (DIMS, 3, ARG),                                                # no tdrn_dtype
             (with_dim(DIMS, 4, 257), BF16, UNSUPPORTED),                   # Cout = 257
             (with_dim(DIMS, 4, 0), BF16, SHAPE),
             (with_dim(DIMS, 0, 0), BF16, SHAPE),
             (with_dim(DIMS, 2, -1), BF16, SHAPE),
             (with_dim(DIMS, 7, 0), BF16, SHAPE),                           # stride 0
             (with_dim(DIMS, 13, 0), BF16, SHAPE),
             ((1, 64, 2, 2, 12, 5, 5, 1, 1, 0, 0, 1, 1, 1), BF16, SHAPE),   # the window does not fit
             # Z (and Y) of 2^24 pixels x 192 columns = 3 * 2^30 elements, beside an input of 2^30
             ((1 << 9, 64, 1 << 8, 1 << 7, 12, 3, 3, 1, 1, 1, 1, 1, 1, 1), BF16, UNSUPPORTED),
             ((1 << 10, 64, 1 << 8, 1 << 7, 12, 3, 3, 1, 1, 1, 1, 1, 1, 1), BF16, UNSUPPORTED)]       # the input itself: 2^31 elements
    for dims, dt, want in cases:
        assert lib.tdrn_deform_conv_ts_workspace_bytes(*dims, dt) == 0, dims
        assert lib.tdrn_deform_conv_ts_y_bytes(*dims, dt) == 0, dims
        assert fwd(lib, dims=dims, dt=dt) == want, (dims, dt)
        assert bwd(lib, dims=dims, dt=dt) == want, (dims, dt)


def test_workspace_and_pointers():
    lib = _lib.lib()
    for dt in (BF16, F16):
        nb = lib.tdrn_deform_conv_ts_workspace_bytes(*DIMS, dt)
        for entry in (fwd, bwd):
            assert entry(lib, dt=dt, nb=nb - 1) == WORKSPACE                # one byte short
            assert entry(lib, dt=dt, nb=nb, ws=None) == WORKSPACE
    # forward: input, weight, offset, output are required, y_save is not; fp32 on 4 bytes, Y on 16
    for i in range(4):
        ptrs = [P] * 5
        ptrs[i] = None
        assert fwd(lib, ptrs=ptrs) == ARG, i
        ptrs[i] = P + 2
        assert fwd(lib, ptrs=ptrs) == ARG, i
    assert fwd(lib, ptrs=[P, P, P, P, None], nb=0) == WORKSPACE
    assert fwd(lib, ptrs=[P + 4, P + 4, P + 4, P + 4, P + 16], nb=0) == WORKSPACE
    assert fwd(lib, ptrs=[P, P, P, P, P + 8]) == ARG
    # backward: input, weight, offset, grad_output are required; y_saved and each gradient may be null, but not all three gradients
    for i in range(4):
        ptrs = [P] * 8
        ptrs[i] = None
        assert bwd(lib, ptrs=ptrs) == ARG, i
    for i in (0, 1, 2, 3, 5, 6, 7):
        ptrs = [P] * 8
        ptrs[i] = P + 2
        assert bwd(lib, ptrs=ptrs) == ARG, i
    assert bwd(lib, ptrs=[P, P, P, P, P + 8, P, P, P]) == ARG
    assert bwd(lib, ptrs=[P, P, P, P, None, None, None, None]) == ARG
    for grads in ((P, None, None), (None, P, None), (None, None, P), (P, P, None), (None, P, P), (P, None, P)):
        assert bwd(lib, ptrs=[P, P, P, P, None] + list(grads), nb=0) == WORKSPACE, grads
    # a refusal of the geometry wins over a short workspace, a bad pointer over both
    assert fwd(lib, dims=with_dim(DIMS, 1, 96), nb=0) == UNSUPPORTED
    assert fwd(lib, dims=with_dim(DIMS, 1, 96), ptrs=[None, P, P, P, P], nb=0) == ARG


def _cpu_inputs(cin=64, cout=12, k=3, h=4, w=5):
    x = torch.zeros(1, cin, h, w)
    off = torch.zeros(1, 2 * k * k, h, w)
    wt = torch.zeros(cout, cin, k, k)
    return x, off, wt


def test_python_refusals():
    x, off, w = _cpu_inputs()
    with pytest.raises(NotImplementedError):                # CPU tensors
        networks.conv_offset2d_ts(x, off, w, 1, 1, 1, "bf16")
    with pytest.raises(NotImplementedError):
        networks.ConvOffset2dTsFunction.apply(x.requires_grad_(True), off, w, 1, 1, 1, "fp16")
    x = x.detach()
    with pytest.raises(ValueError):
        networks.conv_offset2d_ts(x, off, w, 1, 1, 1, "fp32")
    with pytest.raises(ValueError):
        networks.conv_offset2d_ts(x[0], off, w, 1, 1, 1, "bf16")
    # geometry the library refuses: RuntimeError that names what is covered, no fall-back to the gather op
    for bad in (_cpu_inputs(cin=96), _cpu_inputs(cout=257)):
        with pytest.raises(RuntimeError, match="covers one deformable group"):
            networks.conv_offset2d_ts(*bad, 1, 1, 1, "bf16")
    with pytest.raises(RuntimeError, match="invalid shape of offset"):          # G = 2 offsets: this op has one group
        networks.conv_offset2d_ts(x, torch.zeros(1, 36, 4, 5), w, 1, 1, 1, "bf16")


def _vggbn(**kw):
    from tdrn_amd.model.dualrefinedet_vggbn import build_net
    return build_net("train", 320, 3, **kw)


def test_forward_train_checks_before_the_engine_is_marked_stale():
    net = _vggbn()
    x = torch.zeros(1, 3, 320, 320)
    for dirty in (False, True):
        object.__setattr__(net, "_dirty", dirty)
        with pytest.raises(ValueError, match="transform"):
            net.forward_train(x, "fp32", False, "transform")
        with pytest.raises(ValueError, match="transform"):
            net.forward_train(x, deform_algo="transform")                       # compute defaults to fp32
        with pytest.raises(ValueError, match="nonsense"):
            net.forward_train(x, "bf16", deform_algo="nonsense")
        assert net._dirty is dirty
    g2 = _vggbn(def_groups=2)
    object.__setattr__(g2, "_dirty", False)
    with pytest.raises(NotImplementedError, match="def_groups"):
        g2.forward_train(x, "bf16", deform_algo="transform")
    assert g2._dirty is False
    # the accepted values reach the device check, which is the first thing behind the switches
    object.__setattr__(net, "_dirty", False)
    for algo in ("gather", "transform"):
        with pytest.raises(NotImplementedError):
            net.forward_train(x, "bf16", deform_algo=algo)


def test_forward_train_mobilenet_switch():
    from tdrn_amd.model.dualrefinedet_mobilenet import build_net
    net = build_net("train", 320, 3)
    x = torch.zeros(1, 3, 320, 320)
    object.__setattr__(net, "_dirty", False)
    with pytest.raises(ValueError):
        net.forward_train(x, "fp32", deform_algo="transform")
    with pytest.raises(ValueError):
        net.forward_train(x, "fp16", deform_algo="sample")
    assert net._dirty is False
    g2 = build_net("train", 320, 3, def_groups=2)
    with pytest.raises(NotImplementedError, match="def_groups"):
        g2.forward_train(x, "fp16", deform_algo="transform")
