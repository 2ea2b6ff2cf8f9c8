"""C ABI of the dense conv2d with gradients (tdrn_hip.h section i-c), no GPU needed: the workspace query and the entries
decide every error before any launch."""
import pytest
import torch

from tdrn_amd import _lib
from tdrn_amd.model import networks

# N Cin H W Cout kH kW dH dW padH padW dilH dilW
GOOD = (2, 6, 9, 7, 4, 3, 3, 1, 1, 1, 1, 1, 1)


def _entries(lib, dims, dt, nb, p=256):
    """all three entries on fake non-null pointers.  Pointers are only compared with NULL before any launch, so this is called
    only where a check ahead of the first launch fails (bad geometry or a short workspace): a fake pointer never reaches a kernel."""
    assert nb < lib.tdrn_conv2d_workspace_bytes(*dims, dt) or lib.tdrn_conv2d_workspace_bytes(*dims, dt) == 0
    return (lib.tdrn_conv2d_forward(p, p, None, p, *dims, dt, p, nb, None),
            lib.tdrn_conv2d_backward_input(p, p, p, *dims, dt, p, nb, None),
            lib.tdrn_conv2d_backward_parameters(p, p, p, None, *dims, 1.0, dt, p, nb, None))


def test_conv2d_query_positive_for_supported_geometry():
    lib = _lib.lib()
    cases = [GOOD,
             (1, 3, 8, 8, 4, 3, 3, 1, 1, 1, 1, 1, 1),
             (1, 16, 13, 13, 24, 3, 3, 1, 1, 6, 6, 6, 6),        # conv6's geometry
             (1, 8, 10, 9, 8, 3, 3, 1, 1, 0, 0, 1, 1),           # valid conv
             (1, 8, 10, 9, 8, 3, 3, 1, 1, 2, 2, 1, 1),           # pad = dil (k - 1)
             (2, 140, 6, 6, 12, 1, 1, 1, 1, 0, 0, 1, 1),         # 1x1
             (32, 256, 80, 80, 256, 3, 3, 1, 1, 1, 1, 1, 1)]     # conv3_x at batch 32
    for dims in cases:
        for dt in (_lib.F32, _lib.BF16, _lib.F16):
            assert lib.tdrn_conv2d_workspace_bytes(*dims, dt) > 0, (dims, dt)


@pytest.mark.parametrize("dims", [
    (2, 6, 9, 7, 4, 0, 3, 1, 1, 1, 1, 1, 1),      # k <= 0
    (2, 6, 9, 7, 4, 3, -1, 1, 1, 1, 1, 1, 1),
    (2, 6, 9, 7, 4, 3, 3, 0, 1, 1, 1, 1, 1),      # stride <= 0
    (2, 6, 9, 7, 4, 3, 3, 1, 1, 1, 1, 0, 1),      # dilation <= 0
    (2, 6, 9, 7, 4, 3, 3, 1, 1, -1, 1, 1, 1),     # negative pad
    (0, 6, 9, 7, 4, 3, 3, 1, 1, 1, 1, 1, 1),      # N <= 0
    (2, 6, 2, 2, 4, 3, 3, 1, 1, 0, 0, 1, 1),      # output smaller than 1 x 1
    (2, 6, 9, 7, 4, 3, 3, 1, 1, 1, 1, 6, 6),      # ... through the dilation
])
def test_conv2d_bad_sizes_are_shape_errors(dims):
    lib = _lib.lib()
    for dt in (_lib.F32, _lib.BF16, _lib.F16):
        assert lib.tdrn_conv2d_workspace_bytes(*dims, dt) == 0
        assert _entries(lib, dims, dt, 1 << 20) == (-2, -2, -2)


@pytest.mark.parametrize("dims", [
    (2, 6, 9, 7, 4, 3, 3, 2, 2, 1, 1, 1, 1),      # stride 2
    (2, 6, 9, 7, 4, 5, 5, 1, 1, 2, 2, 1, 1),      # k = 5
    (2, 6, 9, 7, 4, 3, 3, 1, 1, 3, 3, 1, 1),      # pad = 3 > dil (k - 1) at k = 3, dil = 1
    (2, 6, 9, 7, 4, 3, 1, 1, 1, 1, 0, 1, 1),      # not square
    (64, 1024, 256, 256, 64, 3, 3, 1, 1, 1, 1, 1, 1),   # past the kernels' 32-bit offsets
])
def test_conv2d_uncovered_geometry_is_unsupported(dims):
    lib = _lib.lib()
    for dt in (_lib.F32, _lib.BF16, _lib.F16):
        assert lib.tdrn_conv2d_workspace_bytes(*dims, dt) == 0
        assert _entries(lib, dims, dt, 1 << 20) == (-4, -4, -4)


def test_conv2d_short_workspace_and_null_pointers():
    lib = _lib.lib()
    p = 256
    for dt in (_lib.F32, _lib.BF16, _lib.F16):
        nb = lib.tdrn_conv2d_workspace_bytes(*GOOD, dt)
        assert _entries(lib, GOOD, dt, nb - 1) == (-3, -3, -3)
        assert lib.tdrn_conv2d_forward(p, p, None, p, *GOOD, dt, None, nb, None) == -3            # no workspace at all
        # a null tensor pointer is refused first, whatever else is passed: every call below has one
        assert lib.tdrn_conv2d_backward_input(None, p, p, *GOOD, dt, p, nb, None) == -1             # grad_output
        assert lib.tdrn_conv2d_backward_parameters(p, None, p, None, *GOOD, 1.0, dt, p, nb, None) == -1
        assert lib.tdrn_conv2d_backward_parameters(None, p, p, None, *GOOD, 1.0, dt, p, nb, None) == -1
        assert lib.tdrn_conv2d_backward_input(p, p, None, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv2d_forward(p, p, None, None, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv2d_forward(None, p, None, p, *GOOD, dt, p, nb, None) == -1


def test_conv2d_rejects_cpu_tensors():
    x, w = torch.zeros(1, 3, 8, 8), torch.zeros(4, 3, 3, 3)
    with pytest.raises(NotImplementedError):
        networks.Conv2dFunction.apply(x, w, None, 1, 1)
    with pytest.raises(NotImplementedError):
        networks.conv2d(x, w, None, 1, 1)
    with pytest.raises(NotImplementedError):
        networks.Conv2d(3, 4, 3, padding=1)(x)


def test_conv2d_refuses_cpu_weight_and_bias_beside_a_gpu_input():
    class OnGpu(object):             # stands in for a CUDA input on a machine without one; the check reads nothing else
        is_cuda = True
    w, b = torch.zeros(4, 3, 3, 3), torch.zeros(4)
    with pytest.raises(NotImplementedError):
        networks._conv2d_require_cuda(OnGpu(), w, None)
    with pytest.raises(NotImplementedError):
        networks._conv2d_require_cuda(OnGpu(), OnGpu(), b)
    networks._conv2d_require_cuda(OnGpu(), OnGpu(), None)


def test_conv2d_module_has_nn_conv2d_parameters():
    m, r = networks.Conv2d(5, 7, 3, padding=1), torch.nn.Conv2d(5, 7, 3, padding=1)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in r.state_dict().items()}
    assert networks.Conv2d(5, 7, 1, bias=False).bias is None
