"""C ABI of the trainable MaxPool2d and L2Norm (tdrn_hip.h section i-e), no GPU needed: the output-size rule is torch's, the
workspace query is positive for the covered shapes, and the four launching entries decide every error before any launch, in the
header's order.  MaxPool2d has no state; L2Norm has the reference module's."""
import pytest
import torch
import torch.nn.functional as F

from tdrn_amd import _lib
from tdrn_amd.layers.modules.l2norm import L2Norm as TorchL2Norm
from tdrn_amd.model import networks

P = 256         # a fake non-null pointer: only compared with NULL (and its low bits) before any launch
ARG, SHAPE, WORKSPACE, UNSUPPORTED = -1, -2, -3, -4
GEOMETRIES = [(2, 2, 0, 0), (2, 2, 0, 1), (3, 1, 1, 0)]        # kernel, stride, pad, ceil_mode
# not on the list
OTHER_GEOMETRIES = [(2, 1, 0, 0), (3, 2, 0, 0), (3, 2, 1, 1), (2, 2, 1, 0), (3, 1, 0, 0), (1, 1, 0, 0), (3, 3, 1, 0), (0, 2, 0, 0),
                    (2, 0, 0, 0), (2, 2, -1, 0)]
GOOD = (2, 5, 7, 9)
# the shapes of tests/test_gpu_l2norm.py, and the measured layers
L2_SHAPES = [(2, 5, 7, 9), (3, 70, 1, 1), (2, 70, 5, 5), (2, 512, 10, 10), (1, 1030, 4, 6), (1, 3, 64, 130), (4, 6, 40, 40), (2, 32, 5, 5),
             (32, 512, 40, 40), (8, 512, 20, 20)]
# 2^31 elements or more, and the largest count that is covered
TOO_LARGE = [(64, 1024, 256, 256), (1 << 16, 1 << 16, 1, 1), (1, 1, 1 << 16, 1 << 16), (2, 1, 1 << 15, 1 << 15)]
LARGEST = (1, 1, 1 << 15, (1 << 16) - 1)


def _pool_fwd(lib, dims, geo=(2, 2, 0, 0), ptrs=(P, P, P)):
    """an entry on fake pointers, called only where a check ahead of the first launch fails"""
    return lib.tdrn_max_pool_forward(*ptrs, *dims, *geo, None)


def _pool_bwd(lib, dims, geo=(2, 2, 0, 0), ptrs=(P, P, P)):
    return lib.tdrn_max_pool_backward(*ptrs, *dims, *geo, None)


def _l2_fwd(lib, dims, eps=1e-10, ptrs=(P, P, P, P)):
    return lib.tdrn_l2norm_forward(*ptrs, *dims, eps, None)


def _l2_bwd(lib, dims, nb, eps=1e-10, ptrs=(P,) * 6, ws=P):
    return lib.tdrn_l2norm_backward(*ptrs, *dims, eps, 1.0, ws, nb, None)


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_max_pool_output_size_is_torchs(geo):
    lib = _lib.lib()
    k, s, p, ceil = geo
    for n in range(1, 71):
        try:
            want = F.max_pool2d(torch.zeros(1, 1, n, n), k, s, p, ceil_mode=bool(ceil)).shape[-1]
        except RuntimeError:
            want = 0
        assert lib.tdrn_max_pool_output_size(n, k, s, p, ceil) == want, (geo, n)
    assert lib.tdrn_max_pool_output_size(0, k, s, p, ceil) == 0 and lib.tdrn_max_pool_output_size(-3, k, s, p, ceil) == 0


def test_max_pool_geometries_outside_the_list_are_refused():
    lib = _lib.lib()
    for geo in OTHER_GEOMETRIES:
        assert lib.tdrn_max_pool_output_size(8, *geo) == 0, geo
        assert _pool_fwd(lib, (2, 3, 8, 8), geo) == UNSUPPORTED, geo
        assert _pool_bwd(lib, (2, 3, 8, 8), geo) == UNSUPPORTED, geo
    # 3 / 1 / 1 gives the same output in either rounding mode
    assert lib.tdrn_max_pool_output_size(8, 3, 1, 1, 1) == 8


def test_max_pool_errors_in_order():
    lib = _lib.lib()
    bad_geo, big = (2, 1, 0, 0), TOO_LARGE[0]
    for fn in (_pool_fwd, _pool_bwd):
        # 1. a null required pointer, ahead of every other fault
        for i in range(3):
            if fn is _pool_fwd and i == 2:
                continue                            # the forward's code is optional
            ptrs = [P, P, P]
            ptrs[i] = None
            assert fn(lib, (0, 5, 7, 9), bad_geo, ptrs) == ARG, (fn.__name__, i)
        assert fn(lib, GOOD, ptrs=(P + 2, P, P)) == ARG             # a float tensor off a 4-byte boundary
        # 2. sizes, ahead of the geometry and of the element limit
        for dims in ((0, 5, 7, 9), (2, 0, 7, 9), (2, 5, -1, 9), (2, 5, 7, 0)):
            assert fn(lib, dims, bad_geo) == SHAPE, (fn.__name__, dims)
        assert fn(lib, (2, 5, 1, 9), (2, 2, 0, 0)) == SHAPE          # no 2x2 window fits a row in floor mode
        assert fn(lib, (1 << 16, 1 << 16, 1, 1), (2, 2, 0, 0)) == SHAPE
        # 3. the element limit and the geometry
        for dims in TOO_LARGE[:1] + TOO_LARGE[2:]:
            for geo in GEOMETRIES:
                assert fn(lib, dims, geo) == UNSUPPORTED, (fn.__name__, dims, geo)
        assert fn(lib, big, bad_geo) == UNSUPPORTED
    # an inference-only forward passes the pointer check without a code tensor: the next fault decides
    assert _pool_fwd(lib, (0, 5, 7, 9), ptrs=(P, P, None)) == SHAPE


def test_l2norm_query():
    lib = _lib.lib()
    for dims in L2_SHAPES:
        nb = lib.tdrn_l2norm_workspace_bytes(*dims)
        assert nb > 0, dims
        # a pure function of (N, C, H W)
        N, C, H, W = dims
        assert lib.tdrn_l2norm_workspace_bytes(N, C, W, H) == nb == lib.tdrn_l2norm_workspace_bytes(N, C, 1, H * W)
        assert nb == 4 * C * ((N * H * W + 63) // 64)                  # tdrn_hip.h
    for dims in ((0, 5, 7, 9), (2, 0, 7, 9), (2, 5, -1, 9), (2, 5, 7, 0)) + tuple(TOO_LARGE):
        assert lib.tdrn_l2norm_workspace_bytes(*dims) == 0, dims
    assert lib.tdrn_l2norm_workspace_bytes(*LARGEST) > 0


def test_l2norm_errors_in_order():
    lib = _lib.lib()
    nb = lib.tdrn_l2norm_workspace_bytes(*GOOD)
    zero = (0, 5, 7, 9)
    # 1. null required pointers and eps, ahead of a bad shape.  forward: input, weight, output, norm (optional)
    for i in range(3):
        ptrs = [P] * 4
        ptrs[i] = None
        assert _l2_fwd(lib, zero, ptrs=ptrs) == ARG, i
    assert _l2_fwd(lib, zero, ptrs=(P, P, P, None)) == SHAPE
    # backward: input, grad_output, weight, norm, grad_input (optional), grad_weight (optional)
    for i in range(4):
        ptrs = [P] * 6
        ptrs[i] = None
        assert _l2_bwd(lib, zero, nb, ptrs=ptrs) == ARG, i
    assert _l2_bwd(lib, GOOD, nb, ptrs=(P, P, P, P, None, None)) == ARG           # nothing asked for
    for eps in (0.0, -1e-10, float("nan")):
        assert _l2_fwd(lib, zero, eps=eps) == ARG and _l2_bwd(lib, zero, 0, eps=eps) == ARG
    assert _l2_fwd(lib, GOOD, ptrs=(P + 2, P, P, P)) == ARG and _l2_bwd(lib, GOOD, nb, ptrs=(P, P, P, P, P + 1, P)) == ARG
    # 2. sizes, with a short workspace as well
    for dims in (zero, (2, 0, 7, 9), (2, 5, -1, 9), (2, 5, 7, 0)):
        assert _l2_fwd(lib, dims) == SHAPE and _l2_bwd(lib, dims, 0) == SHAPE, dims
    # 3. the element limit, with a short workspace as well
    for dims in TOO_LARGE:
        assert _l2_fwd(lib, dims) == UNSUPPORTED and _l2_bwd(lib, dims, 0) == UNSUPPORTED, dims
    # 4. a short workspace is decided last, and only grad_weight needs one
    for dims in L2_SHAPES:
        nb = lib.tdrn_l2norm_workspace_bytes(*dims)
        assert _l2_bwd(lib, dims, nb - 1) == WORKSPACE and _l2_bwd(lib, dims, nb, ws=None) == WORKSPACE, dims
        assert _l2_bwd(lib, dims, nb - 1, ptrs=(P, P, P, P, None, P)) == WORKSPACE, dims
    assert _l2_bwd(lib, LARGEST, 0) == WORKSPACE


def test_modules_have_the_expected_state_and_defaults():
    m = networks.MaxPool2d(2)
    assert list(m.state_dict()) == [] and list(m.parameters()) == []
    assert (m.kernel_size, m.stride, m.padding, m.ceil_mode) == (2, 2, 0, False)
    r = torch.nn.MaxPool2d(2)
    assert (r.kernel_size, r.stride, r.padding, r.ceil_mode) == (m.kernel_size, m.stride, m.padding, m.ceil_mode)
    m = networks.MaxPool2d(3, 1, 1, ceil_mode=True)
    assert (m.kernel_size, m.stride, m.padding, m.ceil_mode) == (3, 1, 1, True)
    ours, ref = networks.L2Norm(512, 10), TorchL2Norm(512, 10)
    assert list(ours.state_dict()) == list(ref.state_dict()) == ["weight"]
    assert torch.equal(ours.weight, ref.weight) and ours.weight.shape == (512,) and float(ours.weight.detach()[0]) == 10.0
    assert (ours.n_channels, ours.gamma, ours.eps) == (ref.n_channels, ref.gamma, ref.eps) == (512, 10, 1e-10)
    ref.weight.data.uniform_(8, 12)
    ours.load_state_dict(ref.state_dict(), strict=True)
    assert torch.equal(ours.weight, ref.weight)


def test_cpu_tensors_and_bad_arguments_raise():
    x = torch.zeros(2, 4, 6, 6)
    with pytest.raises(NotImplementedError):
        networks.max_pool2d(x, 2)
    with pytest.raises(NotImplementedError):
        networks.MaxPool2dFunction.apply(x, 2, 2, 0, True)
    with pytest.raises(NotImplementedError):
        networks.MaxPool2d(3, 1, 1)(x)
    with pytest.raises(NotImplementedError):
        networks.l2norm(x, torch.ones(4))
    with pytest.raises(NotImplementedError):
        networks.L2NormFunction.apply(x, torch.ones(4), 1e-10)
    with pytest.raises(NotImplementedError):
        networks.L2Norm(4, 10)(x)
    with pytest.raises(ValueError):
        networks.max_pool2d(x[0], 2)                       # 3-D
    with pytest.raises(ValueError):
        networks.max_pool2d(x.double(), 2)
    with pytest.raises(ValueError):
        networks.l2norm(x[0], torch.ones(4))
    with pytest.raises(ValueError):
        networks.l2norm(x.double(), torch.ones(4))


def test_l2norm_refuses_a_cpu_weight_beside_a_gpu_input():
    class OnGpu(object):             # stands in for a CUDA input on a machine without one; the check reads nothing else
        is_cuda = True
        shape = (2, 4, 6, 6)
        dtype = torch.float32

        def dim(self):
            return 4
    with pytest.raises(NotImplementedError):
        networks._l2norm_check(OnGpu(), torch.ones(4), 1e-10)
