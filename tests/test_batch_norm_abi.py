"""C ABI of BatchNorm2d with a fused ReLU (tdrn_hip.h section i-d), no GPU needed: the workspace query and both entries decide
every error before any launch; the module has nn.BatchNorm2d's state."""
import pytest
import torch

from tdrn_amd import _lib
from tdrn_amd.model import networks

GOOD = (2, 5, 7, 9)
SHAPES = [GOOD, (2, 3, 1, 1), (6, 70, 1, 1), (2, 70, 5, 5), (3, 130, 10, 10), (4, 3, 40, 40), (1, 2, 64, 130), (3, 4, 33, 31),
          (32, 2, 40, 40), (32, 64, 320, 320)]
P = 256         # a fake non-null pointer: only compared with NULL (and its low bits) before any launch


def _fwd(lib, dims, nb, training=1, momentum=0.1, eps=1e-5, ptrs=None, ws=P):
    """the forward entry on fake pointers, called only where a check ahead of the first launch fails"""
    ptrs = [P] * 8 if ptrs is None else ptrs
    return lib.tdrn_batch_norm_forward(*ptrs, *dims, training, momentum, eps, 1, ws, nb, None)


def _bwd(lib, dims, nb, training=1, ptrs=None, ws=P):
    ptrs = [P] * 9 if ptrs is None else ptrs
    return lib.tdrn_batch_norm_backward(*ptrs, *dims, training, 1, 1.0, ws, nb, None)


def test_batch_norm_query_is_positive_for_supported_shapes():
    lib = _lib.lib()
    for dims in SHAPES:
        assert lib.tdrn_batch_norm_workspace_bytes(*dims) > 0, dims
    assert lib.tdrn_batch_norm_workspace_bytes(1, 70, 1, 1) > 0          # one value per channel: legal in eval mode


@pytest.mark.parametrize("dims", [(0, 5, 7, 9), (2, 0, 7, 9), (2, 5, -1, 9), (2, 5, 7, 0)])
def test_batch_norm_non_positive_sizes_are_shape_errors(dims):
    lib = _lib.lib()
    assert lib.tdrn_batch_norm_workspace_bytes(*dims) == 0
    for training in (0, 1):
        assert _fwd(lib, dims, 1 << 20, training) == -2
        assert _bwd(lib, dims, 1 << 20, training) == -2


def test_batch_norm_one_value_per_channel_is_refused_in_training_only():
    lib = _lib.lib()
    for dims in ((1, 70, 1, 1), (1, 1, 1, 1)):
        nb = lib.tdrn_batch_norm_workspace_bytes(*dims)
        assert nb > 0
        assert _fwd(lib, dims, nb, training=1) == -2 and _bwd(lib, dims, nb, training=1) == -2
        # eval mode passes every check up to the workspace's
        assert _fwd(lib, dims, nb - 1, training=0) == -3 and _bwd(lib, dims, nb - 1, training=0) == -3
    # two values per channel are legal
    nb = lib.tdrn_batch_norm_workspace_bytes(2, 3, 1, 1)
    assert _fwd(lib, (2, 3, 1, 1), nb - 1) == -3 and _bwd(lib, (2, 3, 1, 1), nb - 1) == -3


def test_batch_norm_past_32_bit_offsets_is_unsupported():
    lib = _lib.lib()
    for dims in ((64, 1024, 256, 256), (1 << 16, 1 << 16, 1, 1), (1, 1, 1 << 16, 1 << 16), (2, 1, 1 << 15, 1 << 15)):
        assert lib.tdrn_batch_norm_workspace_bytes(*dims) == 0
        assert _fwd(lib, dims, 1 << 20) == -4 and _bwd(lib, dims, 1 << 20) == -4
    assert lib.tdrn_batch_norm_workspace_bytes(1, 1, 1 << 15, (1 << 16) - 1) > 0      # 2^31 - 2^15 elements


def test_batch_norm_bad_arguments():
    lib = _lib.lib()
    nb = lib.tdrn_batch_norm_workspace_bytes(*GOOD)
    # these pass the pointer and shape checks and fail on the scalar; the workspace is short as well, which is decided later
    assert _fwd(lib, GOOD, nb - 1, eps=0.0) == -1
    assert _fwd(lib, GOOD, nb - 1, eps=-1e-5) == -1
    assert _fwd(lib, GOOD, nb - 1, eps=float("nan")) == -1
    assert _fwd(lib, GOOD, nb - 1, momentum=1.5) == -1
    assert _fwd(lib, GOOD, nb - 1, momentum=-0.1) == -1
    assert _fwd(lib, GOOD, nb - 1, momentum=0.0) == -3 and _fwd(lib, GOOD, nb - 1, momentum=1.0) == -3
    # forward: input, weight, bias, running_mean, running_var, output, save_mean, save_invstd
    for i in (0, 1, 2, 5, 6, 7):
        ptrs = [P] * 8
        ptrs[i] = None
        assert _fwd(lib, GOOD, nb, ptrs=ptrs) == -1, i
    # the running buffers: both or neither in training, both in eval mode
    assert _fwd(lib, GOOD, nb, ptrs=[P, P, P, None, P, P, P, P]) == -1
    assert _fwd(lib, GOOD, nb, ptrs=[P, P, P, P, None, P, P, P]) == -1
    assert _fwd(lib, GOOD, nb, training=0, ptrs=[P, P, P, None, None, P, P, P]) == -1
    assert _fwd(lib, GOOD, nb - 1, training=1, ptrs=[P, P, P, None, None, P, P, P]) == -3
    # backward: input, grad_output, weight, bias, save_mean, save_invstd, grad_input, grad_weight, grad_bias
    for i in range(6):
        ptrs = [P] * 9
        ptrs[i] = None
        assert _bwd(lib, GOOD, nb, ptrs=ptrs) == -1, i
    assert _bwd(lib, GOOD, nb, ptrs=[P] * 7 + [P, None]) == -1            # grad_weight without grad_bias
    assert _bwd(lib, GOOD, nb, ptrs=[P] * 7 + [None, P]) == -1
    assert _bwd(lib, GOOD, nb, ptrs=[P] * 6 + [None, None, None]) == -1   # nothing asked for
    assert _bwd(lib, GOOD, nb - 1, ptrs=[P] * 6 + [None, P, P]) == -3
    assert _bwd(lib, GOOD, nb - 1, ptrs=[P] * 6 + [P, None, None]) == -3
    # a tensor off a 4-byte boundary
    assert _fwd(lib, GOOD, nb, ptrs=[P + 2] + [P] * 7) == -1
    assert _bwd(lib, GOOD, nb, ptrs=[P] * 6 + [P + 1, P, P]) == -1


def test_batch_norm_short_workspace():
    lib = _lib.lib()
    for dims in SHAPES:
        nb = lib.tdrn_batch_norm_workspace_bytes(*dims)
        for training in (0, 1):
            assert _fwd(lib, dims, nb - 1, training) == -3 and _bwd(lib, dims, nb - 1, training) == -3
            assert _fwd(lib, dims, nb, training, ws=None) == -3 and _bwd(lib, dims, nb, training, ws=None) == -3


def test_batch_norm_split_counts_are_the_design_table():
    """the query returns 12 C splits + 8 C bytes (tdrn_hip.h): the split counts DESIGN.md section 12 lists are the library's"""
    import os
    import re
    lib = _lib.lib()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    rows = re.findall(r"^\| `?([\w ,]+?)`? \| (\d+), (\d+), (\d+), (\d+) \| (\d+) \| (\d+) \| (\d+) \|", text, re.M)
    seen = set()
    for name, N, C, H, W, M, per, splits in rows:
        N, C, H, W, M, per, splits = (int(v) for v in (N, C, H, W, M, per, splits))
        nb = lib.tdrn_batch_norm_workspace_bytes(N, C, H, W)
        assert M == N * H * W and nb == 12 * C * splits + 8 * C, name
        assert per % 4 == 0 and (splits - 1) * per < M <= splits * per, name
        seen.add((N, C, H, W))
    assert set(SHAPES) <= seen
    assert {(8, c, s, s) for c, s in ((64, 320), (128, 160), (256, 80), (512, 40), (1024, 10))} <= seen


def test_batch_norm_rejects_cpu_tensors():
    x, w, b, rm, rv = torch.zeros(2, 7, 4, 4), torch.ones(7), torch.zeros(7), torch.zeros(7), torch.ones(7)
    with pytest.raises(NotImplementedError):
        networks.BatchNormFunction.apply(x, rm, rv, w, b, True, 0.1, 1e-5, True)
    with pytest.raises(NotImplementedError):
        networks.batch_norm(x, rm, rv, w, b, True)
    with pytest.raises(NotImplementedError):
        networks.batch_norm(x, rm, rv, w, b, False, relu=True)
    m = networks.BatchNorm2d(7, relu=True)
    with pytest.raises(NotImplementedError):
        m(x)
    with pytest.raises(NotImplementedError):
        m.eval()(x)
    assert int(m.num_batches_tracked) == 0                                 # a refused call is no tracked batch
    with pytest.raises(ValueError):
        networks.batch_norm(x[0], rm, rv, w, b, True)                      # 3-D


def test_batch_norm_refuses_cpu_parameters_beside_a_gpu_input():
    class OnGpu(object):             # stands in for a CUDA input on a machine without one; the check reads nothing else
        is_cuda = True
        shape = (2, 7, 4, 4)

        def dim(self):
            return 4
    w, b, rm, rv = torch.ones(7), torch.zeros(7), torch.zeros(7), torch.ones(7)
    with pytest.raises(NotImplementedError):
        networks._batch_norm_check(OnGpu(), rm, rv, w, b, True)
    with pytest.raises(NotImplementedError):
        networks._batch_norm_check(OnGpu(), None, None, w, b, True)


def test_batch_norm_module_has_nn_batchnorm2d_state():
    m, r = networks.BatchNorm2d(7), torch.nn.BatchNorm2d(7)
    sm, sr = m.state_dict(), r.state_dict()
    assert list(sm) == list(sr) == ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    for k in sr:
        assert sm[k].shape == sr[k].shape and sm[k].dtype == sr[k].dtype and torch.equal(sm[k], sr[k]), k
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in r.named_parameters()]
    # each loads the other's state strictly, values included
    gen = torch.Generator().manual_seed(3)
    state = {"weight": torch.rand(7, generator=gen), "bias": torch.randn(7, generator=gen), "running_mean": torch.randn(7, generator=gen),
             "running_var": torch.rand(7, generator=gen) + 0.5, "num_batches_tracked": torch.tensor(4)}
    r.load_state_dict(state, strict=True)
    m.load_state_dict(r.state_dict(), strict=True)
    assert m._batches == 4
    r2 = torch.nn.BatchNorm2d(7)
    r2.load_state_dict(m.state_dict(), strict=True)
    for k, v in state.items():
        assert torch.equal(m.state_dict()[k], v) and torch.equal(r2.state_dict()[k], v), k
    assert (m.eps, m.momentum, m.relu) == (r.eps, r.momentum, False)
    m.reset_running_stats()
    assert m._batches == 0 and int(m.num_batches_tracked) == 0 and bool((m.running_var == 1).all())
