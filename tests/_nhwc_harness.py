"""What the GPU tests of the resident-tensor entries share (tdrn_hip.h section i-k; test_gpu_nhwc_conv.py, test_gpu_nhwc_batch_norm.py,
test_gpu_nhwc_pool.py, test_gpu_train_resident.py): resident tensors from NCHW values, the C entries on plain device buffers, the
bounds of the 16-bit outputs and guarded resident buffers.

Notation of the bounds: u = the unit roundoff of nearest-even (2^-8 bf16, 2^-11 fp16), tiny = the type's smallest normal, c = C_ACC of
tests/_conv_train_harness.py, S = the same op on absolute values."""
import torch

from tdrn_amd import _lib

from _conv_train_harness import C_ACC, DEV, Guarded

TYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
TINY = {"bf16": float(torch.finfo(torch.bfloat16).tiny), "fp16": float(torch.finfo(torch.float16).tiny)}


def exact(t, mode):
    """fp32 values that the 16-bit type of `mode` holds exactly"""
    return t.float().to(TYPES[mode]).float()


def resident(t, mode):
    """NCHW values (exact in the type) -> the resident tensor on the device"""
    return t.to(DEV).to(TYPES[mode]).contiguous(memory_format=torch.channels_last)


def nchw64(t):
    """a resident (or any) device tensor -> float64 NCHW on the CPU"""
    return t.detach().float().cpu().double().contiguous()


def raw_equal(p, q):
    """bit for bit, as 16-bit words in memory order"""
    assert p.dtype == q.dtype and p.shape == q.shape
    a, b = (t.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1).contiguous().view(torch.int16) for t in (p, q))
    return torch.equal(a, b)


def bound16(mode, ref, S):
    """c S + u (|ref| + c S) + tiny: fp32 accumulation, then one rounding of the result"""
    c = C_ACC[mode]
    return c * S + U[mode] * (ref.abs() + c * S) + TINY[mode]


def assert_within(what, got, ref, bound):
    d = (got - ref).abs()
    assert torch.isfinite(got).all(), "%s: non-finite values" % what
    ratio = float((d / bound.clamp_min(1e-300)).max())
    print("%s: max|d| %.3e  worst share of the bound %.3e" % (what, float(d.max()), ratio))
    assert bool((d <= bound).all()), (what, ratio)


class GuardedResident(object):
    """a resident tensor of logical shape (N, C, H, W) in guarded device memory that starts `offset` (a multiple of 16) bytes behind a
    256-byte boundary"""

    def __init__(self, shape, mode, offset=16, init=None):
        N, Cc, H, W = shape
        self.g = Guarded(nbytes=2 * N * Cc * H * W, offset=offset)
        self.t = self.g.t.view(TYPES[mode]).view(N, H, W, Cc).permute(0, 3, 1, 2)
        assert self.t.is_contiguous(memory_format=torch.channels_last) and self.t.data_ptr() % 16 == 0
        if init is not None:
            self.t.copy_(init)

    def check(self, what, full=True):
        self.g.check(what, full)


def stream():
    return _lib.current_stream(DEV)


class ConvAbi(object):
    """the conv entries on plain device buffers: x, go resident; w, b fp32"""

    def __init__(self, dims, mode, flags=0):
        self.lib, self.dims, self.mode, self.dt, self.flags = _lib.lib(), tuple(dims), mode, _lib.DTYPES[mode], flags
        self.nb = self.lib.tdrn_conv2d_nhwc_workspace_bytes(*self.dims, self.dt, flags)
        assert self.nb > 0
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)

    def route(self, dgrad):
        return self.lib.tdrn_conv2d_nhwc_route(*self.dims, self.dt, self.flags, dgrad).decode()

    def forward(self, x, w, b, out):
        _lib.check(self.lib.tdrn_conv2d_nhwc_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(out), *self.dims, self.dt,
                                                     _lib.ptr(self.ws), self.nb, stream(), self.flags))
        return out

    def backward_input(self, go, w, gi):
        _lib.check(self.lib.tdrn_conv2d_nhwc_backward_input(_lib.ptr(go), _lib.ptr(w), _lib.ptr(gi), *self.dims, self.dt,
                                                            _lib.ptr(self.ws), self.nb, stream(), self.flags))
        return gi

    def backward_parameters(self, x, go, gw, gb, scale=1.0):
        _lib.check(self.lib.tdrn_conv2d_nhwc_backward_parameters(_lib.ptr(x), _lib.ptr(go), _lib.ptr(gw), _lib.ptr(gb), *self.dims, scale,
                                                                 self.dt, _lib.ptr(self.ws), self.nb, stream(), self.flags))
        return gw, gb


def bn_workspace(dims):
    nb = _lib.lib().tdrn_batch_norm_nhwc_workspace_bytes(*dims)
    assert nb > 0
    return torch.empty(nb, dtype=torch.uint8, device=DEV), nb


def bn_forward(x, w, b, rm, rv, out, save_mean, save_invstd, training, momentum, eps, relu, mode):
    dims = tuple(x.shape)
    ws, nb = bn_workspace(dims)
    _lib.check(_lib.lib().tdrn_batch_norm_nhwc_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(rm), _lib.ptr(rv), _lib.ptr(out),
                                                       _lib.ptr(save_mean), _lib.ptr(save_invstd), *dims, int(training), momentum, eps,
                                                       int(relu), _lib.DTYPES[mode], _lib.ptr(ws), nb, stream()))


def bn_backward(x, go, w, b, save_mean, save_invstd, gi, gw, gb, training, relu, scale, mode):
    dims = tuple(x.shape)
    ws, nb = bn_workspace(dims)
    _lib.check(_lib.lib().tdrn_batch_norm_nhwc_backward(_lib.ptr(x), _lib.ptr(go), _lib.ptr(w), _lib.ptr(b), _lib.ptr(save_mean),
                                                        _lib.ptr(save_invstd), _lib.ptr(gi), _lib.ptr(gw), _lib.ptr(gb), *dims,
                                                        int(training), int(relu), scale, _lib.DTYPES[mode], _lib.ptr(ws), nb, stream()))


def pool_forward(x, out, code, geo, mode):
    _lib.check(_lib.lib().tdrn_max_pool_nhwc_forward(_lib.ptr(x), _lib.ptr(out), _lib.ptr(code), *x.shape, *geo, _lib.DTYPES[mode], stream()))


def pool_backward(go, code, gi, geo, mode):
    _lib.check(_lib.lib().tdrn_max_pool_nhwc_backward(_lib.ptr(go), _lib.ptr(code), _lib.ptr(gi), *gi.shape, *geo, _lib.DTYPES[mode],
                                                      stream()))
