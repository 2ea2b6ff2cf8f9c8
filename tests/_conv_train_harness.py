"""What the GPU tests of the three trainable conv families share (test_gpu_conv_grad.py, test_gpu_conv_transpose.py,
test_gpu_conv_strided.py): the four C entries of a family on plain device buffers, the bound check against a float64 reference,
bitwise comparison and guarded device buffers.  Cases, inputs, seeds and references stay with each test file.

Bounds.  fp32 mode: |got - ref| <= 1e-4 * max(1, max|ref|).  16-bit modes: the inputs are exact and the products are exact in fp32, so
only the fp32 accumulation is left: |got - ref| <= c * S elementwise, S = the same op on absolute values, c = C_ACC of
test_gpu_pin16.py (2e-6 bf16, 4e-5 fp16).  Outputs are fp32: no element is exempted.
"""
import torch

from tdrn_amd import _lib

DEV = "cuda:0"
DT = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}
C_ACC = {"bf16": 2e-6, "fp16": 4e-5}
NAMES = ("output", "grad_input", "grad_weight", "grad_bias")


def round_to(t, mode):
    """a tensor as the op uses it: rounded to the 16-bit type of `mode`, back in fp32"""
    return t if DT[mode] is None else t.to(DT[mode]).float()


def compare(case, mode, name, g, r, s, floor=1.0):
    """one tensor `g` against its ready float64 reference `r` and absolute-value sum `s` (unused in fp32 mode) -> the worst share
    of the bound, printed before it is asserted.  `floor`: the 1 of max(1, max|ref|) in fp32 mode; tests/_train_stage_ref.py passes
    0 (the bound is then 1e-4 max|ref|, and a reference that is all zero asks for exact zeros)."""
    assert tuple(g.shape) == tuple(r.shape), (case, mode, name)
    d = (g.detach().cpu().double() - r).abs()
    assert torch.isfinite(d).all(), "%s %s %s: non-finite values" % (case, mode, name)
    if mode == "fp32":
        bound = 1e-4 * max(floor, float(r.abs().max()))
        if bound == 0.0:
            print("%s %s %-11s max|d| %.3e  reference all zero" % (case, mode, name, float(d.max())))
            assert float(d.max()) == 0.0, (case, mode, name, float(d.max()), bound)
            return 0.0
        print("%s %s %-11s max|d| %.3e  bound %.3e  ratio %.3e" % (case, mode, name, float(d.max()), bound, float(d.max()) / bound))
        assert float(d.max()) <= bound, (case, mode, name, float(d.max()), bound)
        return float(d.max()) / bound
    ratio = float((d / s.clamp_min(1e-300)).max())
    print("%s %s %-11s max|d|/S %.3e  c %.1e" % (case, mode, name, ratio, C_ACC[mode]))
    assert bool((d <= C_ACC[mode] * s).all()), (case, mode, name, ratio, C_ACC[mode])
    return ratio / C_ACC[mode]


def check(reference, case, mode, names, got):
    """reference(case, mode) -> ((y, gx, gw, gb), (Sy, Sgx, Sgw, Sgb)) in float64; `got`: the tensors that `names` name"""
    ref, S = reference(case, mode)
    for name, g in zip(names, got):
        compare(case, mode, name, g, ref[NAMES.index(name)], S[NAMES.index(name)])


class Abi(object):
    """the four C entries of the family `prefix` on plain device buffers; inputs = (x, w, b, grad_output) on the CPU"""

    def __init__(self, prefix, dims, inputs, mode):
        self.lib, self.prefix, self.dims, self.dt = _lib.lib(), prefix, dims, _lib.DTYPES[mode]
        self.nb = self._entry("workspace_bytes")(*self.dims, self.dt)
        assert self.nb > 0
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)
        self.x, self.w, self.b, self.go = (t.to(DEV) for t in inputs)

    def _entry(self, name):
        return getattr(self.lib, "%s_%s" % (self.prefix, name))

    def forward(self, out, bias=True):
        _lib.check(self._entry("forward")(_lib.ptr(self.x), _lib.ptr(self.w), _lib.ptr(self.b if bias else None), _lib.ptr(out),
                                          *self.dims, self.dt, _lib.ptr(self.ws), self.nb, _lib.current_stream(DEV)))
        return out

    def backward_input(self, gi):
        _lib.check(self._entry("backward_input")(_lib.ptr(self.go), _lib.ptr(self.w), _lib.ptr(gi), *self.dims, self.dt,
                                                 _lib.ptr(self.ws), self.nb, _lib.current_stream(DEV)))
        return gi

    def backward_parameters(self, gw, gb, scale=1.0):
        _lib.check(self._entry("backward_parameters")(_lib.ptr(self.x), _lib.ptr(self.go), _lib.ptr(gw), _lib.ptr(gb), *self.dims, scale,
                                                      self.dt, _lib.ptr(self.ws), self.nb, _lib.current_stream(DEV)))
        return gw, gb

    def all(self):
        out = self.forward(torch.full_like(self.go, float("nan")))
        gi = self.backward_input(torch.full_like(self.x, float("nan")))
        gw, gb = self.backward_parameters(torch.zeros_like(self.w), torch.zeros_like(self.b))
        torch.cuda.synchronize()
        return out, gi, gw, gb


def bits_equal(p, q):
    return torch.equal(p.contiguous().view(torch.int32), q.contiguous().view(torch.int32))


SENTINEL = 0x7FBADBAD
GUARD = 4096


class Guarded(object):
    """`nbytes` of device memory that start `offset` bytes behind a 256-byte boundary, between two guard bands of a NaN pattern no
    kernel computes (the pattern of test_gpu_caller_memory.py)"""

    def __init__(self, shape=None, offset=0, nbytes=None, init=None):
        n = int(nbytes) if nbytes is not None else 4 * int(torch.Size(shape).numel())
        total = 2 * GUARD + 256 + offset + n
        self.raw = torch.full(((total + 3) // 4,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.uint8)
        base = (-self.raw.data_ptr()) % 256 + GUARD
        self.lo, self.hi = base + offset, base + offset + n
        body = self.raw[self.lo:self.hi]
        self.t = body if shape is None else body.view(torch.float32).view(shape)
        if init is not None:
            self.t.copy_(init)

    def check(self, what, full=True):
        torch.cuda.synchronize()
        words = self.raw.view(torch.int32)
        assert self.lo % 4 == 0 and self.hi % 4 == 0
        assert bool((words[:self.lo // 4] == SENTINEL).all()), "%s: bytes in front of the buffer were written" % what
        assert bool((words[self.hi // 4:] == SENTINEL).all()), "%s: bytes behind the end of the buffer were written" % what
        if full:
            assert int((words[self.lo // 4:self.hi // 4] == SENTINEL).sum()) == 0, "%s: elements never written" % what
