"""Parameter-holder builders mirroring model/networks.py of the reference (vgg :136-163,
conv_dw :736-745) and the deformable-conv module surface (conv_offset2d :600-615,
ConvOffset2dFunction :617-697, ConvOffset2d :699-733), plus the trainable dense conv (Conv2dFunction / conv2d / Conv2d: what
nn.Conv2d and autograd give the reference's training loop; stride 1, and 3x3 at stride 2) and the trainable batch norm with a fused ReLU (BatchNormFunction /
batch_norm / BatchNorm2d), max pool (MaxPool2dFunction / max_pool2d / MaxPool2d) and L2Norm (L2NormFunction / l2norm / L2Norm),
and the trainable 2x2 stride-2 transposed conv of the TCB up_layers (ConvTranspose2dFunction / conv_transpose2d / ConvTranspose2d),
and the trainable depthwise 3x3 conv of conv_dw (DepthwiseConv2dFunction / depthwise_conv2d / DepthwiseConv2d).
and the resident-tensor ops (to_nhwc / from_nhwc, conv2d_nhwc, batch_norm_nhwc, max_pool2d_nhwc: 16-bit NHWC activations and
gradients between layers, C ABI section i-k).
The modules only own parameters with the reference's names and
shapes; arithmetic happens in libtdrn_hip.so."""
import collections
import ctypes as C
import math

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from .. import _lib

vgg_base = {k: [64, 64, "M", 128, 128, "M", 256, 256, 256, "C", 512, 512, 512, "M", 512, 512, 512]
            for k in ("300", "320", "512")}


def vgg(cfg, i, batch_norm=False, pool5_ds=False, c7_channel=1024):
    layers, cin = [], i
    for v in cfg:
        if v in ("M", "C"):
            layers.append(nn.MaxPool2d(2, 2, ceil_mode=(v == "C")))
            continue
        layers.append(nn.Conv2d(cin, v, 3, padding=1))
        if batch_norm:
            layers.append(nn.BatchNorm2d(v))
        layers.append(nn.ReLU(inplace=True))
        cin = v
    layers.append(nn.MaxPool2d(2, 2) if pool5_ds else nn.MaxPool2d(3, 1, 1))
    for conv in (nn.Conv2d(512, 1024, 3, padding=6, dilation=6), nn.Conv2d(1024, c7_channel, 1)):
        layers.append(conv)
        if batch_norm:
            layers.append(nn.BatchNorm2d(conv.out_channels))
        layers.append(nn.ReLU(inplace=True))
    return layers


def conv_dw(inp, oup, stride):
    return nn.Sequential(nn.Conv2d(inp, inp, 3, stride, 1, groups=inp, bias=False), nn.BatchNorm2d(inp),
                         nn.ReLU(inplace=True),
                         nn.Conv2d(inp, oup, 1, 1, 0, bias=False), nn.BatchNorm2d(oup), nn.ReLU(inplace=True))


def mobilenet_backbone(c_last=1024):
    plan = [(32, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 1), (256, 256, 1), (256, 512, 2)] + \
           [(512, 512, 1)] * 5 + [(512, 1024, 2), (1024, c_last, 1)]
    first = nn.Sequential(nn.Conv2d(3, 32, 3, 2, 1, bias=False), nn.BatchNorm2d(32), nn.ReLU(inplace=True))
    return nn.ModuleList([first] + [conv_dw(a, b, s) for a, b, s in plan])


def _grad_output(grad_output, shape, op):
    """what every backward does first: a CUDA grad_output, as contiguous fp32, of the output's shape"""
    if not grad_output.is_cuda:
        raise NotImplementedError("%s backward: grad_output must be a CUDA tensor" % op)
    go = grad_output.float().contiguous()          # (y.sum().backward() hands in a stride-0 tensor)
    if tuple(go.shape) != tuple(shape):
        raise RuntimeError("grad_output has shape %r, expected %r" % (tuple(go.shape), tuple(shape)))
    return go


def _workspace(query, args, device, message, *what):
    """-> (a uint8 workspace of query(*args) bytes, its size); a query of 0 raises `message % what`"""
    nb = query(*args)
    if nb == 0:
        raise RuntimeError(message % what)
    return torch.empty(nb, dtype=torch.uint8, device=device), nb


def _dispatch(function, args, tracked, plain):
    """the grad-or-plain rule of every public op: through `function` when grad mode is on and one of `tracked` (tensors, or None)
    requires grad; else plain(), the forward alone on detached tensors, whose output has no grad_fn"""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tracked):
        return function.apply(*args)
    return plain()


# ---- resident tensors (tdrn_hip.h section i-k): activations and their gradients as 16-bit NHWC between layers ----------------------------
_RESIDENT_DTYPES = {torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}
_RESIDENT_NAMES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp16": torch.float16, "f16": torch.float16,
                   "float16": torch.float16, "half": torch.float16}
RESIDENT_CHANNELS = 64          # kChanPad: a resident tensor holds whole 64-channel blocks


def _resident_dtype(dtype):
    dtype = _RESIDENT_NAMES.get(dtype, dtype)
    if dtype not in _RESIDENT_DTYPES:
        raise ValueError("a resident tensor is torch.bfloat16 or torch.float16, got %r" % (dtype,))
    return dtype


def _resident(t, dtype=None):
    """`t` as a resident tensor: of `dtype` (default: its own), contiguous in channels_last, its data on a 16-byte boundary (a
    misaligned storage is cloned)"""
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    t = t.contiguous(memory_format=torch.channels_last)
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.channels_last)


def _resident_input(input, op):
    """the checks every resident op starts with -> the library's type code"""
    if input.dim() != 4:
        raise ValueError("Expected 4D tensor as input, got {}D tensor instead.".format(input.dim()))
    _lib.require_cuda(input, "input")
    if input.dtype not in _RESIDENT_DTYPES:
        raise ValueError("%s: input must be torch.bfloat16 or torch.float16 (got %s); to_nhwc makes one" % (op, input.dtype))
    if input.shape[1] % RESIDENT_CHANNELS:
        raise RuntimeError("%s: %d channels are outside what libtdrn_hip covers (a multiple of %d)" % (op, input.shape[1], RESIDENT_CHANNELS))
    return _RESIDENT_DTYPES[input.dtype]


def _resident_empty(shape, dtype, device):
    return torch.empty(tuple(shape), dtype=dtype, device=device, memory_format=torch.channels_last)


def _resident_grad_output(grad_output, shape, dtype, op):
    """what every resident backward does first: a CUDA grad_output of the output's shape, made resident whatever it arrives as"""
    if not grad_output.is_cuda:
        raise NotImplementedError("%s backward: grad_output must be a CUDA tensor" % op)
    if tuple(grad_output.shape) != tuple(shape):
        raise RuntimeError("grad_output has shape %r, expected %r" % (tuple(grad_output.shape), tuple(shape)))
    return _resident(grad_output, dtype)


# One tensor format of the training ops: what differs between an op on fp32 NCHW tensors and its twin on resident ones, and nothing else.
#   infix: in the C entries' names and behind the op's name in messages; covered: the channel rule in a "shape outside" message
#   check(input, op): the format's own checks of an op's input, before the op's
#   ready(t): `t` as the entries read it (for max_pool2d, which has checked for float32, no cast: plain contiguous())
#   empty(like, shape=None): an output or gradient like `like`, or of `shape` in like's type and on its device
#   grad_output(grad_output, shape, dtype, op): what a backward does first
#   codes(dtype) -> the type-code arguments of an entry; code_shape(N, C, Ho, Wo) -> the shape of max pool's code tensor
_Format = collections.namedtuple("_Format", "infix covered check ready empty grad_output codes code_shape")
_NCHW = _Format("", "", lambda input, op: None, lambda t: t.contiguous().float(),
                lambda like, shape=None: (torch.empty_like(like) if shape is None
                                          else torch.empty(tuple(shape), dtype=torch.float32, device=like.device)),
                lambda grad_output, shape, dtype, op: _grad_output(grad_output, shape, op),
                lambda dtype: (), lambda N, C, Ho, Wo: (N, C, Ho, Wo))
_NHWC = _Format("_nhwc", "C a multiple of 64, ", _resident_input, _resident,
                lambda like, shape=None: _resident_empty(like.shape if shape is None else shape, like.dtype, like.device),
                _resident_grad_output, lambda dtype: (_RESIDENT_DTYPES[dtype],), lambda N, C, Ho, Wo: (N, Ho, Wo, C))


def _deform_geometry(x, off, w, stride, padding, dilation, deform_groups):
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    N, Cin, H, W = x.shape
    Cout, Cw, kh, kw = w.shape
    if Cw != Cin:
        raise RuntimeError("invalid number of input planes, expected: %d, but got: %d" % (Cw, Cin))
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    if Ho < 1 or Wo < 1:
        raise ValueError("convolution input is too small (output would be {}x{})".format(Ho, Wo))
    if tuple(off.shape) != (N, deform_groups * 2 * kh * kw, Ho, Wo):
        raise RuntimeError("invalid shape of offset: expected %r, got %r"
                           % ((N, deform_groups * 2 * kh * kw, Ho, Wo), tuple(off.shape)))
    # the C ABI's argument order: N, Cin, H, W, Cout, kW, kH, dW, dH, padW, padH, dilationH, dilationW, G
    return (N, Cin, H, W, Cout, kw, kh, sw, sh, pw, ph, dh, dw, deform_groups), (N, Cout, Ho, Wo)


def _deform_forward(x, off, w, stride, padding, dilation, deform_groups, compute):
    lib = _lib.lib()
    dims, out_shape = _deform_geometry(x, off, w, stride, padding, dilation, deform_groups)
    N, Cin, H, W, Cout, kw, kh, sw, sh, pw, ph, dh, dw, G = dims
    dt = _lib.DTYPES[compute]
    ws, nb = _workspace(lib.tdrn_deform_conv_workspace_bytes, (N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, G, dt), x.device,
                        "deform_conv: shape check failed")
    out = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    _lib.check(lib.tdrn_deform_conv_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(off), _lib.ptr(out), *dims, dt, _lib.ptr(ws), nb,
                                            _lib.current_stream(x.device)), "tdrn_deform_conv_forward")
    return out


class ConvOffset2dFunction(torch.autograd.Function):
    """Deformable conv v1 with gradients (model/networks.py:617-681 of the reference, as a torch.autograd.Function):
    forward through tdrn_deform_conv_forward, backward through tdrn_deform_conv_backward_input (input and offset
    gradients, one call when either is needed) and tdrn_deform_conv_backward_parameters (weight gradient, scale 1 into a
    zeroed buffer).  The backward is fp32 whatever `compute` the forward used (the reference has no 16-bit backward).

        y = ConvOffset2dFunction.apply(input, offset, weight, stride, padding, dilation, deform_groups[, compute])
    """

    @staticmethod
    def forward(ctx, input, offset, weight, stride=1, padding=0, dilation=1, deform_groups=1, compute="fp32"):
        if input.dim() != 4:
            raise ValueError("Expected 4D tensor as input, got {}D tensor instead.".format(input.dim()))
        _lib.require_cuda(input, "input")
        x, off, w = input.contiguous().float(), offset.contiguous().float(), weight.contiguous().float()
        out = _deform_forward(x, off, w, stride, padding, dilation, deform_groups, compute)
        ctx.conf = (stride, padding, dilation, deform_groups)
        ctx.save_for_backward(x, off, w)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        x, off, w = ctx.saved_tensors
        dims, out_shape = _deform_geometry(x, off, w, *ctx.conf)
        go = _grad_output(grad_output, out_shape, "conv_offset2d")
        lib = _lib.lib()
        need_in, need_off, need_w = ctx.needs_input_grad[:3]
        grad_input = grad_offset = grad_weight = None
        if need_in or need_off or need_w:
            N, Cin, H, W, Cout, kw, kh, sw, sh, pw, ph, dh, dw, G = dims
            ws, nb = _workspace(lib.tdrn_deform_conv_backward_workspace_bytes, (N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, G),
                                x.device, "deform_conv backward: shape check failed")
            stream = _lib.current_stream(x.device)
        if need_in or need_off:
            gi = torch.zeros_like(x)
            goff = torch.empty_like(off)
            _lib.check(lib.tdrn_deform_conv_backward_input(_lib.ptr(x), _lib.ptr(off), _lib.ptr(go), _lib.ptr(gi), _lib.ptr(goff),
                                                           _lib.ptr(w), *dims, _lib.ptr(ws), nb, stream),
                       "tdrn_deform_conv_backward_input")
            grad_input = gi if need_in else None
            grad_offset = goff if need_off else None
        if need_w:
            gw = torch.zeros_like(w)
            _lib.check(lib.tdrn_deform_conv_backward_parameters(_lib.ptr(x), _lib.ptr(off), _lib.ptr(go), _lib.ptr(gw), *dims, 1.0,
                                                                _lib.ptr(ws), nb, stream),
                       "tdrn_deform_conv_backward_parameters")
            grad_weight = gw
        return grad_input, grad_offset, grad_weight, None, None, None, None, None


def conv_offset2d(input, offset, weight, stride=1, padding=0, dilation=1, deform_groups=1, compute="fp32"):
    """Deformable conv v1 (replaces the FFI call at model/networks.py:641-645).  NCHW fp32 CUDA tensors in, NCHW fp32
    out, no bias.

    Differentiable exactly when torch.is_grad_enabled() and the input or the offset requires grad (every training use in
    TDRN: the offsets come from a conv): the call then goes through ConvOffset2dFunction and the weight gets its gradient
    as well.  Otherwise the output has no grad_fn -- one difference from the reference, whose Function always records:
    with a constant input and constant offsets and a trainable weight, call ConvOffset2dFunction.apply(...) directly.
    A forward with compute="bf16"/"fp16" gets the fp32 backward of the op."""
    if input is not None and input.dim() != 4:
        raise ValueError("Expected 4D tensor as input, got {}D tensor instead.".format(input.dim()))
    _lib.require_cuda(input, "input")
    return _dispatch(ConvOffset2dFunction, (input, offset, weight, stride, padding, dilation, deform_groups, compute), (input, offset),
                     lambda: _deform_forward(input.contiguous().float(), offset.contiguous().float(), weight.detach().contiguous().float(),
                                             stride, padding, dilation, deform_groups, compute))


_DEFORM_TS_COVERED = ("conv_offset2d_ts covers one deformable group, compute 'bf16' or 'fp16', Cin a multiple of 64, 1 <= Cout <= 256 and "
                      "tensors (input, offset, output, the transform Y of kH*kW*ceil8(Cout) columns per input pixel) below 2^31 elements; "
                      "got input %r, offset %r, weight %r, stride %r, padding %r, dilation %r, compute %r")


def _deform_ts_dims(x, off, w, stride, padding, dilation, compute):
    """the checks of the transform-domain op that need no device, in this order: compute (ValueError), the shapes (_deform_geometry),
    the library's scope (RuntimeError naming what is covered) -> (the C ABI's dims, the output's shape, the workspace's bytes)"""
    if compute not in ("bf16", "fp16"):
        raise ValueError("conv_offset2d_ts: compute must be 'bf16' or 'fp16', got %r (the fp32 op is conv_offset2d)" % (compute,))
    dims, out_shape = _deform_geometry(x, off, w, stride, padding, dilation, 1)
    nb = _lib.lib().tdrn_deform_conv_ts_workspace_bytes(*dims, _lib.DTYPES[compute])
    if nb == 0:
        raise RuntimeError(_DEFORM_TS_COVERED % (tuple(x.shape), tuple(off.shape), tuple(w.shape), stride, padding, dilation, compute))
    return dims, out_shape, nb


def _deform_ts_forward(x, off, w, stride, padding, dilation, compute, save_y):
    """-> (output, Y as a uint8 tensor when save_y else None)"""
    lib = _lib.lib()
    dims, out_shape, nb = _deform_ts_dims(x, off, w, stride, padding, dilation, compute)
    _lib.require_cuda(x, "input")
    dt = _lib.DTYPES[compute]
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    out = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    y = torch.empty(lib.tdrn_deform_conv_ts_y_bytes(*dims, dt), dtype=torch.uint8, device=x.device) if save_y else None
    _lib.check(lib.tdrn_deform_conv_ts_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(off), _lib.ptr(out), _lib.ptr(y), *dims, dt,
                                               _lib.ptr(ws), nb, _lib.current_stream(x.device)), "tdrn_deform_conv_ts_forward")
    return out, y


class ConvOffset2dTsFunction(torch.autograd.Function):
    """Deformable conv v1 with gradients in the transform domain (tdrn_hip.h section i-l): one deformable
    group, compute "bf16" | "fp16".  The forward forms Y = the 1x1 product of the un-deformed input with every tap's weight on MFMA
    and samples rows of Cout values; the backward is ONE call of tdrn_deform_conv_ts_backward, with null pointers for the gradients
    that needs_input_grad does not ask for, in the same compute type.  Saved: input, offset, weight and (save_y, the default) Y;
    save_y = False recomputes Y in the backward, to the same bits.

        y = ConvOffset2dTsFunction.apply(input, offset, weight, stride, padding, dilation[, compute])
    """

    save_y = True

    @staticmethod
    def forward(ctx, input, offset, weight, stride=1, padding=0, dilation=1, compute="bf16"):
        if input.dim() != 4:
            raise ValueError("Expected 4D tensor as input, got {}D tensor instead.".format(input.dim()))
        x, off, w = input.contiguous().float(), offset.contiguous().float(), weight.contiguous().float()
        out, y = _deform_ts_forward(x, off, w, stride, padding, dilation, compute, ConvOffset2dTsFunction.save_y)
        ctx.conf = (stride, padding, dilation, compute)
        ctx.save_for_backward(*((x, off, w) if y is None else (x, off, w, y)))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        x, off, w = ctx.saved_tensors[:3]
        y = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        stride, padding, dilation, compute = ctx.conf
        dims, out_shape, nb = _deform_ts_dims(x, off, w, stride, padding, dilation, compute)
        go = _grad_output(grad_output, out_shape, "conv_offset2d_ts")
        need_in, need_off, need_w = ctx.needs_input_grad[:3]
        if not (need_in or need_off or need_w):
            return (None,) * 7
        lib = _lib.lib()
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        gi = torch.empty_like(x) if need_in else None
        goff = torch.empty_like(off) if need_off else None
        gw = torch.empty_like(w) if need_w else None
        _lib.check(lib.tdrn_deform_conv_ts_backward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(off), _lib.ptr(go), _lib.ptr(y), _lib.ptr(gi),
                                                    _lib.ptr(goff), _lib.ptr(gw), *dims, _lib.DTYPES[compute], _lib.ptr(ws), nb,
                                                    _lib.current_stream(x.device)), "tdrn_deform_conv_ts_backward")
        return gi, goff, gw, None, None, None, None


def conv_offset2d_ts(input, offset, weight, stride=1, padding=0, dilation=1, compute="bf16"):
    """Deformable conv v1, one deformable group, by the transform-then-sample algorithm: an opt-in sibling of conv_offset2d whose
    forward AND backward run in the 16-bit `compute` type ("bf16" | "fp16"; "fp32" raises ValueError), with all Cin-wide arithmetic
    on MFMA.  NCHW fp32 tensors in, NCHW fp32 out, no bias.  The dispatch rule is conv_offset2d's: differentiable exactly when
    torch.is_grad_enabled() and the input or the offset requires grad; otherwise the output has no grad_fn.
    A geometry outside the library's scope raises RuntimeError naming what is covered, CPU tensors raise NotImplementedError: there
    is no fall-back to the gather op.  grad_input and grad_weight come through float atomics (their low bits depend on arrival
    order); the output and grad_offset are bitwise reproducible."""
    if input is not None and input.dim() != 4:
        raise ValueError("Expected 4D tensor as input, got {}D tensor instead.".format(input.dim()))
    return _dispatch(ConvOffset2dTsFunction, (input, offset, weight, stride, padding, dilation, compute), (input, offset),
                     lambda: _deform_ts_forward(input.contiguous().float(), offset.contiguous().float(), weight.detach().contiguous().float(),
                                                stride, padding, dilation, compute, False)[0])


class ConvOffset2d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                 num_deformable_groups=1):
        super(ConvOffset2d, self).__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = _pair(kernel_size), _pair(stride)
        self.padding, self.dilation = _pair(padding), _pair(dilation)
        self.num_deformable_groups = num_deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        nn.init.xavier_uniform_(self.weight)

    def forward(self, input, offset):
        return conv_offset2d(input, offset, self.weight, self.stride, self.padding, self.dilation,
                             self.num_deformable_groups)


# One trainable conv family of the C ABI (tdrn_hip.h sections i-c, i-f, i-g, i-h): `prefix`_workspace_bytes / _forward / _backward_input /
# _backward_parameters.  geometry(x, w, *geo) -> (the ABI's dims, the output's shape); cout_axis: the weight axis that is Cout;
# covered / dim_names: the error message of a geometry the library refuses.  `name` is the op's name in messages.  fmt: the tensor format
# of input, output and their gradients (weight and bias are fp32 in both).
_ConvFamily = collections.namedtuple("_ConvFamily", "name prefix geometry cout_axis covered dim_names fmt", defaults=(_NCHW,))


def _conv2d_family(stride):
    """the C ABI family of a stride: "tdrn_conv2d" (stride 1, section i-c) or "tdrn_conv2d_strided" (stride 2, section i-g)"""
    sh, sw = (int(v) for v in _pair(stride))
    if (sh, sw) == (1, 1):
        return "tdrn_conv2d"
    if (sh, sw) == (2, 2):
        return "tdrn_conv2d_strided"
    raise RuntimeError("conv2d: stride %r is outside what libtdrn_hip covers (%s)" % (stride, _CONV2D_COVERED))


def _conv2d_geometry(x, w, padding, dilation, stride=1):
    (ph, pw), (dh, dw), (sh, sw) = _pair(padding), _pair(dilation), _pair(stride)
    N, Cin, H, W = x.shape
    Cout, Cw, kh, kw = w.shape
    if Cw != Cin:
        raise RuntimeError("invalid number of input planes, expected: %d, but got: %d" % (Cw, Cin))
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    # the C ABI's argument order: N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilationH, dilationW
    return (N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw), (N, Cout, Ho, Wo)


def _conv_transpose2d_geometry(x, w, stride, padding=0, output_padding=0):
    (sh, sw), (ph, pw), (oh, ow) = _pair(stride), _pair(padding), _pair(output_padding)
    N, Cin, H, W = x.shape
    Cw, Cout, kh, kw = w.shape
    if Cw != Cin:
        raise RuntimeError("invalid number of input planes, expected: %d, but got: %d" % (Cw, Cin))
    Ho = (H - 1) * sh - 2 * ph + (kh - 1) + oh + 1
    Wo = (W - 1) * sw - 2 * pw + (kw - 1) + ow + 1
    # the C ABI's argument order: N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, output_padH, output_padW, dilationH, dilationW
    return (N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, oh, ow, 1, 1), (N, Cout, Ho, Wo)


_CONV2D_COVERED = ("square k in {1, 3} at stride 1 with 0 <= pad <= dilation * (k - 1); k = 3 at stride 2 with dilation 1 and "
                   "0 <= pad <= 2")
_CONV2D = {prefix: _ConvFamily("conv2d", prefix, _conv2d_geometry, 0, _CONV2D_COVERED,
                               "N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilH, dilW")
           for prefix in ("tdrn_conv2d", "tdrn_conv2d_strided")}
_CONV_TRANSPOSE2D = _ConvFamily("conv_transpose2d", "tdrn_conv_transpose2d", _conv_transpose2d_geometry, 1,
                                "kernel 2 x 2, stride 2, padding 0, output_padding 0, dilation 1",
                                "N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, opadH, opadW, dilH, dilW")
_CONV2D_NHWC = _ConvFamily("conv2d_nhwc", "tdrn_conv2d_nhwc", _conv2d_geometry, 0,
                           "square k in {1, 3} at stride 1 with 0 <= pad <= dilation * (k - 1), Cin and Cout multiples of 64",
                           "N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilH, dilW", _NHWC)


def _conv2d_require_cuda(input, weight, bias):
    """a module left on the CPU is the likeliest mistake: its parameters must not reach the library as host pointers"""
    _lib.require_cuda(input, "input")
    _lib.require_cuda(weight, "weight")
    if bias is not None:
        _lib.require_cuda(bias, "bias")


def _conv_check(input, weight, bias):
    """what every conv op checks before it touches the library: a 4-D input, everything on the device"""
    if input is not None and input.dim() != 4:
        raise ValueError("Expected 4D tensor as input, got {}D tensor instead.".format(input.dim()))
    _conv2d_require_cuda(input, weight, bias)


def _conv_reset_parameters(weight, bias):
    """nn.Conv2d's default init of an (out, in, kH, kW) weight and its bias (or None)"""
    nn.init.kaiming_uniform_(weight, a=math.sqrt(5))
    if bias is not None:
        fan_in = weight.shape[1] * weight.shape[2] * weight.shape[3]
        bound = 1 / math.sqrt(fan_in) if fan_in > 0 else 0
        nn.init.uniform_(bias, -bound, bound)


def _conv_workspace(lib, fam, dims, dt, extra, device):
    return _workspace(getattr(lib, fam.prefix + "_workspace_bytes"), dims + (dt,) + extra, device,
                      "%s: geometry outside what libtdrn_hip covers (%s): %s = %r", fam.name, fam.covered, fam.dim_names, dims)


def _conv_type(fam, x, compute):
    """the type code of a conv entry: that of a resident input, else the MFMA input type `compute` of an fp32 one"""
    return (fam.fmt.codes(x.dtype) or (_lib.DTYPES[compute],))[0]


def _conv_forward(fam, x, w, b, geo, compute, extra=()):
    """`extra`: the entry arguments a family has behind the stream (conv2d_nhwc's flags)"""
    lib = _lib.lib()
    dims, out_shape = fam.geometry(x, w, *geo)
    if b is not None and tuple(b.shape) != (out_shape[1],):
        raise RuntimeError("%s: bias has shape %r, expected (%d,)" % (fam.name, tuple(b.shape), out_shape[1]))
    dt = _conv_type(fam, x, compute)
    ws, nb = _conv_workspace(lib, fam, dims, dt, extra, x.device)
    out = fam.fmt.empty(x, out_shape)
    _lib.check(getattr(lib, fam.prefix + "_forward")(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(out), *dims, dt, _lib.ptr(ws), nb,
                                                     _lib.current_stream(x.device), *extra), fam.prefix + "_forward")
    return out


def _conv_function_forward(ctx, fam, input, weight, bias, geo, compute, extra=()):
    """the forward of every conv Function, after its checks"""
    x, w = fam.fmt.ready(input), weight.contiguous().float()
    b = None if bias is None else bias.contiguous().float()
    out = _conv_forward(fam, x, w, b, geo, compute, extra)
    ctx.conf = (fam, geo, compute, extra, bias is not None)
    ctx.save_for_backward(x, w)
    return out


def _conv_function_backward(ctx, grad_output):
    """the backward of every conv Function -> (grad_input, grad_weight, grad_bias), each None where it is not needed"""
    x, w = ctx.saved_tensors
    fam, geo, compute, extra, has_bias = ctx.conf
    dims, out_shape = fam.geometry(x, w, *geo)
    go = fam.fmt.grad_output(grad_output, out_shape, x.dtype, fam.name)
    lib = _lib.lib()
    need_in, need_w = ctx.needs_input_grad[:2]
    need_b = has_bias and ctx.needs_input_grad[2]
    grad_input = grad_weight = grad_bias = None
    if need_in or need_w or need_b:
        dt = _conv_type(fam, x, compute)
        ws, nb = _conv_workspace(lib, fam, dims, dt, extra, x.device)
        stream = _lib.current_stream(x.device)
    if need_in:
        grad_input = fam.fmt.empty(x)
        _lib.check(getattr(lib, fam.prefix + "_backward_input")(_lib.ptr(go), _lib.ptr(w), _lib.ptr(grad_input), *dims, dt, _lib.ptr(ws),
                                                                nb, stream, *extra), fam.prefix + "_backward_input")
    if need_w or need_b:
        gw = torch.zeros_like(w)
        gb = torch.zeros(w.shape[fam.cout_axis], dtype=torch.float32, device=x.device) if need_b else None
        _lib.check(getattr(lib, fam.prefix + "_backward_parameters")(_lib.ptr(x), _lib.ptr(go), _lib.ptr(gw), _lib.ptr(gb), *dims, 1.0, dt,
                                                                     _lib.ptr(ws), nb, stream, *extra), fam.prefix + "_backward_parameters")
        grad_weight = gw if need_w else None
        grad_bias = gb
    return grad_input, grad_weight, grad_bias


def _conv_dispatch(function, fam, input, weight, bias, geo, compute, *apply_args, extra=()):
    """_dispatch for a conv family: input, weight and bias count"""
    return _dispatch(function, (input, weight, bias) + apply_args, (input, weight, bias),
                     lambda: _conv_forward(fam, fam.fmt.ready(input.detach()), weight.detach().contiguous().float(),
                                           None if bias is None else bias.detach().contiguous().float(), geo, compute, extra))


class Conv2dFunction(torch.autograd.Function):
    """Dense conv2d with gradients: forward through tdrn_conv2d_forward, backward through
    tdrn_conv2d_backward_input (when the input needs a gradient) and tdrn_conv2d_backward_parameters (weight and bias
    gradients, scale 1 into zeroed buffers).  `compute` ("fp32" | "bf16" | "fp16") is the MFMA input type of the forward and
    of both gradients.  `stride` (an int or a pair) 1 is that family; 2 is the 3x3 family tdrn_conv2d_strided_* with the same three
    entries.  Geometry the library rejects raises; nothing falls back to torch.

        y = Conv2dFunction.apply(input, weight, bias_or_None, padding, dilation[, compute, stride])
    """

    @staticmethod
    def forward(ctx, input, weight, bias=None, padding=0, dilation=1, compute="fp32", stride=1):
        _conv_check(input, weight, bias)
        return _conv_function_forward(ctx, _CONV2D[_conv2d_family(stride)], input, weight, bias, (padding, dilation, stride), compute)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return _conv_function_backward(ctx, grad_output) + (None, None, None, None)


def conv2d(input, weight, bias=None, padding=0, dilation=1, compute="fp32", stride=1):
    """Dense conv2d on libtdrn_hip (NCHW fp32 CUDA tensors in, NCHW fp32 out), differentiable in input, weight and
    bias.  `stride` is an int or a pair: 1, or 2 for a 3x3 kernel at dilation 1 (the `extras` layer of the VGG detectors, the first
    conv of the MobileNet trunk); another stride raises.  With grad mode off, or when nothing requires grad, only the forward runs
    and the output has no grad_fn."""
    fam = _CONV2D[_conv2d_family(stride)]   # a stride the library does not cover raises before anything else
    _conv_check(input, weight, bias)
    return _conv_dispatch(Conv2dFunction, fam, input, weight, bias, (padding, dilation, stride), compute, padding, dilation, compute, stride)


class Conv2d(nn.Module):
    """nn.Conv2d's parameters and default init (weight, bias) on conv2d above: stride 1 or 2 (the last argument), groups 1."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, dilation=1, bias=True, compute="fp32", stride=1):
        super(Conv2d, self).__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.padding, self.dilation, self.stride = _pair(kernel_size), _pair(padding), _pair(dilation), _pair(stride)
        self.compute = compute
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        _conv_reset_parameters(self.weight, self.bias)

    def forward(self, input):
        return conv2d(input, self.weight, self.bias, self.padding, self.dilation, self.compute, self.stride)


def _conv_transpose2d_check(input, weight, bias):
    if weight.dim() != 4:
        raise ValueError("Expected a 4D weight (in_channels, out_channels, kH, kW), got {}D.".format(weight.dim()))
    _conv_check(input, weight, bias)


class ConvTranspose2dFunction(torch.autograd.Function):
    """ConvTranspose2d(kernel 2, stride 2) with gradients: forward through tdrn_conv_transpose2d_forward, backward through
    tdrn_conv_transpose2d_backward_input (when the input needs a gradient) and tdrn_conv_transpose2d_backward_parameters (weight
    and bias gradients, scale 1 into zeroed buffers).  `compute` ("fp32" | "bf16" | "fp16") is the MFMA input type of the forward
    and of both gradients.  The weight is (in_channels, out_channels, 2, 2), torch's layout.  Geometry the library rejects raises;
    nothing falls back to torch.

        y = ConvTranspose2dFunction.apply(input, weight, bias_or_None, stride[, padding, output_padding, compute])
    """

    @staticmethod
    def forward(ctx, input, weight, bias=None, stride=2, padding=0, output_padding=0, compute="fp32"):
        _conv_transpose2d_check(input, weight, bias)
        return _conv_function_forward(ctx, _CONV_TRANSPOSE2D, input, weight, bias, (stride, padding, output_padding), compute)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return _conv_function_backward(ctx, grad_output) + (None, None, None, None)


def _conv_transpose2d(input, weight, bias, stride, padding, output_padding, compute):
    _conv_transpose2d_check(input, weight, bias)
    return _conv_dispatch(ConvTranspose2dFunction, _CONV_TRANSPOSE2D, input, weight, bias, (stride, padding, output_padding), compute,
                          stride, padding, output_padding, compute)


def conv_transpose2d(input, weight, bias=None, stride=2, compute="fp32"):
    """ConvTranspose2d with a 2 x 2 kernel at stride 2 on libtdrn_hip (NCHW fp32 CUDA tensors in, (N, Cout, 2H, 2W) fp32 out; weight
    (Cin, Cout, 2, 2)), differentiable in input, weight and bias.  With grad mode off, or when nothing requires grad, only the
    forward runs and the output has no grad_fn."""
    return _conv_transpose2d(input, weight, bias, stride, 0, 0, compute)


class ConvTranspose2d(nn.Module):
    """nn.ConvTranspose2d's parameters and default init (weight (in, out, kH, kW), bias) on conv_transpose2d above: groups 1,
    dilation 1.  Every geometry can be constructed (a checkpoint loads); one the library does not cover raises in forward."""

    def __init__(self, in_channels, out_channels, kernel_size=2, stride=2, padding=0, output_padding=0, bias=True, compute="fp32"):
        super(ConvTranspose2d, self).__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = _pair(kernel_size), _pair(stride)
        self.padding, self.output_padding = _pair(padding), _pair(output_padding)
        self.compute = compute
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        # nn.ConvTranspose2d's: fan_in is taken from dimension 1 of the weight, the output channels
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in = self.out_channels * self.kernel_size[0] * self.kernel_size[1]
            bound = 1 / math.sqrt(fan_in) if fan_in > 0 else 0
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, input):
        return _conv_transpose2d(input, self.weight, self.bias, self.stride, self.padding, self.output_padding, self.compute)


def _depthwise_geometry(x, w, stride, padding):
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    N, Ch, H, W = x.shape
    if w.dim() != 4 or w.shape[0] != Ch or w.shape[1] != 1:
        raise RuntimeError("depthwise_conv2d: weight has shape %r, expected (%d, 1, kH, kW) for an input of %d channels"
                           % (tuple(w.shape), Ch, Ch))
    kh, kw = w.shape[2:]
    Ho = (H + 2 * ph - kh) // sh + 1
    Wo = (W + 2 * pw - kw) // sw + 1
    # the C ABI's argument order: N, C, H, W, kH, kW, dH, dW, padH, padW, dilationH, dilationW
    return (N, Ch, H, W, kh, kw, sh, sw, ph, pw, 1, 1), (N, Ch, Ho, Wo)


_DEPTHWISE = _ConvFamily("depthwise_conv2d", "tdrn_dwconv2d", _depthwise_geometry, 0,
                         "kernel 3 x 3, stride 1 or 2, padding 1, dilation 1, channel multiplier 1, fewer than 2^31 elements",
                         "N, C, H, W, kH, kW, dH, dW, padH, padW, dilH, dilW")


class DepthwiseConv2dFunction(torch.autograd.Function):
    """Depthwise 3x3 conv (groups = channels, pad 1, stride 1 or 2) with gradients: forward through tdrn_dwconv2d_forward, backward
    through tdrn_dwconv2d_backward_input (when the input needs a gradient) and tdrn_dwconv2d_backward_parameters (weight and bias
    gradients, scale 1 into zeroed buffers).  fp32 throughout: the op has no 16-bit mode.  The weight is (channels, 1, 3, 3), torch's
    layout.  Geometry the library rejects raises; nothing falls back to torch.

        y = DepthwiseConv2dFunction.apply(input, weight, bias_or_None, stride, padding)
    """

    @staticmethod
    def forward(ctx, input, weight, bias=None, stride=1, padding=1):
        _conv_check(input, weight, bias)
        return _conv_function_forward(ctx, _DEPTHWISE, input, weight, bias, (stride, padding), "fp32")

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return _conv_function_backward(ctx, grad_output) + (None, None)


def depthwise_conv2d(input, weight, bias=None, stride=1, padding=1):
    """F.conv2d(input, weight, bias, stride, padding, groups=channels) for a (channels, 1, 3, 3) weight on libtdrn_hip (NCHW fp32 CUDA
    tensors in, NCHW fp32 out), differentiable in input, weight and bias: the depthwise conv of conv_dw.  `stride` is 1 or 2,
    `padding` 1; anything else raises.  With grad mode off, or when nothing requires grad, only the forward runs and the output has
    no grad_fn."""
    _conv_check(input, weight, bias)
    return _conv_dispatch(DepthwiseConv2dFunction, _DEPTHWISE, input, weight, bias, (stride, padding), "fp32", stride, padding)


class DepthwiseConv2d(nn.Module):
    """The parameters, state-dict keys and default init of nn.Conv2d(channels, channels, 3, stride, 1, groups=channels) on
    depthwise_conv2d above."""

    def __init__(self, channels, stride=1, bias=False):
        super(DepthwiseConv2d, self).__init__()
        self.channels, self.stride, self.padding = channels, _pair(stride), (1, 1)
        self.weight = nn.Parameter(torch.empty(channels, 1, 3, 3))
        self.bias = nn.Parameter(torch.empty(channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            nn.init.uniform_(self.bias, -1.0 / 3, 1.0 / 3)          # 1 / sqrt(fan_in), fan_in = 9

    def forward(self, input):
        return depthwise_conv2d(input, self.weight, self.bias, self.stride, self.padding)

    def extra_repr(self):
        return "{channels}, stride={stride}, bias={0}".format(self.bias is not None, **self.__dict__)


_CONV5X5_COVERED = "kernel 5 x 5, stride 1, padding 2, dilation 1, groups 1"


def _conv5x5_geometry(x, w):
    if w.dim() != 4 or tuple(w.shape[2:]) != (5, 5):
        raise RuntimeError("conv5x5: weight has shape %r, expected (Cout, Cin, 5, 5); libtdrn_hip covers %s"
                           % (tuple(w.shape), _CONV5X5_COVERED))
    return _conv2d_geometry(x, w, 2, 1, 1)


_CONV5X5 = _ConvFamily("conv5x5", "tdrn_conv5x5", _conv5x5_geometry, 0, _CONV5X5_COVERED,
                       "N, Cin, H, W, Cout, kH, kW, dH, dW, padH, padW, dilH, dilW")


class Conv5x5Function(torch.autograd.Function):
    """Dense 5x5 conv (pad 2, stride 1) with gradients: forward through tdrn_conv5x5_forward, backward through
    tdrn_conv5x5_backward_input (when the input needs a gradient) and tdrn_conv5x5_backward_parameters (weight and bias gradients,
    scale 1 into zeroed buffers).  `compute` ("fp32" | "bf16" | "fp16") is the MFMA input type of the forward and of both
    gradients.  Another weight shape raises; nothing falls back to torch.

        y = Conv5x5Function.apply(input, weight, bias_or_None[, compute])
    """

    @staticmethod
    def forward(ctx, input, weight, bias=None, compute="fp32"):
        _conv_check(input, weight, bias)
        return _conv_function_forward(ctx, _CONV5X5, input, weight, bias, (), compute)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return _conv_function_backward(ctx, grad_output) + (None,)


def conv5x5(input, weight, bias=None, compute="fp32"):
    """F.conv2d(input, weight, bias, padding=2) for a (Cout, Cin, 5, 5) weight on libtdrn_hip (NCHW fp32 CUDA tensors in, NCHW fp32
    out), differentiable in input, weight and bias: the second ODM heads of refinedet_vgg's multihead.  With grad mode off, or when
    nothing requires grad, only the forward runs and the output has no grad_fn."""
    _conv_check(input, weight, bias)
    return _conv_dispatch(Conv5x5Function, _CONV5X5, input, weight, bias, (), compute, compute)


class Conv5x5(nn.Module):
    """The parameters, state-dict keys and default init of nn.Conv2d(in_channels, out_channels, 5, padding=2) on conv5x5 above."""

    def __init__(self, in_channels, out_channels, bias=True, compute="fp32"):
        super(Conv5x5, self).__init__()
        self.in_channels, self.out_channels, self.compute = in_channels, out_channels, compute
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 5, 5))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        _conv_reset_parameters(self.weight, self.bias)

    def forward(self, input):
        return conv5x5(input, self.weight, self.bias, self.compute)

    def extra_repr(self):
        return "{in_channels}, {out_channels}, bias={0}, compute={compute}".format(self.bias is not None, **self.__dict__)


def _batch_norm_check(input, running_mean, running_var, weight, bias, training):
    if input.dim() != 4:
        raise ValueError("expected 4D input (got {}D input)".format(input.dim()))
    _lib.require_cuda(input, "input")
    for name, t in (("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var)):
        if t is None:
            if name in ("weight", "bias") or not training:
                raise ValueError("batch_norm: %s is required%s" % (name, "" if training else " when training is False"))
            continue
        _lib.require_cuda(t, name)          # a module left on the CPU must not reach the library as host pointers
        if tuple(t.shape) != (input.shape[1],):
            raise RuntimeError("batch_norm: %s has shape %r, expected (%d,)" % (name, tuple(t.shape), input.shape[1]))
    if (running_mean is None) != (running_var is None):
        raise ValueError("batch_norm: running_mean and running_var come as a pair")
    for name, t in (("running_mean", running_mean), ("running_var", running_var)):
        # they are updated in place through their address: a copy would take the update with it
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("batch_norm: %s must be a contiguous float32 tensor" % name)
    if training and input.numel() == input.shape[1]:
        raise ValueError("Expected more than 1 value per channel when training, got input size {}".format(input.size()))


def _batch_norm_workspace(fmt, lib, dims, device):
    return _workspace(getattr(lib, "tdrn_batch_norm%s_workspace_bytes" % fmt.infix), dims, device,
                      "batch_norm%s: shape outside what libtdrn_hip covers (positive sizes, %sfewer than 2^31 elements): N, C, H, W = %r",
                      fmt.infix, fmt.covered, dims)


def _batch_norm_forward(fmt, x, running_mean, running_var, w, b, training, momentum, eps, relu):
    lib = _lib.lib()
    dims = tuple(x.shape)
    ws, nb = _batch_norm_workspace(fmt, lib, dims, x.device)
    out = fmt.empty(x)
    save_mean = torch.empty(dims[1], dtype=torch.float32, device=x.device)
    save_invstd = torch.empty_like(save_mean)
    entry = "tdrn_batch_norm%s_forward" % fmt.infix
    _lib.check(getattr(lib, entry)(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(running_mean), _lib.ptr(running_var), _lib.ptr(out),
                                   _lib.ptr(save_mean), _lib.ptr(save_invstd), *dims, int(bool(training)), float(momentum), float(eps),
                                   int(bool(relu)), *fmt.codes(x.dtype), _lib.ptr(ws), nb, _lib.current_stream(x.device)), entry)
    return out, save_mean, save_invstd


def _batch_norm_function_forward(ctx, fmt, input, running_mean, running_var, weight, bias, training, momentum, eps, relu):
    """the forward of both batch norm Functions"""
    fmt.check(input, "batch_norm" + fmt.infix)
    _batch_norm_check(input, running_mean, running_var, weight, bias, training)
    x, w, b = fmt.ready(input), weight.contiguous().float(), bias.contiguous().float()
    out, save_mean, save_invstd = _batch_norm_forward(fmt, x, running_mean, running_var, w, b, training, momentum, eps, relu)
    ctx.conf = (bool(training), bool(relu))
    ctx.save_for_backward(x, w, b, save_mean, save_invstd)
    return out


def _batch_norm_function_backward(ctx, fmt, grad_output):
    """the backward of both batch norm Functions"""
    x, w, b, save_mean, save_invstd = ctx.saved_tensors
    go = fmt.grad_output(grad_output, x.shape, x.dtype, "batch_norm" + fmt.infix)
    training, relu = ctx.conf
    need_in, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[3], ctx.needs_input_grad[4]
    grad_input = gw = gb = None
    if need_in or need_w or need_b:
        lib = _lib.lib()
        dims = tuple(x.shape)
        ws, nb = _batch_norm_workspace(fmt, lib, dims, x.device)
        if need_in:
            grad_input = fmt.empty(x)
        if need_w or need_b:
            gw, gb = torch.zeros_like(w), torch.zeros_like(b)
        entry = "tdrn_batch_norm%s_backward" % fmt.infix
        _lib.check(getattr(lib, entry)(_lib.ptr(x), _lib.ptr(go), _lib.ptr(w), _lib.ptr(b), _lib.ptr(save_mean), _lib.ptr(save_invstd),
                                       _lib.ptr(grad_input), _lib.ptr(gw), _lib.ptr(gb), *dims, int(training), int(relu), 1.0,
                                       *fmt.codes(x.dtype), _lib.ptr(ws), nb, _lib.current_stream(x.device)), entry)
    return grad_input, None, None, gw if need_w else None, gb if need_b else None, None, None, None, None


def _batch_norm(fmt, function, input, running_mean, running_var, weight, bias, training, momentum, eps, relu):
    """batch_norm and batch_norm_nhwc: the checks, then _dispatch; input, weight and bias count"""
    fmt.check(input, "batch_norm" + fmt.infix)
    _batch_norm_check(input, running_mean, running_var, weight, bias, training)
    return _dispatch(function, (input, running_mean, running_var, weight, bias, training, momentum, eps, relu), (input, weight, bias),
                     lambda: _batch_norm_forward(fmt, fmt.ready(input.detach()), running_mean, running_var, weight.detach().contiguous().float(),
                                                 bias.detach().contiguous().float(), training, momentum, eps, relu)[0])


class BatchNormFunction(torch.autograd.Function):
    """BatchNorm2d with an optional fused ReLU and gradients: forward through tdrn_batch_norm_forward, backward through
    tdrn_batch_norm_backward (scale 1 into zeroed parameter gradients; only what needs_input_grad asks for is computed).  Saves
    the input and the statistics, no ReLU output and no mask: the backward recomputes the mask from the input.  The running
    buffers (or None, in training) are updated in place.

        y = BatchNormFunction.apply(input, running_mean, running_var, weight, bias, training, momentum, eps, relu)
    """

    @staticmethod
    def forward(ctx, input, running_mean, running_var, weight, bias, training=True, momentum=0.1, eps=1e-5, relu=False):
        return _batch_norm_function_forward(ctx, _NCHW, input, running_mean, running_var, weight, bias, training, momentum, eps, relu)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return _batch_norm_function_backward(ctx, _NCHW, grad_output)


def batch_norm(input, running_mean, running_var, weight, bias, training, momentum=0.1, eps=1e-5, relu=False):
    """F.batch_norm for NCHW fp32 CUDA tensors on libtdrn_hip, with `relu=True` fusing the ReLU behind it; differentiable in input,
    weight and bias.  In training the running buffers (float32, contiguous; or both None) are updated in place with `momentum`,
    nn.BatchNorm2d's semantics.  With grad mode off, or when nothing requires grad, only the forward runs and the output has no
    grad_fn."""
    return _batch_norm(_NCHW, BatchNormFunction, input, running_mean, running_var, weight, bias, training, momentum, eps, relu)


class BatchNormNhwcFunction(torch.autograd.Function):
    """BatchNormFunction on resident tensors: tdrn_batch_norm_nhwc_forward / _backward.  Saves the 16-bit input and the fp32
    statistics; the backward recomputes the ReLU mask from the input.

        y = BatchNormNhwcFunction.apply(input, running_mean, running_var, weight, bias, training, momentum, eps, relu)
    """

    @staticmethod
    def forward(ctx, input, running_mean, running_var, weight, bias, training=True, momentum=0.1, eps=1e-5, relu=False):
        return _batch_norm_function_forward(ctx, _NHWC, input, running_mean, running_var, weight, bias, training, momentum, eps, relu)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return _batch_norm_function_backward(ctx, _NHWC, grad_output)


def batch_norm_nhwc(input, running_mean, running_var, weight, bias, training, momentum=0.1, eps=1e-5, relu=False):
    """batch_norm above from a resident tensor to a resident tensor: the same semantics, fp32 parameters, buffers and statistics,
    the output rounded once to the input's dtype.  With grad mode off, or when nothing requires grad, only the forward runs and the
    output has no grad_fn."""
    return _batch_norm(_NHWC, BatchNormNhwcFunction, input, running_mean, running_var, weight, bias, training, momentum, eps, relu)


class BatchNorm2d(nn.Module):
    """nn.BatchNorm2d's parameters, buffers, state_dict keys and default init on batch_norm above, with `relu=True` fusing the
    nn.ReLU that follows it in the reference's nets.  Always affine, always tracking running statistics.  `momentum=None` is the
    cumulative average; its factor 1 / num_batches_tracked comes from a host-side count, never from a device read."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, relu=False):
        super(BatchNorm2d, self).__init__()
        self.num_features, self.eps, self.momentum, self.relu = num_features, eps, momentum, relu
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self._batches = 0        # num_batches_tracked as the host knows it

    def reset_running_stats(self):
        self.running_mean.zero_()
        self.running_var.fill_(1)
        self.num_batches_tracked.zero_()
        self._batches = 0

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super(BatchNorm2d, self)._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        key = prefix + "num_batches_tracked"
        if key in state_dict:
            self._batches = int(state_dict[key])        # at load time, off the training path

    def forward(self, input):
        factor = 0.0 if self.momentum is None else self.momentum
        if self.training:
            # checked before the count moves: a refused call is no tracked batch
            _batch_norm_check(input, self.running_mean, self.running_var, self.weight, self.bias, True)
            self.num_batches_tracked.add_(1)
            self._batches += 1
            if self.momentum is None:
                factor = 1.0 / self._batches
        return batch_norm(input, self.running_mean, self.running_var, self.weight, self.bias, self.training, factor, self.eps,
                          self.relu)

    def extra_repr(self):
        return "{num_features}, eps={eps}, momentum={momentum}, relu={relu}".format(**self.__dict__)


_POOL_GEOMETRIES = "kernel_size 2, stride 2, padding 0 (ceil_mode False or True) and kernel_size 3, stride 1, padding 1"


def _square(v, name):
    a, b = _pair(v)
    if a != b:
        raise NotImplementedError("max_pool2d: %s %r is not square; libtdrn_hip covers %s" % (name, v, _POOL_GEOMETRIES))
    return int(a)


def _max_pool_check(fmt, input, kernel_size, stride, padding, ceil_mode):
    """-> (kernel, stride, pad, ceil, Ho, Wo) + the format's type codes, of a call the library covers"""
    op = "max_pool2d" + fmt.infix
    fmt.check(input, op)
    if input.dim() != 4:
        raise ValueError("expected 4D input (got {}D input)".format(input.dim()))
    if fmt is _NCHW and input.dtype != torch.float32:          # the fp32 op casts nothing; a resident input's type is settled above
        raise ValueError("max_pool2d: input must be float32 (got %s)" % input.dtype)
    _lib.require_cuda(input, "input")
    k = _square(kernel_size, "kernel_size")
    geo = (k, k if stride is None else _square(stride, "stride"), _square(padding, "padding"), int(bool(ceil_mode)))
    lib = _lib.lib()
    Ho, Wo = (lib.tdrn_max_pool_output_size(int(n), *geo) for n in input.shape[2:])
    if geo[:3] not in ((2, 2, 0), (3, 1, 1)):
        raise NotImplementedError("%s: kernel_size %d, stride %d, padding %d is not covered; libtdrn_hip covers %s"
                                  % (op, geo[0], geo[1], geo[2], _POOL_GEOMETRIES))
    if Ho == 0 or Wo == 0 or input.numel() == 0:
        raise RuntimeError("%s: input %r gives an empty output" % (op, tuple(input.shape)))
    return geo + (Ho, Wo) + fmt.codes(input.dtype)


def _max_pool_forward(fmt, x, conf, with_code):
    k, s, p, ceil, Ho, Wo, *codes = conf
    N, Ch, H, W = x.shape
    out = fmt.empty(x, (N, Ch, Ho, Wo))
    code = torch.empty(fmt.code_shape(N, Ch, Ho, Wo), dtype=torch.uint8, device=x.device) if with_code else None
    entry = "tdrn_max_pool%s_forward" % fmt.infix
    _lib.check(getattr(_lib.lib(), entry)(_lib.ptr(x), _lib.ptr(out), _lib.ptr(code), N, Ch, H, W, k, s, p, ceil, *codes,
                                          _lib.current_stream(x.device)), entry)
    return out, code


def _max_pool_function_forward(ctx, fmt, input, kernel_size, stride, padding, ceil_mode):
    """the forward of both max pool Functions"""
    conf = _max_pool_check(fmt, input, kernel_size, stride, padding, ceil_mode)
    x = fmt.ready(input)            # fp32: checked to be float32, so contiguous() and no cast
    out, code = _max_pool_forward(fmt, x, conf, True)
    ctx.conf, ctx.in_shape, ctx.dtype = conf, tuple(x.shape), x.dtype
    ctx.save_for_backward(code)
    return out


def _max_pool_function_backward(ctx, fmt, grad_output):
    """the backward of both max pool Functions"""
    code, = ctx.saved_tensors
    k, s, p, ceil, Ho, Wo, *codes = ctx.conf
    N, Ch, H, W = ctx.in_shape
    go = fmt.grad_output(grad_output, (N, Ch, Ho, Wo), ctx.dtype, "max_pool2d" + fmt.infix)
    grad_input = None
    if ctx.needs_input_grad[0]:
        grad_input = fmt.empty(go, ctx.in_shape)
        entry = "tdrn_max_pool%s_backward" % fmt.infix
        _lib.check(getattr(_lib.lib(), entry)(_lib.ptr(go), _lib.ptr(code), _lib.ptr(grad_input), N, Ch, H, W, k, s, p, ceil, *codes,
                                              _lib.current_stream(go.device)), entry)
    return grad_input, None, None, None, None


def _max_pool2d(fmt, function, input, kernel_size, stride, padding, ceil_mode):
    """max_pool2d and max_pool2d_nhwc: the check, then _dispatch; the input alone counts"""
    conf = _max_pool_check(fmt, input, kernel_size, stride, padding, ceil_mode)
    return _dispatch(function, (input, kernel_size, stride, padding, ceil_mode), (input,),
                     lambda: _max_pool_forward(fmt, fmt.ready(input.detach()), conf, False)[0])


class MaxPool2dFunction(torch.autograd.Function):
    """MaxPool2d with a gradient: forward through tdrn_max_pool_forward, backward through tdrn_max_pool_backward.  Saves one uint8
    code per output element (the selected slot of the window), not the input and no int64 indices.

        y = MaxPool2dFunction.apply(input, kernel_size, stride, padding, ceil_mode)
    """

    @staticmethod
    def forward(ctx, input, kernel_size, stride=None, padding=0, ceil_mode=False):
        return _max_pool_function_forward(ctx, _NCHW, input, kernel_size, stride, padding, ceil_mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return _max_pool_function_backward(ctx, _NCHW, grad_output)


def max_pool2d(input, kernel_size, stride=None, padding=0, ceil_mode=False):
    """F.max_pool2d for NCHW fp32 CUDA tensors on libtdrn_hip, differentiable in input, for the geometries of vgg(): 2 / 2 / 0 with
    either ceil_mode, and 3 / 1 / 1.  With grad mode off, or an input that does not require grad, only the forward runs, no code
    tensor is made and the output has no grad_fn."""
    return _max_pool2d(_NCHW, MaxPool2dFunction, input, kernel_size, stride, padding, ceil_mode)


class MaxPool2dNhwcFunction(torch.autograd.Function):
    """MaxPool2dFunction on resident tensors: tdrn_max_pool_nhwc_forward / _backward.  Saves one uint8 code per output element,
    (N, Ho, Wo, C).

        y = MaxPool2dNhwcFunction.apply(input, kernel_size, stride, padding, ceil_mode)
    """

    @staticmethod
    def forward(ctx, input, kernel_size, stride=None, padding=0, ceil_mode=False):
        return _max_pool_function_forward(ctx, _NHWC, input, kernel_size, stride, padding, ceil_mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return _max_pool_function_backward(ctx, _NHWC, grad_output)


def max_pool2d_nhwc(input, kernel_size, stride=None, padding=0, ceil_mode=False):
    """max_pool2d above from a resident tensor to a resident tensor: the same three geometries, the same selection.  With grad mode
    off, or an input that does not require grad, only the forward runs, no code tensor is made and the output has no grad_fn."""
    return _max_pool2d(_NHWC, MaxPool2dNhwcFunction, input, kernel_size, stride, padding, ceil_mode)


class MaxPool2d(nn.Module):
    """nn.MaxPool2d's constructor arguments (without dilation and return_indices) on max_pool2d above; no state."""

    def __init__(self, kernel_size, stride=None, padding=0, ceil_mode=False):
        super(MaxPool2d, self).__init__()
        self.kernel_size, self.stride, self.padding, self.ceil_mode = kernel_size, kernel_size if stride is None else stride, padding, ceil_mode

    def forward(self, input):
        return max_pool2d(input, self.kernel_size, self.stride, self.padding, self.ceil_mode)

    def extra_repr(self):
        return "kernel_size={kernel_size}, stride={stride}, padding={padding}, ceil_mode={ceil_mode}".format(**self.__dict__)


def _l2norm_check(input, weight, eps):
    if input.dim() != 4:
        raise ValueError("expected 4D input (got {}D input)".format(input.dim()))
    if input.dtype != torch.float32 or weight.dtype != torch.float32:
        raise ValueError("l2norm: input and weight must be float32 (got %s, %s)" % (input.dtype, weight.dtype))
    _lib.require_cuda(input, "input")
    _lib.require_cuda(weight, "weight")         # a module left on the CPU must not reach the library as host pointers
    if tuple(weight.shape) != (input.shape[1],):
        raise RuntimeError("l2norm: weight has shape %r, expected (%d,)" % (tuple(weight.shape), input.shape[1]))
    if not eps > 0:
        raise ValueError("l2norm: eps must be positive")
    if input.numel() == 0 or input.numel() >= 2 ** 31:
        raise RuntimeError("l2norm: shape outside what libtdrn_hip covers (positive sizes, fewer than 2^31 elements): %r"
                           % (tuple(input.shape),))


def _l2norm_forward(x, w, eps, with_norm):
    N, Ch, H, W = x.shape
    out = torch.empty_like(x)
    norm = torch.empty((N, H, W), dtype=torch.float32, device=x.device) if with_norm else None
    _lib.check(_lib.lib().tdrn_l2norm_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(out), _lib.ptr(norm), N, Ch, H, W, float(eps),
                                              _lib.current_stream(x.device)), "tdrn_l2norm_forward")
    return out, norm


class L2NormFunction(torch.autograd.Function):
    """weight x / (sqrt(sum_c x^2) + eps) with gradients: forward through tdrn_l2norm_forward, backward through tdrn_l2norm_backward
    (scale 1 into a zeroed grad_weight; only what needs_input_grad asks for is computed).  Saves the input, the weight and the
    per-pixel norm.  At an all-zero pixel the input gradient is weight grad_output / eps, where torch's autograd gives NaN.

        y = L2NormFunction.apply(input, weight, eps)
    """

    @staticmethod
    def forward(ctx, input, weight, eps=1e-10):
        _l2norm_check(input, weight, eps)
        x, w = input.contiguous(), weight.contiguous()
        out, norm = _l2norm_forward(x, w, eps, True)
        ctx.eps = float(eps)
        ctx.save_for_backward(x, w, norm)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        x, w, norm = ctx.saved_tensors
        go = _grad_output(grad_output, x.shape, "l2norm")
        need_in, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        grad_input = gw = None
        if need_in or need_w:
            lib = _lib.lib()
            dims = tuple(x.shape)
            ws, nb = None, 0
            if need_in:
                grad_input = torch.empty_like(x)
            if need_w:
                gw = torch.zeros_like(w)
                nb = lib.tdrn_l2norm_workspace_bytes(*dims)
                ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
            _lib.check(lib.tdrn_l2norm_backward(_lib.ptr(x), _lib.ptr(go), _lib.ptr(w), _lib.ptr(norm), _lib.ptr(grad_input), _lib.ptr(gw),
                                                *dims, ctx.eps, 1.0, _lib.ptr(ws), nb, _lib.current_stream(x.device)),
                       "tdrn_l2norm_backward")
        return grad_input, gw, None


def l2norm(input, weight, eps=1e-10):
    """The reference's L2Norm (layers/modules/l2norm.py) for NCHW fp32 CUDA tensors on libtdrn_hip, differentiable in input and
    weight.  With grad mode off, or when nothing requires grad, only the forward runs, no norm tensor is made and the output has
    no grad_fn."""
    _l2norm_check(input, weight, eps)
    return _dispatch(L2NormFunction, (input, weight, eps), (input, weight),
                     lambda: _l2norm_forward(input.detach().contiguous(), weight.detach().contiguous(), eps, False)[0])


class L2Norm(nn.Module):
    """The reference module's single `weight` key and init (layers/modules/l2norm.py: every channel starts at `scale`) on l2norm
    above."""

    def __init__(self, n_channels, scale):
        super(L2Norm, self).__init__()
        self.n_channels, self.gamma, self.eps = n_channels, scale or None, 1e-10
        self.weight = nn.Parameter(torch.full((n_channels,), float(scale)))

    def forward(self, x):
        return l2norm(x, self.weight, self.eps)


# ---- the resident ops that have no fp32 NCHW twin: into the format and out of it, and the conv family on it -------------------------------
def _to_nhwc_forward(x, dtype):
    out = _resident_empty(x.shape, dtype, x.device)
    _lib.check(_lib.lib().tdrn_nhwc16_from_nchw(_lib.ptr(x), _lib.ptr(out), *x.shape, _RESIDENT_DTYPES[dtype],
                                                _lib.current_stream(x.device)), "tdrn_nhwc16_from_nchw")
    return out


def _from_nhwc_forward(x):
    out = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().tdrn_nchw_from_nhwc16(_lib.ptr(x), _lib.ptr(out), *x.shape, _RESIDENT_DTYPES[x.dtype],
                                                _lib.current_stream(x.device)), "tdrn_nchw_from_nhwc16")
    return out


class ToNhwcFunction(torch.autograd.Function):
    """fp32 NCHW -> resident (tdrn_nhwc16_from_nchw); the backward is from_nhwc's forward."""

    @staticmethod
    def forward(ctx, input, dtype):
        ctx.dtype = dtype
        return _to_nhwc_forward(input.contiguous().float(), dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return _from_nhwc_forward(_resident_grad_output(grad_output, grad_output.shape, ctx.dtype, "to_nhwc")), None


class FromNhwcFunction(torch.autograd.Function):
    """resident -> fp32 NCHW (tdrn_nchw_from_nhwc16); the backward is to_nhwc's forward in the input's type."""

    @staticmethod
    def forward(ctx, input):
        ctx.dtype = input.dtype
        return _from_nhwc_forward(_resident(input))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return _to_nhwc_forward(_grad_output(grad_output, grad_output.shape, "from_nhwc"), ctx.dtype)


def to_nhwc(x, dtype):
    """An NCHW CUDA tensor (C a multiple of 64) -> the resident tensor of the same values, each rounded once to `dtype`
    (torch.bfloat16 / torch.float16 or "bf16" / "fp16"): logical shape (N, C, H, W), contiguous in channels_last.  Bit for bit
    x.to(dtype).contiguous(memory_format=torch.channels_last); differentiable (the gradient comes back as fp32 NCHW)."""
    dtype = _resident_dtype(dtype)
    if x.dim() != 4:
        raise ValueError("Expected 4D tensor as input, got {}D tensor instead.".format(x.dim()))
    _lib.require_cuda(x, "input")
    if x.shape[1] % RESIDENT_CHANNELS:
        raise RuntimeError("to_nhwc: %d channels are outside what libtdrn_hip covers (a multiple of %d)" % (x.shape[1], RESIDENT_CHANNELS))
    return _dispatch(ToNhwcFunction, (x, dtype), (x,), lambda: _to_nhwc_forward(x.detach().contiguous().float(), dtype))


def from_nhwc(x):
    """A resident tensor -> the same values as fp32 NCHW (exact); differentiable (the gradient is rounded once to x's type)."""
    _resident_input(x, "from_nhwc")
    return _dispatch(FromNhwcFunction, (x,), (x,), lambda: _from_nhwc_forward(_resident(x.detach())))


class Conv2dNhwcFunction(torch.autograd.Function):
    """Dense stride-1 conv2d on resident tensors with gradients: tdrn_conv2d_nhwc_forward / _backward_input / _backward_parameters
    (scale 1 into zeroed fp32 buffers).  The compute type is the input's dtype; weight and bias stay fp32.

        y = Conv2dNhwcFunction.apply(input, weight, bias_or_None, padding, dilation[, flags])
    """

    @staticmethod
    def forward(ctx, input, weight, bias=None, padding=0, dilation=1, flags=0):
        _resident_input(input, "conv2d_nhwc")
        _conv2d_require_cuda(input, weight, bias)
        return _conv_function_forward(ctx, _CONV2D_NHWC, input, weight, bias, (padding, dilation), None, (flags,))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return _conv_function_backward(ctx, grad_output) + (None, None, None)


def conv2d_nhwc(input, weight, bias=None, padding=0, dilation=1, flags=0):
    """Dense stride-1 conv2d on libtdrn_hip from a resident tensor to a resident tensor (to_nhwc), differentiable in input, weight and
    bias; weight (OIHW) and bias are fp32.  The compute type is the input's dtype.  `flags`: _lib.CONV_NHWC_IGEMM_ONLY keeps the
    launches on the generic implicit GEMM (for comparison: bit-equal only for one 64-channel chunk and no bias, otherwise equal up to
    one rounding of the result; tdrn_hip.h section i-k).  Geometry the library rejects raises; nothing falls back to torch.  With
    grad mode off, or when nothing requires grad, only the forward runs and the output has no grad_fn."""
    _resident_input(input, "conv2d_nhwc")
    _conv2d_require_cuda(input, weight, bias)
    return _conv_dispatch(Conv2dNhwcFunction, _CONV2D_NHWC, input, weight, bias, (padding, dilation), None, padding, dilation, flags,
                          extra=(flags,))
