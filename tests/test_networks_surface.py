"""The public surface of tdrn_amd.model.networks, pinned with literals, no GPU needed: the signature of every public function, of
every autograd Function's forward, of every Module's constructor, and the names of the classes.  The shared bodies behind the ops
(`_ConvFamily`, `_Format`, `_dispatch`) may be rearranged; what a caller writes may not change.  The literals
are written out here, not computed from the module."""
import inspect

import torch

from tdrn_amd.model import networks

BATCH_NORM = "(input, running_mean, running_var, weight, bias, training, momentum=0.1, eps=1e-05, relu=False)"
MAX_POOL = "(input, kernel_size, stride=None, padding=0, ceil_mode=False)"
FUNCTIONS = {
    "vgg": "(cfg, i, batch_norm=False, pool5_ds=False, c7_channel=1024)",
    "conv_dw": "(inp, oup, stride)",
    "mobilenet_backbone": "(c_last=1024)",
    "conv_offset2d": "(input, offset, weight, stride=1, padding=0, dilation=1, deform_groups=1, compute='fp32')",
    "conv_offset2d_ts": "(input, offset, weight, stride=1, padding=0, dilation=1, compute='bf16')",
    "conv2d": "(input, weight, bias=None, padding=0, dilation=1, compute='fp32', stride=1)",
    "conv_transpose2d": "(input, weight, bias=None, stride=2, compute='fp32')",
    "depthwise_conv2d": "(input, weight, bias=None, stride=1, padding=1)",
    "conv5x5": "(input, weight, bias=None, compute='fp32')",
    "batch_norm": BATCH_NORM,
    "max_pool2d": MAX_POOL,
    "l2norm": "(input, weight, eps=1e-10)",
    "to_nhwc": "(x, dtype)",
    "from_nhwc": "(x)",
    "conv2d_nhwc": "(input, weight, bias=None, padding=0, dilation=1, flags=0)",
    "batch_norm_nhwc": BATCH_NORM,
    "max_pool2d_nhwc": MAX_POOL,
}
BATCH_NORM_FORWARD = "(ctx, input, running_mean, running_var, weight, bias, training=True, momentum=0.1, eps=1e-05, relu=False)"
MAX_POOL_FORWARD = "(ctx, input, kernel_size, stride=None, padding=0, ceil_mode=False)"
FORWARDS = {
    "ConvOffset2dFunction": "(ctx, input, offset, weight, stride=1, padding=0, dilation=1, deform_groups=1, compute='fp32')",
    "ConvOffset2dTsFunction": "(ctx, input, offset, weight, stride=1, padding=0, dilation=1, compute='bf16')",
    "Conv2dFunction": "(ctx, input, weight, bias=None, padding=0, dilation=1, compute='fp32', stride=1)",
    "ConvTranspose2dFunction": "(ctx, input, weight, bias=None, stride=2, padding=0, output_padding=0, compute='fp32')",
    "DepthwiseConv2dFunction": "(ctx, input, weight, bias=None, stride=1, padding=1)",
    "Conv5x5Function": "(ctx, input, weight, bias=None, compute='fp32')",
    "BatchNormFunction": BATCH_NORM_FORWARD,
    "MaxPool2dFunction": MAX_POOL_FORWARD,
    "L2NormFunction": "(ctx, input, weight, eps=1e-10)",
    "ToNhwcFunction": "(ctx, input, dtype)",
    "FromNhwcFunction": "(ctx, input)",
    "Conv2dNhwcFunction": "(ctx, input, weight, bias=None, padding=0, dilation=1, flags=0)",
    "BatchNormNhwcFunction": BATCH_NORM_FORWARD,
    "MaxPool2dNhwcFunction": MAX_POOL_FORWARD,
}
MODULES = {
    "ConvOffset2d": "(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, num_deformable_groups=1)",
    "Conv2d": "(self, in_channels, out_channels, kernel_size, padding=0, dilation=1, bias=True, compute='fp32', stride=1)",
    "ConvTranspose2d": "(self, in_channels, out_channels, kernel_size=2, stride=2, padding=0, output_padding=0, bias=True, compute='fp32')",
    "DepthwiseConv2d": "(self, channels, stride=1, bias=False)",
    "Conv5x5": "(self, in_channels, out_channels, bias=True, compute='fp32')",
    "BatchNorm2d": "(self, num_features, eps=1e-05, momentum=0.1, relu=False)",
    "MaxPool2d": "(self, kernel_size, stride=None, padding=0, ceil_mode=False)",
    "L2Norm": "(self, n_channels, scale)",
}


def _own(kind):
    """the public names of `kind` that networks itself defines (not what it imports)"""
    return {n: o for n, o in vars(networks).items() if not n.startswith("_") and kind(o) and o.__module__ == networks.__name__}


def test_public_functions():
    own = _own(inspect.isfunction)
    assert sorted(own) == sorted(FUNCTIONS)
    assert {n: str(inspect.signature(f)) for n, f in own.items()} == FUNCTIONS


def test_classes_and_their_signatures():
    own = _own(inspect.isclass)
    assert sorted(own) == sorted(list(FORWARDS) + list(MODULES))
    for name in FORWARDS:
        cls = own[name]
        assert cls.__name__ == name and issubclass(cls, torch.autograd.Function)
        assert str(inspect.signature(cls.forward)) == FORWARDS[name], name
        assert str(inspect.signature(cls.backward)) == "(ctx, grad_output)", name
    for name in MODULES:
        cls = own[name]
        assert cls.__name__ == name and issubclass(cls, torch.nn.Module)
        assert str(inspect.signature(cls.__init__)) == MODULES[name], name
        assert list(inspect.signature(cls.forward).parameters) == (["self", "input", "offset"] if name == "ConvOffset2d" else
                                                                   ["self", "x"] if name == "L2Norm" else ["self", "input"])


def test_constants():
    assert networks.RESIDENT_CHANNELS == 64
    assert networks.ConvOffset2dTsFunction.save_y is True
    assert sorted(networks.vgg_base) == ["300", "320", "512"]
