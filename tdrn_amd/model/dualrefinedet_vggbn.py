"""Dual-refinement detector on VGG16(-BN): drop-in for model/dualrefinedet_vggbn.py of the
reference (RefineSSD.__init__ :10-117, forward :119-206, build_net :217-222).  Same
state_dict keys, same `net(x)` 4-tuple, same prior ordering; the arithmetic runs in
libtdrn_hip.so (MFMA implicit-GEMM convs, fused deformable heads).  `net(x)` is the inference engine (BatchNorm folded, no
autograd graph); `net.forward_train(x)` computes the phase-'train' outputs from the module's own fp32 parameters through the
library's differentiable ops (networks.conv2d / batch_norm / max_pool2d / l2norm / conv_transpose2d / conv_offset2d), so that
`loss.backward()` fills their .grad."""
import torch
import torch.nn as nn

from .. import _lib
from ..layers.modules.l2norm import L2Norm
from . import networks
from ._base import EngineModule
from .networks import ConvOffset2d, vgg, vgg_base


def _c3(cin, cout, **kw):
    return nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1, **kw)


def add_refine_head(m, arm_channels, num_classes, def_groups, multihead, bias=True):
    """ARM loc / offset convs, TCB-FPN and deformable ODM heads shared by the VGG and MobileNet
    variants (dualrefinedet_vggbn.py:30-34,47-114; dualrefinedet_mobilenet.py:50-122)."""
    nb = 3
    m.last_layer_trans = nn.Sequential(_c3(arm_channels[3], 256, bias=bias), nn.ReLU(inplace=True),
                                       _c3(256, 256, bias=bias), _c3(256, 256, bias=bias))
    m.arm_loc = nn.ModuleList([_c3(c, nb * 4, bias=bias) for c in arm_channels])
    m.offset = nn.ModuleList([nn.Conv2d(nb * 4, def_groups * 18, 1, bias=bias) for _ in range(4)])
    dc = lambda cout, k: nn.ModuleList([ConvOffset2d(256, cout, k, 1, k // 2, num_deformable_groups=def_groups)
                                        for _ in range(4)])
    m.odm_loc, m.odm_conf = dc(nb * 4, 3), dc(nb * num_classes, 3)
    if multihead:
        m.offset2 = nn.ModuleList([nn.Conv2d(nb * 4, def_groups * 50, 1, bias=bias) for _ in range(4)])
        m.odm_loc_2, m.odm_conf_2 = dc(nb * 4, 5), dc(nb * num_classes, 5)
    m.trans_layers = nn.ModuleList([nn.Sequential(_c3(c, 256, bias=bias), nn.ReLU(inplace=True), _c3(256, 256, bias=bias))
                                    for c in arm_channels[:3]])
    m.up_layers = nn.ModuleList([nn.ConvTranspose2d(256, 256, 2, 2, 0, bias=bias) for _ in range(3)])
    m.latent_layers = nn.ModuleList([_c3(256, 256, bias=bias) for _ in range(3)])


class RefineSSD(EngineModule):
    def __init__(self, size, num_classes=21, phase='train', c7_channel=1024, def_groups=1, bn=True,
                 multihead=False, return_feature=False, device='cuda'):
        super(RefineSSD, self).__init__()
        self.num_classes, self.size, self.phase = num_classes, size, phase
        self.def_groups, self.bn, self.multihead = def_groups, bn, multihead
        self.return_feature, self.device = return_feature, device   # kwarg kept; its norm map was never returned
        self.backbone = nn.ModuleList(vgg(vgg_base['320'], 3, batch_norm=bn, pool5_ds=True, c7_channel=c7_channel))
        self.L2Norm_4_3 = L2Norm(512, 10)
        self.L2Norm_5_3 = L2Norm(512, 8)
        if bn:
            self.extras = nn.Sequential(nn.Conv2d(c7_channel, 256, 1), nn.BatchNorm2d(256), nn.ReLU(inplace=True),
                                        nn.Conv2d(256, 512, 3, 2, 1), nn.BatchNorm2d(512), nn.ReLU(inplace=True))
        else:
            self.extras = nn.Sequential(nn.Conv2d(c7_channel, 256, 1), nn.ReLU(inplace=True),
                                        nn.Conv2d(256, 512, 3, 2, 1), nn.ReLU(inplace=True))
        add_refine_head(self, [512, 512, c7_channel, 512], num_classes, def_groups, multihead, bias=True)
        if phase == 'test':
            self.softmax = nn.Softmax(dim=1)
        self._engine_init(model=_lib.DRN_VGGBN, size=size, num_classes=num_classes, c7_channel=c7_channel,
                          def_groups=def_groups, bn=bn, multihead=multihead, test_phase=(phase == 'test'))

    def forward(self, x):
        r = self.engine_for(x).forward(x, want_offsets=True)
        conf = r["conf"] if self.phase == 'test' else r["conf"].view(x.size(0), -1, self.num_classes)
        return (r["arm_loc"], r["offsets"] if self.phase == 'test' else None, r["odm_loc"], conf)

    # ---- the training forward: the reference's forward (:119-206) on the library's differentiable ops ------------------------
    def _bn_relu(self, bn, x):
        if bn.momentum is None:
            raise NotImplementedError("forward_train: BatchNorm2d(momentum=None) needs a host-side batch count; use networks.BatchNorm2d")
        if self.training and bn.track_running_stats:
            bn.num_batches_tracked.add_(1)            # on the device: no host read, no synchronisation
        return networks.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, self.training, bn.momentum, bn.eps,
                                   relu=True)

    def _walk(self, layers, x, compute, taps=()):
        """A list of nn.Conv2d [+ nn.BatchNorm2d] [+ nn.ReLU] and nn.MaxPool2d holders, in order -> (output, [the output behind
        conv number n (1-based, activation included) for n in taps])."""
        layers, kept, n_conv, i = list(layers), [], 0, 0
        while i < len(layers):
            m = layers[i]
            i += 1
            if isinstance(m, nn.MaxPool2d):
                x = networks.max_pool2d(x, m.kernel_size, m.stride, m.padding, m.ceil_mode)
                continue
            if not isinstance(m, nn.Conv2d) or m.groups != 1:
                raise NotImplementedError("forward_train: no differentiable op for %r" % (m,))
            x = networks.conv2d(x, m.weight, m.bias, m.padding, m.dilation, compute, m.stride)
            if i < len(layers) and isinstance(layers[i], nn.BatchNorm2d):
                x = self._bn_relu(layers[i], x)        # the nn.ReLU behind it is fused
                i += 2 if i + 1 < len(layers) and isinstance(layers[i + 1], nn.ReLU) else 1
            elif i < len(layers) and isinstance(layers[i], nn.ReLU):
                x = torch.relu(x)
                i += 1
            n_conv += 1
            if n_conv in taps:
                kept.append(x)
        return x, kept

    def forward_train(self, x, compute="fp32"):
        """-> (arm_loc (B, P, 4), None, odm_loc (B, P, 4), conf (B, P, num_classes) raw logits): the phase-'train' outputs of
        forward, computed from this module's fp32 parameters with an autograd graph.  BatchNorm runs in the module's mode
        (self.training: batch statistics, running buffers updated with each layer's momentum; else the running buffers).
        `compute` ("fp32" | "bf16" | "fp16") is the MFMA input type of every conv-type op; BatchNorm, pools and L2Norm are fp32.
        The engine's packed weights are marked stale, so net(x) after an optimizer step re-packs by itself."""
        if x.dim() != 4:
            raise ValueError("Expected 4D tensor as input, got {}D tensor instead.".format(x.dim()))
        _lib.require_cuda(x, "input")
        object.__setattr__(self, "_dirty", True)
        B = x.size(0)
        conv = lambda m, t, pad: networks.conv2d(t, m.weight, m.bias, pad, 1, compute)
        x, (c43, c53) = self._walk(self.backbone, x.float(), compute, taps=(10, 13))     # x: fc7; conv4_3, conv5_3 behind their ReLU
        arm_sources = [networks.l2norm(c43, self.L2Norm_4_3.weight, self.L2Norm_4_3.eps),
                       networks.l2norm(c53, self.L2Norm_5_3.weight, self.L2Norm_5_3.eps), x]
        x, _ = self._walk(self.extras, x, compute)
        arm_sources.append(x)
        arm_loc, off1, off2 = [], [], []
        for s, a in enumerate(arm_sources):
            loc_a = conv(self.arm_loc[s], a, 1)
            arm_loc.append(loc_a.permute(0, 2, 3, 1).contiguous().view(B, -1))
            off1.append(conv(self.offset[s], loc_a, 0))
            if self.multihead:
                off2.append(conv(self.offset2[s], loc_a, 0))
        x, _ = self._walk(self.last_layer_trans, x, compute)
        odm_sources = [x]
        trans = [self._walk(self.trans_layers[s], arm_sources[s], compute)[0] for s in range(3)]
        trans.reverse()
        for i, t in enumerate(trans):
            up = self.up_layers[i]
            u = torch.relu(networks.conv_transpose2d(x, up.weight, up.bias, 2, compute) + t)
            x = torch.relu(conv(self.latent_layers[i], u, 1))
            odm_sources.append(x)
        odm_sources.reverse()
        odm_loc, odm_conf = [], []
        for s, ob in enumerate(odm_sources):
            heads = [(self.odm_loc[s], self.odm_conf[s], off1[s])]
            if self.multihead:
                heads.append((self.odm_loc_2[s], self.odm_conf_2[s], off2[s]))
            l = c = None
            for hl, hc, off in heads:
                dl, dc = (networks.conv_offset2d(ob, off, h.weight, h.stride, h.padding, h.dilation, h.num_deformable_groups, compute)
                          for h in (hl, hc))
                l, c = (dl, dc) if l is None else (l + dl, c + dc)
            odm_loc.append(l.permute(0, 2, 3, 1).contiguous().view(B, -1))
            odm_conf.append(c.permute(0, 2, 3, 1).contiguous().view(B, -1))
        return (torch.cat(arm_loc, 1).view(B, -1, 4), None, torch.cat(odm_loc, 1).view(B, -1, 4),
                torch.cat(odm_conf, 1).view(B, -1, self.num_classes))


def build_net(phase, size=320, num_classes=21, c7_channel=1024, def_groups=1, bn=True, multihead=False,
              return_feature=False):
    if size not in [320, 512]:
        print("Error: Sorry only SSD320 and SSD512 is supported currently!")
        return
    return RefineSSD(size, num_classes=num_classes, phase=phase, c7_channel=c7_channel, def_groups=def_groups,
                     bn=bn, multihead=multihead, return_feature=return_feature)
