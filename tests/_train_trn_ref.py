"""Differentiable CPU restatement of SSD4Scale.forward_train (ssd4scale_vgg) and SSD4Scale_MobNet.forward_train (ssd4scale_mobile)
(test helper; product code never imports it).

The walks are oracle/net_ref.py's (_vgg_sources / mobilenet_trunk, _ssd4scale_heads) on torch's functional ops, in the dtype of the
tensors they are given (float64: the reference; float32: the yardstick of what two correct fp32 implementations may differ by), with
F.batch_norm(training=...) in place of the folded inference BN and tests/_deform_grad_ref.deform_conv (8 deformable groups) for the
heads of deform=True, as tests/_train_net_ref.py does; split_state and smooth_loss are that file's.  The trunk walks (vgg_sources,
mobilenet_sources, Ops) also serve tests/_train_refinedet_ref.py.
"""
import torch
import torch.nn.functional as F

import _deform_grad_ref as D
from _train_net_ref import EPS, MOMENTUM, VGG_CFG, smooth_loss, split_state  # noqa: F401

STRIDES = [1, 2, 1, 1, 1, 2, 1, 1, 1, 1, 1, 2, 1]       # backbone.1 .. backbone.13 of the MobileNet trunk
G = 8                                                   # deformable groups of the temporal nets


class Ops(object):
    """the layer functions over one parameter / buffer dict.  sums: {bias name: the output of a biased conv that feeds a BatchNorm},
    kept so that the caller can take its gradient (a cancelling bias is judged against sum |grad_output|)"""

    def __init__(self, params, buffers, training):
        self.P = dict(params)
        self.P.update(buffers)
        self.training, self.sums = training, {}

    def conv(self, name, t, stride=1, padding=0, dilation=1, groups=1):
        return F.conv2d(t, self.P[name + ".weight"], self.P.get(name + ".bias"), stride, padding, dilation, groups)

    def bn_relu(self, name, t):
        P = self.P
        if self.training:
            P[name + ".num_batches_tracked"] += 1
        return F.relu(F.batch_norm(t, P[name + ".running_mean"], P[name + ".running_var"], P[name + ".weight"], P[name + ".bias"],
                                   self.training, MOMENTUM, EPS))

    def conv_bn_relu(self, conv, bn, t, **kw):
        z = self.conv(conv, t, **kw)
        if (conv + ".bias") in self.P:
            self.sums[conv + ".bias"] = z
        return self.bn_relu(bn, z)

    def conv_dw(self, name, t, stride):
        t = self.conv_bn_relu(name + ".0", name + ".1", t, stride=stride, padding=1, groups=t.shape[1])
        return self.conv_bn_relu(name + ".3", name + ".4", t)

    def l2norm(self, name, t):
        return self.P[name + ".weight"].view(1, -1, 1, 1) * (t / (t.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10))

    def deform(self, t, off, name, pad, groups):
        return D.deform_conv(t.double(), off.double(), self.P[name + ".weight"].double(), 1, pad, 1, groups).to(t.dtype)


def vgg_sources(o, x):
    """the VGG16-BN trunk -> [L2Norm(conv4_3), L2Norm(conv5_3), fc7, extras]"""
    idx, n_conv, feats = 0, 0, []
    for v in VGG_CFG:
        if v in ("M", "C"):
            x = F.max_pool2d(x, 2, 2, ceil_mode=(v == "C"))
            idx += 1
            continue
        x = o.conv_bn_relu("backbone.%d" % idx, "backbone.%d" % (idx + 1), x, padding=1)
        idx += 3
        n_conv += 1
        if n_conv in (10, 13):
            feats.append(x)
    x = F.max_pool2d(x, 2, 2)
    idx += 1
    x = o.conv_bn_relu("backbone.%d" % idx, "backbone.%d" % (idx + 1), x, padding=6, dilation=6)
    idx += 3
    x = o.conv_bn_relu("backbone.%d" % idx, "backbone.%d" % (idx + 1), x)
    e = o.conv_bn_relu("extras.0", "extras.1", x)
    e = o.conv_bn_relu("extras.3", "extras.4", e, stride=2, padding=1)
    return [o.l2norm("L2Norm_4_3", feats[0]), o.l2norm("L2Norm_5_3", feats[1]), x, e]


def mobilenet_sources(o, x):
    """the MobileNet trunk -> [L2Norm(block 11), L2Norm(block 13), extras.0, extras.1]"""
    x = o.conv_bn_relu("backbone.0.0", "backbone.0.1", x, stride=2, padding=1)
    srcs = []
    for i, s in enumerate(STRIDES):
        x = o.conv_dw("backbone.%d" % (i + 1), x, s)
        if i + 1 == 11:
            srcs.append(o.l2norm("L2Norm_4_3", x))
    srcs.append(o.l2norm("L2Norm_5_3", x))
    for k in range(2):
        x = o.conv_dw("extras.%d.3" % k, o.conv_bn_relu("extras.%d.0" % k, "extras.%d.1" % k, x), 2)
        srcs.append(x)
    return srcs


SOURCES = {"vgg": vgg_sources, "mobile": mobilenet_sources}


def forward(params, buffers, x, arch, deform, training, ref_loc=None, num_classes=21, taps=None, sums=None):
    """-> (arm_loc (B, P, 4), arm_conf (B, P, num_classes), the four loc maps or []); the running buffers are updated in place in
    training.  taps["offset.<s>"]: the offsets of level s."""
    o = Ops(params, buffers, training)
    srcs = SOURCES[arch](o, x)
    B = x.size(0)
    locs, confs, maps = [], [], []
    for s, a in enumerate(srcs):
        if deform:
            off = o.conv("offset.%d" % s, ref_loc[s])
            if taps is not None:
                taps["offset.%d" % s] = off.detach()
            l, c = o.deform(a, off, "arm_loc.%d" % s, 1, G), o.deform(a, off, "arm_conf.%d" % s, 1, G)
        else:
            l, c = o.conv("arm_loc.%d" % s, a, padding=1), o.conv("arm_conf.%d" % s, a, padding=1)
            maps.append(l)
        locs.append(l.permute(0, 2, 3, 1).contiguous().view(B, -1))
        confs.append(c.permute(0, 2, 3, 1).contiguous().view(B, -1))
    if sums is not None:
        sums.update(o.sums)
    return torch.cat(locs, 1).view(B, -1, 4), torch.cat(confs, 1).view(B, -1, num_classes), maps


def sgd_run(sd, x, targets, arch, deform, dtype, steps, lr, ref_loc=None, ref_loc_grad=False):
    """`steps` plain-SGD steps on smooth_loss in training mode -> a list, one entry per step, of dict(outs, loss, grads, buffers
    (after the step's forward), taps, abs_go ({cancelling bias: sum |grad_output| of its conv, per channel}), ref_loc_grads (when
    ref_loc_grad)), and the final parameters"""
    params, buffers = split_state(sd, dtype)
    x = torch.as_tensor(x).to(dtype)
    if ref_loc is not None:
        ref_loc = [torch.as_tensor(r).to(dtype).clone().requires_grad_(ref_loc_grad) for r in ref_loc]
    log = []
    for _ in range(steps):
        taps, sums = {}, {}
        outs = forward(params, buffers, x, arch, deform, True, ref_loc, taps=taps, sums=sums)[:2]
        loss = smooth_loss(outs, targets)
        names, zs = list(params), list(sums)
        extra = list(ref_loc) if ref_loc_grad else []
        got = torch.autograd.grad(loss, [params[n] for n in names] + [sums[z] for z in zs] + extra)
        grads = dict(zip(names, got))
        abs_go = {z: g.detach().abs().sum((0, 2, 3)) for z, g in zip(zs, got[len(names):len(names) + len(zs)])}
        log.append(dict(outs=[t.detach().clone() for t in outs], loss=float(loss.detach()), grads=grads,
                        buffers={k: v.clone() for k, v in buffers.items()}, taps=taps, abs_go=abs_go,
                        ref_loc_grads=list(got[len(names) + len(zs):])))
        with torch.no_grad():
            for n in names:
                params[n] -= lr * grads[n]
    return log, {n: p.detach() for n, p in params.items()}
