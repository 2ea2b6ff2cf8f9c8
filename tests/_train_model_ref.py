"""Differentiable CPU restatement of forward_train of the five trainable models (test helper; product code never imports it):
dualrefinedet_vggbn, dualrefinedet_mobilenet, refinedet_vgg (bn=True), ssd4scale_vgg (bn=True) and ssd4scale_mobile.

The walks are oracle/net_ref.py's (vgg_trunk / mobilenet_trunk, _drn_head, refinedet_vgg_forward, _ssd4scale_heads) on torch's
functional ops, in the dtype of the tensors they are given (float64: the reference; float32: the yardstick of what two correct fp32
implementations may differ by), with F.batch_norm(training=...) in place of the folded inference BN and
tests/_deform_grad_ref.deform_conv for the deformable heads.  That helper computes in float64 whatever it is given, so in a float32
run the deformable heads alone are float64 (cast back): the yardstick is then a little BETTER than a pure float32 evaluation, which
makes the bound derived from it tighter, never wider.  tests/test_train_model_ref.py ties every walk to the oracle in eval mode.

Each piece is written once: Ops (the layer vocabulary), the two trunks, the TCB pyramid, the three head forms; a model's forward
composes them.  The order in which a forward creates its ops is part of the reference: autograd sums the gradients of a tensor with
three consumers (fc7; an ARM loc map under multihead) in the reverse of that order.
"""
import numpy as np
import torch
import torch.nn.functional as F

import _deform_grad_ref as D

VGG_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "C", 512, 512, 512, "M", 512, 512, 512]
STRIDES = [1, 2, 1, 1, 1, 2, 1, 1, 1, 1, 1, 2, 1]       # backbone.1 .. backbone.13 of the MobileNet trunk
MOMENTUM, EPS = 0.1, 1e-5
G = 8                                                   # deformable groups of the temporal nets
CANCELLING = ("extras.0.0.bias", "extras.1.0.bias")    # MobileNet's two conv biases in front of a training-mode BatchNorm


def split_state(sd, dtype):
    """a state dict (numpy or torch) -> ({name: leaf tensor requiring grad}, {name: buffer clone}) in `dtype` (counters stay int64)"""
    params, buffers = {}, {}
    for k, v in sd.items():
        t = torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v.detach().cpu())
        if k.endswith("num_batches_tracked"):
            buffers[k] = t.clone().long()
        elif k.endswith("running_mean") or k.endswith("running_var"):
            buffers[k] = t.clone().to(dtype)
        else:
            params[k] = t.clone().to(dtype).requires_grad_(True)
    return params, buffers


def bn_after_conv(keys):
    """state-dict keys -> {conv bias name: the prefix of the BatchNorm that follows the conv}: backbone.<i> -> backbone.<i+1>,
    extras.0 -> extras.1, extras.3 -> extras.4"""
    keys, out = set(keys), {}
    for k in keys:
        if k.endswith(".bias") and (k[:-5] + ".running_mean") not in keys:
            head, _, idx = k[:-5].rpartition(".")
            if idx.isdigit() and ("%s.%d.running_mean" % (head, int(idx) + 1)) in keys:
                out[k] = "%s.%d" % (head, int(idx) + 1)
    return out


def smooth_loss(outs, targets):
    """mean squared distance of the outputs to fixed targets"""
    return sum(((o - t.to(o.dtype).to(o.device)) ** 2).mean() for o, t in zip(outs, targets))


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


def vgg_sources(o, x, bn=True):
    """the VGG16 trunk -> [L2Norm(conv4_3), L2Norm(conv5_3), fc7, extras].  bn=False: ReLU in place of BatchNorm + ReLU and the
    state-dict indices of vgg(batch_norm=False): a conv every 2 holders instead of every 3, extras.0 and extras.2"""
    step = 3 if bn else 2

    def layer(prefix, idx, t, **kw):
        name = "%s.%d" % (prefix, idx)
        return o.conv_bn_relu(name, "%s.%d" % (prefix, idx + 1), t, **kw) if bn else F.relu(o.conv(name, t, **kw))

    idx, n_conv, feats = 0, 0, []
    for v in VGG_CFG:
        if v in ("M", "C"):
            x = F.max_pool2d(x, 2, 2, ceil_mode=(v == "C"))
            idx += 1
            continue
        x = layer("backbone", idx, x, padding=1)
        idx += step
        n_conv += 1
        if n_conv in (10, 13):
            feats.append(x)
    x = F.max_pool2d(x, 2, 2)
    idx += 1
    x = layer("backbone", idx, x, padding=6, dilation=6)
    idx += step
    x = layer("backbone", idx, x)
    e = layer("extras", 0, x)
    e = layer("extras", step, e, stride=2, padding=1)
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


def tcb_pyramid(o, srcs):
    """last_layer_trans on the last source, then the three transfer-connection blocks -> the four ODM sources, largest map first"""
    x = F.relu(o.conv("last_layer_trans.0", srcs[3], padding=1))
    x = o.conv("last_layer_trans.3", o.conv("last_layer_trans.2", x, padding=1), padding=1)
    odm = [x]
    trans = [o.conv("trans_layers.%d.2" % s, F.relu(o.conv("trans_layers.%d.0" % s, srcs[s], padding=1)), padding=1) for s in range(3)]
    trans.reverse()
    for i, t in enumerate(trans):
        u = F.relu(F.conv_transpose2d(x, o.P["up_layers.%d.weight" % i], o.P.get("up_layers.%d.bias" % i), stride=2) + t)
        x = F.relu(o.conv("latent_layers.%d" % i, u, padding=1))
        odm.append(x)
    odm.reverse()
    return odm


def rows(maps, width):
    """per-level (B, A * width, H, W) maps -> (B, P, width), scale-major, then pixel, then anchor"""
    B = maps[0].size(0)
    return torch.cat([m.permute(0, 2, 3, 1).contiguous().view(B, -1) for m in maps], 1).view(B, -1, width)


def arm_loc_maps(o, srcs):
    return [o.conv("arm_loc.%d" % s, a, padding=1) for s, a in enumerate(srcs)]


def drn_odm_heads(o, loc_maps, odm, multihead, taps=None):
    """the dual-refinement heads: offsets from the ARM loc maps, one deformable group, 3x3 and with multihead a 5x5 branch, summed ->
    the loc and conf maps per level.  taps["offset.<s>"] = [offset ; offset2], as net_ref.border_rows reads them"""
    locs, confs = [], []
    for s, (loc_a, ob) in enumerate(zip(loc_maps, odm)):
        off1 = o.conv("offset.%d" % s, loc_a)
        off2 = o.conv("offset2.%d" % s, loc_a) if multihead else None
        if taps is not None:
            taps["offset.%d" % s] = torch.cat([off1] + ([off2] if multihead else []), 1).detach()
        l, c = o.deform(ob, off1, "odm_loc.%d" % s, 1, 1), o.deform(ob, off1, "odm_conf.%d" % s, 1, 1)
        if multihead:
            l = l + o.deform(ob, off2, "odm_loc_2.%d" % s, 2, 1)
            c = c + o.deform(ob, off2, "odm_conf_2.%d" % s, 2, 1)
        locs.append(l)
        confs.append(c)
    return locs, confs


def dense_odm_heads(o, odm, multihead):
    """RefineDet's heads: plain convs, 3x3 and with multihead a 5x5 at pad 2, summed -> the loc and conf maps per level"""
    locs, confs = [], []
    for s, ob in enumerate(odm):
        l, c = o.conv("odm_loc.%d" % s, ob, padding=1), o.conv("odm_conf.%d" % s, ob, padding=1)
        if multihead:
            l = l + o.conv("odm_loc_2.%d" % s, ob, padding=2)
            c = c + o.conv("odm_conf_2.%d" % s, ob, padding=2)
        locs.append(l)
        confs.append(c)
    return locs, confs


def ssd4scale_heads(o, srcs, deform, ref_loc=None, taps=None):
    """SSD4Scale's heads on the sources: dense 3x3, or deformable with G groups and offsets from ref_loc -> the loc and conf maps per
    level.  taps["offset.<s>"]: the offsets of level s"""
    locs, confs = [], []
    for s, a in enumerate(srcs):
        if deform:
            off = o.conv("offset.%d" % s, ref_loc[s])
            if taps is not None:
                taps["offset.%d" % s] = off.detach()
            l, c = o.deform(a, off, "arm_loc.%d" % s, 1, G), o.deform(a, off, "arm_conf.%d" % s, 1, G)
        else:
            l, c = o.conv("arm_loc.%d" % s, a, padding=1), o.conv("arm_conf.%d" % s, a, padding=1)
        locs.append(l)
        confs.append(c)
    return locs, confs


# ---- the models: forward(o, x, taps) -> the phase-'train' outputs; the running buffers of `o` are updated in place in training ---------
def drn_forward(o, x, taps=None, *, arch, multihead, num_classes=21):
    """dualrefinedet_vggbn / dualrefinedet_mobilenet -> (arm_loc (B, P, 4), odm_loc (B, P, 4), conf (B, P, num_classes))"""
    srcs = SOURCES[arch](o, x)
    loc_maps = arm_loc_maps(o, srcs)
    arm = rows(loc_maps, 4)
    locs, confs = drn_odm_heads(o, loc_maps, tcb_pyramid(o, srcs), multihead, taps)
    return arm, rows(locs, 4), rows(confs, num_classes)


def refinedet_forward(o, x, taps=None, *, use_refine, multihead, num_classes=21):
    """refinedet_vgg (bn=True) -> (arm_loc, odm_loc, conf) with use_refine, else (odm_loc, conf)"""
    srcs = vgg_sources(o, x)
    arm = (rows(arm_loc_maps(o, srcs), 4),) if use_refine else ()
    locs, confs = dense_odm_heads(o, tcb_pyramid(o, srcs), multihead)
    return arm + (rows(locs, 4), rows(confs, num_classes))


def ssd4scale_forward(o, x, taps=None, ref_loc=None, *, arch, deform, num_classes=21, ret_loc=False):
    """ssd4scale_vgg (bn=True) / ssd4scale_mobile -> (arm_loc (B, P, 4), arm_conf (B, P, num_classes)) and, with ret_loc, the four loc
    maps of the static net ([] for the temporal one, as the model)"""
    locs, confs = ssd4scale_heads(o, SOURCES[arch](o, x), deform, ref_loc, taps)
    out = (rows(locs, 4), rows(confs, num_classes))
    return out + ([] if deform else locs,) if ret_loc else out


def run(forward, sd, x, dtype, training, *extra):
    """one forward under no_grad on a private copy of the state `sd` (numpy or torch, never changed) -> what `forward` returns"""
    o = Ops(*split_state(sd, dtype), training)
    with torch.no_grad():
        return forward(o, torch.as_tensor(x).to(dtype), None, *extra)


def arm_loc(sd, x, bn, dtype):
    """the part of dualrefinedet_vggbn in front of the deformable heads, with or without BatchNorm: the trunk and the four ARM loc
    heads, training mode -> arm_loc (B, P, 4) in `dtype`"""
    return run(lambda o, t, taps: rows(arm_loc_maps(o, vgg_sources(o, t, bn)), 4), sd, x, dtype, True)


def sgd_run(forward, sd, x, targets, dtype, steps, lr, extra=None, extra_grad=False):
    """`steps` plain-SGD steps on smooth_loss in training mode.  forward(o, x, taps[, extra]): a model above with its arguments bound;
    extra: further input tensors (ref_loc), leaves that require grad with extra_grad.  -> a list, one entry per step, of dict(outs,
    loss, grads, buffers (after the step's forward), taps (the offsets, for net_ref.border_rows), abs_go ({cancelling bias: sum
    |grad_output| of its conv, per channel}), extra_grads ([] without extra_grad)), and the final parameters"""
    params, buffers = split_state(sd, dtype)
    x = torch.as_tensor(x).to(dtype)
    if extra is not None:
        extra = [torch.as_tensor(r).to(dtype).clone().requires_grad_(extra_grad) for r in extra]
    log = []
    for _ in range(steps):
        o, taps = Ops(params, buffers, True), {}
        outs = forward(o, x, taps) if extra is None else forward(o, x, taps, extra)
        loss = smooth_loss(outs, targets)
        names, zs = list(params), list(o.sums)
        leaves = list(extra) if extra_grad else []
        got = torch.autograd.grad(loss, [params[n] for n in names] + [o.sums[z] for z in zs] + leaves)
        grads = dict(zip(names, got))
        abs_go = {z: g.detach().abs().sum((0, 2, 3)) for z, g in zip(zs, got[len(names):len(names) + len(zs)])}
        log.append(dict(outs=[t.detach().clone() for t in outs], loss=float(loss.detach()), grads=grads,
                        buffers={k: v.clone() for k, v in buffers.items()}, taps=taps, abs_go=abs_go,
                        extra_grads=list(got[len(names) + len(zs):])))
        with torch.no_grad():
            for n in names:
                params[n] -= lr * grads[n]
    return log, {n: p.detach() for n, p in params.items()}
