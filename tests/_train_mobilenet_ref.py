"""Differentiable CPU restatement of RefineSSD.forward_train of dualrefinedet_mobilenet (test helper; product code never imports it).

The walk is oracle/net_ref.py's (mobilenet_trunk, drn_mobilenet_forward, _drn_head) on torch's functional ops, in the dtype of the
tensors it is given (float64: the reference; float32: the yardstick of what two correct fp32 implementations may differ by), with
F.batch_norm(training=...) in place of the folded inference BN and tests/_deform_grad_ref.deform_conv for the heads, as
tests/_train_net_ref.py does for the VGG model; split_state and smooth_loss are that file's.  The head convs are bias-free.
"""
import torch
import torch.nn.functional as F

import _deform_grad_ref as D
from _train_net_ref import EPS, MOMENTUM, smooth_loss, split_state  # noqa: F401
from _train_net_ref import bn_after_conv as bn_after_conv_names  # noqa: F401

STRIDES = [1, 2, 1, 1, 1, 2, 1, 1, 1, 1, 1, 2, 1]       # backbone.1 .. backbone.13
CANCELLING = ("extras.0.0.bias", "extras.1.0.bias")    # the two conv biases in front of a training-mode BatchNorm


def forward(params, buffers, x, multihead, training, num_classes=21, taps=None, sums=None):
    """-> (arm_loc (B, P, 4), odm_loc (B, P, 4), conf (B, P, num_classes)); the running buffers are updated in place in training.
    sums (a dict): the outputs of the two biased convs, kept so that the caller can take their gradient"""
    P = dict(params)
    P.update(buffers)
    tp = taps if taps is not None else {}

    def conv(name, t, stride=1, padding=0, groups=1):
        return F.conv2d(t, P[name + ".weight"], P.get(name + ".bias"), stride, padding, 1, groups)

    def bn_relu(name, t):
        if training:
            P[name + ".num_batches_tracked"] += 1
        return F.relu(F.batch_norm(t, P[name + ".running_mean"], P[name + ".running_var"], P[name + ".weight"], P[name + ".bias"],
                                   training, MOMENTUM, EPS))

    def conv_dw(name, t, stride):
        t = bn_relu(name + ".1", conv(name + ".0", t, stride, 1, t.shape[1]))
        return bn_relu(name + ".4", conv(name + ".3", t))

    def l2norm(name, t):
        return P[name + ".weight"].view(1, -1, 1, 1) * (t / (t.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10))

    def deform(t, off, name, pad):
        return D.deform_conv(t.double(), off.double(), P[name + ".weight"].double(), 1, pad, 1, 1).to(t.dtype)

    x = bn_relu("backbone.0.1", conv("backbone.0.0", x, 2, 1))
    srcs = []
    for i, s in enumerate(STRIDES):
        x = conv_dw("backbone.%d" % (i + 1), x, s)
        if i + 1 == 11:
            srcs.append(l2norm("L2Norm_4_3", x))
    srcs.append(l2norm("L2Norm_5_3", x))
    for k in range(2):
        z = conv("extras.%d.0" % k, x)
        if sums is not None:
            sums["extras.%d.0" % k] = z
        x = conv_dw("extras.%d.3" % k, bn_relu("extras.%d.1" % k, z), 2)
        srcs.append(x)

    B = x.size(0)
    arm, off1, off2 = [], [], []
    for s, a in enumerate(srcs):
        loc_a = conv("arm_loc.%d" % s, a, padding=1)
        arm.append(loc_a.permute(0, 2, 3, 1).contiguous().view(B, -1))
        off1.append(conv("offset.%d" % s, loc_a))
        if multihead:
            off2.append(conv("offset2.%d" % s, loc_a))
        tp["offset.%d" % s] = torch.cat([off1[-1]] + ([off2[-1]] if multihead else []), 1).detach()
    x = F.relu(conv("last_layer_trans.0", x, padding=1))
    x = conv("last_layer_trans.3", conv("last_layer_trans.2", x, padding=1), padding=1)
    odm_sources = [x]
    trans = [conv("trans_layers.%d.2" % s, F.relu(conv("trans_layers.%d.0" % s, srcs[s], padding=1)), padding=1) for s in range(3)]
    trans.reverse()
    for i, t in enumerate(trans):
        u = F.relu(F.conv_transpose2d(x, P["up_layers.%d.weight" % i], P.get("up_layers.%d.bias" % i), stride=2) + t)
        x = F.relu(conv("latent_layers.%d" % i, u, padding=1))
        odm_sources.append(x)
    odm_sources.reverse()
    locs, confs = [], []
    for s, ob in enumerate(odm_sources):
        l, c = deform(ob, off1[s], "odm_loc.%d" % s, 1), deform(ob, off1[s], "odm_conf.%d" % s, 1)
        if multihead:
            l = l + deform(ob, off2[s], "odm_loc_2.%d" % s, 2)
            c = c + deform(ob, off2[s], "odm_conf_2.%d" % s, 2)
        locs.append(l.permute(0, 2, 3, 1).contiguous().view(B, -1))
        confs.append(c.permute(0, 2, 3, 1).contiguous().view(B, -1))
    return torch.cat(arm, 1).view(B, -1, 4), torch.cat(locs, 1).view(B, -1, 4), torch.cat(confs, 1).view(B, -1, num_classes)


def sgd_run(sd, x, targets, multihead, dtype, steps, lr):
    """`steps` plain-SGD steps on smooth_loss in training mode -> a list, one entry per step, of dict(outs, loss, grads, buffers
    (after the step's forward), taps (the offsets, for net_ref.border_rows), abs_go ({cancelling bias: sum |grad_output| of its
    conv, per channel})), and the final parameters"""
    params, buffers = split_state(sd, dtype)
    x = torch.as_tensor(x).to(dtype)
    log = []
    for _ in range(steps):
        taps, sums = {}, {}
        outs = forward(params, buffers, x, multihead, True, taps=taps, sums=sums)
        loss = smooth_loss(outs, targets)
        names, zs = list(params), list(sums)
        got = torch.autograd.grad(loss, [params[n] for n in names] + [sums[z] for z in zs])
        grads = dict(zip(names, got))
        abs_go = {z + ".bias": g.detach().abs().sum((0, 2, 3)) for z, g in zip(zs, got[len(names):])}
        log.append(dict(outs=[o.detach().clone() for o in outs], loss=float(loss.detach()), grads=grads,
                        buffers={k: v.clone() for k, v in buffers.items()}, taps=taps, abs_go=abs_go))
        with torch.no_grad():
            for n in names:
                params[n] -= lr * grads[n]
    return log, {n: p.detach() for n, p in params.items()}
