"""Differentiable CPU restatement of RefineSSD.forward_train of dualrefinedet_vggbn (test helper; product code never imports it).

The walk is oracle/net_ref.py's (vgg_trunk, drn_vggbn_forward, _drn_head) on torch's functional ops, in the dtype of the tensors it is
given (float64: the reference; float32: the yardstick of what two correct fp32 implementations may differ by), with
F.batch_norm(training=...) in place of the folded inference BN and tests/_deform_grad_ref.deform_conv for the heads.  That helper
computes in float64 whatever it is given, so in a float32 run the heads alone are float64 (cast back): the yardstick is then a
little BETTER than a pure float32 evaluation, which makes the bound derived from it tighter, never wider.
"""
import numpy as np
import torch
import torch.nn.functional as F

import _deform_grad_ref as D

VGG_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "C", 512, 512, 512, "M", 512, 512, 512]
MOMENTUM, EPS = 0.1, 1e-5


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


def forward(params, buffers, x, multihead, training, num_classes=21, taps=None):
    """-> (arm_loc (B, P, 4), odm_loc (B, P, 4), conf (B, P, num_classes)); the running buffers are updated in place in training"""
    P = dict(params)
    P.update(buffers)
    tp = taps if taps is not None else {}

    def conv(name, t, stride=1, padding=0, dilation=1):
        return F.conv2d(t, P[name + ".weight"], P.get(name + ".bias"), stride, padding, dilation)

    def bn_relu(name, t):
        if training:
            P[name + ".num_batches_tracked"] += 1
        return F.relu(F.batch_norm(t, P[name + ".running_mean"], P[name + ".running_var"], P[name + ".weight"], P[name + ".bias"],
                                   training, MOMENTUM, EPS))

    def l2norm(name, t):
        return P[name + ".weight"].view(1, -1, 1, 1) * (t / (t.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10))

    def deform(t, off, name, pad):
        return D.deform_conv(t.double(), off.double(), P[name + ".weight"].double(), 1, pad, 1, 1).to(t.dtype)

    idx, n_conv, feats = 0, 0, []
    for v in VGG_CFG:
        if v in ("M", "C"):
            x = F.max_pool2d(x, 2, 2, ceil_mode=(v == "C"))
            idx += 1
            continue
        x = bn_relu("backbone.%d" % (idx + 1), conv("backbone.%d" % idx, x, padding=1))
        idx += 3
        n_conv += 1
        if n_conv in (10, 13):
            feats.append(x)
    x = F.max_pool2d(x, 2, 2)
    idx += 1
    x = bn_relu("backbone.%d" % (idx + 1), conv("backbone.%d" % idx, x, padding=6, dilation=6))
    idx += 3
    x = bn_relu("backbone.%d" % (idx + 1), conv("backbone.%d" % idx, x))
    srcs = [l2norm("L2Norm_4_3", feats[0]), l2norm("L2Norm_5_3", feats[1]), x]
    e = bn_relu("extras.1", conv("extras.0", x))
    e = bn_relu("extras.4", conv("extras.3", e, stride=2, padding=1))
    srcs.append(e)

    B = x.size(0)
    arm, off1, off2 = [], [], []
    for s, a in enumerate(srcs):
        loc_a = conv("arm_loc.%d" % s, a, padding=1)
        arm.append(loc_a.permute(0, 2, 3, 1).contiguous().view(B, -1))
        off1.append(conv("offset.%d" % s, loc_a))
        if multihead:
            off2.append(conv("offset2.%d" % s, loc_a))
        tp["offset.%d" % s] = torch.cat([off1[-1]] + ([off2[-1]] if multihead else []), 1).detach()
    x = F.relu(conv("last_layer_trans.0", e, padding=1))
    x = conv("last_layer_trans.3", conv("last_layer_trans.2", x, padding=1), padding=1)
    odm_sources = [x]
    trans = [conv("trans_layers.%d.2" % s, F.relu(conv("trans_layers.%d.0" % s, srcs[s], padding=1)), padding=1) for s in range(3)]
    trans.reverse()
    for i, t in enumerate(trans):
        u = F.relu(F.conv_transpose2d(x, P["up_layers.%d.weight" % i], P["up_layers.%d.bias" % i], stride=2) + t)
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


def smooth_loss(outs, targets):
    """mean squared distance of the three outputs to fixed targets"""
    return sum(((o - t.to(o.dtype).to(o.device)) ** 2).mean() for o, t in zip(outs, targets))


def sgd_run(sd, x, targets, multihead, dtype, steps, lr):
    """`steps` plain-SGD steps on smooth_loss in training mode -> a list, one entry per step, of dict(outs, loss, grads, buffers
    (after the step's forward), taps (the offsets, for net_ref.border_rows)), and the final parameters"""
    params, buffers = split_state(sd, dtype)
    x = torch.as_tensor(x).to(dtype)
    log = []
    for _ in range(steps):
        taps = {}
        outs = forward(params, buffers, x, multihead, True, taps=taps)
        loss = smooth_loss(outs, targets)
        names = list(params)
        grads = dict(zip(names, torch.autograd.grad(loss, [params[n] for n in names])))
        log.append(dict(outs=[o.detach().clone() for o in outs], loss=float(loss.detach()), grads=grads,
                        buffers={k: v.clone() for k, v in buffers.items()}, taps=taps))
        with torch.no_grad():
            for n in names:
                params[n] -= lr * grads[n]
    return log, {n: p.detach() for n, p in params.items()}
