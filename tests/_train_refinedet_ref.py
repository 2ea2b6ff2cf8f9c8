"""Differentiable CPU restatement of RefineSSD.forward_train of refinedet_vgg with bn=True (test helper; product code never imports
it).

The walk is oracle/net_ref.py's refinedet_vgg_forward on torch's functional ops, in the dtype of the tensors it is given (float64: the
reference; float32: the yardstick), with F.batch_norm(training=...) in place of the folded inference BN.  The trunk is
tests/_train_trn_ref.py's; the ODM heads are plain convs, 3x3 and, with multihead, 5x5 at pad 2, summed.
"""
import torch
import torch.nn.functional as F

from _train_trn_ref import Ops, smooth_loss, split_state, vgg_sources  # noqa: F401


def forward(params, buffers, x, use_refine, multihead, training, num_classes=21, sums=None):
    """-> (arm_loc, odm_loc, conf) with use_refine, else (odm_loc, conf); the running buffers are updated in place in training"""
    o = Ops(params, buffers, training)
    srcs = vgg_sources(o, x)
    B = x.size(0)
    flat = lambda t: t.permute(0, 2, 3, 1).contiguous().view(B, -1)
    arm = [flat(o.conv("arm_loc.%d" % s, a, padding=1)) for s, a in enumerate(srcs)] if use_refine else None
    x = F.relu(o.conv("last_layer_trans.0", srcs[3], padding=1))
    x = o.conv("last_layer_trans.3", o.conv("last_layer_trans.2", x, padding=1), padding=1)
    odm = [x]
    trans = [o.conv("trans_layers.%d.2" % s, F.relu(o.conv("trans_layers.%d.0" % s, srcs[s], padding=1)), padding=1) for s in range(3)]
    trans.reverse()
    for i, t in enumerate(trans):
        u = F.relu(F.conv_transpose2d(x, o.P["up_layers.%d.weight" % i], o.P["up_layers.%d.bias" % i], stride=2) + t)
        x = F.relu(o.conv("latent_layers.%d" % i, u, padding=1))
        odm.append(x)
    odm.reverse()
    locs, confs = [], []
    for s, ob in enumerate(odm):
        l, c = o.conv("odm_loc.%d" % s, ob, padding=1), o.conv("odm_conf.%d" % s, ob, padding=1)
        if multihead:
            l = l + o.conv("odm_loc_2.%d" % s, ob, padding=2)
            c = c + o.conv("odm_conf_2.%d" % s, ob, padding=2)
        locs.append(flat(l))
        confs.append(flat(c))
    if sums is not None:
        sums.update(o.sums)
    out = (torch.cat(locs, 1).view(B, -1, 4), torch.cat(confs, 1).view(B, -1, num_classes))
    return (torch.cat(arm, 1).view(B, -1, 4),) + out if use_refine else out


def sgd_run(sd, x, targets, use_refine, multihead, dtype, steps, lr):
    """`steps` plain-SGD steps on smooth_loss in training mode -> a list, one entry per step, of dict(outs, loss, grads, buffers
    (after the step's forward), abs_go ({cancelling bias: sum |grad_output| of its conv, per channel})), and the final parameters"""
    params, buffers = split_state(sd, dtype)
    x = torch.as_tensor(x).to(dtype)
    log = []
    for _ in range(steps):
        sums = {}
        outs = forward(params, buffers, x, use_refine, multihead, True, sums=sums)
        loss = smooth_loss(outs, targets)
        names, zs = list(params), list(sums)
        got = torch.autograd.grad(loss, [params[n] for n in names] + [sums[z] for z in zs])
        grads = dict(zip(names, got))
        abs_go = {z: g.detach().abs().sum((0, 2, 3)) for z, g in zip(zs, got[len(names):])}
        log.append(dict(outs=[t.detach().clone() for t in outs], loss=float(loss.detach()), grads=grads,
                        buffers={k: v.clone() for k, v in buffers.items()}, abs_go=abs_go))
        with torch.no_grad():
            for n in names:
                params[n] -= lr * grads[n]
    return log, {n: p.detach() for n, p in params.items()}
