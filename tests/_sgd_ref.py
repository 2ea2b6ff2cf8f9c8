"""The SGD step of tdrn_hip.h section (i-j) restated in numpy fp32, and the reference's two learning-rate schedules.

numpy never fuses a multiply into an add: every line below is one fp32 operation per element, rounded on its own, which is what
the kernel (built with -ffp-contract=off) promises bit for bit.
"""
import numpy as np


def sgd_step(p, g, b, lr, momentum=0.0, weight_decay=0.0, nesterov=False):
    """One step on fp32 arrays: returns the new (p, b), leaves the inputs alone.  b is returned unchanged when momentum == 0."""
    assert p.dtype == g.dtype == b.dtype == np.float32
    lr, mom, wd = np.float32(lr), np.float32(momentum), np.float32(weight_decay)
    with np.errstate(all="ignore"):
        d = g + wd * p if wd != 0 else g
        if mom != 0:
            b = mom * b + d
            u = d + mom * b if nesterov else b
        else:
            u = d
        p = p - lr * u
    assert p.dtype == np.float32 and b.dtype == np.float32
    return p, b


def warmup_step_lr(base_lr, gamma, epoch, step_index, iteration, epoch_size, warm_epoch):
    # train.py:321-326
    #     if epoch <= args.warm_epoch:
    #         lr = 1e-6 + (args.lr - 1e-6) * iteration / (epoch_size * args.warm_epoch)
    #     else:
    #         lr = args.lr * (gamma ** (step_index))
    if epoch <= warm_epoch:
        lr = 1e-6 + (base_lr - 1e-6) * iteration / (epoch_size * warm_epoch)
    else:
        lr = base_lr * (gamma ** (step_index))
    return lr


def step_lr(base_lr, gamma, step_index):
    # train_trn.py:262
    #     lr = args.lr * (gamma ** (step_index))
    lr = base_lr * (gamma ** (step_index))
    return lr
