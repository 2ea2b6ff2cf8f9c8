"""Training losses: device time of the ARM + ODM criteria of train.py (RefineMultiBoxLoss, tdrn_hip.h section ii-b),
forward + backward, against a torch yardstick, with traffic derived from shapes.

    python scripts/loss_bench.py OUT_DIR [--batches 8,32] [--reps 21] [--ours-only]

Workload: VOC_320 priors (P = 6375), C = 21, VOC-like targets (1 to 40 truths per image), the engine's output shapes.
One step = arm_criterion(arm_loc) + criterion((odm_loc, conf), arm_data) and backward of their sum, between two device
events; the median of `reps` steps after a warm-up.  The yardstick is the reference's algorithm written as torch ops on
the GPU (a Python loop over images and truths for the matching, two sorts for the mining, boolean-mask gathers) and
differentiated by torch autograd; the two are timed alternately.  Writes OUT_DIR/loss_bench.json.
--ours-only skips the yardstick (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _loss_ref as R  # noqa: E402
from tdrn_amd.layers import RefineMultiBoxLoss  # noqa: E402
from tdrn_amd.utils import synth  # noqa: E402

DEV = torch.device("cuda:0")
HBM_BPS = 8.0e12
C = 21


def inputs(B, seed=0):
    priors = R.priors_of("VOC_320", os.path.join(ROOT, "tests", "golden"))
    P = priors.shape[0]
    rng = synth._rng("loss_bench", seed)
    targets = [torch.from_numpy(t).to(DEV) for t in R.synth_targets(rng, B, 1, 40, C)]
    t = lambda a: torch.from_numpy(a).to(DEV)
    arm = t((0.3 * rng.standard_normal((B, P, 4))).astype(np.float32))
    odm = t((0.5 * rng.standard_normal((B, P, 4))).astype(np.float32))
    conf = t((1.5 * rng.standard_normal((B, P, C))).astype(np.float32))
    return t(priors), targets, arm, odm, conf


# ---- yardstick: the reference's algorithm as torch ops ------------------------------------------------------------
def _point(p):
    return torch.cat([p[:, :2] - p[:, 2:] / 2, p[:, :2] + p[:, 2:] / 2], 1)


def _iou(a, b):
    lo = torch.max(a[:, None, :2], b[None, :, :2])
    hi = torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (hi - lo).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    aa = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None]
    ab = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :]
    return inter / (aa + ab - inter)


def _match(target, priors, arm):
    v0, v1 = 0.1, 0.2
    if arm is None:
        boxes, anchors = _point(priors), priors
    else:
        c = priors[:, :2] + arm[:, :2] * v0 * priors[:, 2:]
        wh = priors[:, 2:] * torch.exp(arm[:, 2:] * v1)
        boxes = torch.cat([c - wh / 2, c + wh / 2], 1)
        anchors = torch.cat([c, wh], 1)
    ov = _iou(target[:, :4], boxes)
    _, bp = ov.max(1)
    bo, bt = ov.max(0)
    bo.index_fill_(0, bp, 2)
    for j in range(bp.size(0)):
        bt[bp[j]] = j
    m = target[bt, :4]
    conf = (target[bt, 4] + 1).long()
    conf[bo < 0.5] = 0
    g = torch.cat([((m[:, :2] + m[:, 2:]) / 2 - anchors[:, :2]) / (v0 * anchors[:, 2:]),
                   torch.log((m[:, 2:] - m[:, :2]) / anchors[:, 2:]) / v1], 1)
    return g, conf


def torch_criterion(loc, conf, priors, targets, arm=None):
    B, P = loc.shape[:2]
    with torch.no_grad():
        lt, ct = zip(*[_match(targets[b], priors, None if arm is None else arm[b]) for b in range(B)])
        loc_t, conf_t = torch.stack(lt), torch.stack(ct)
    pos = conf_t > 0
    N = pos.sum().float()
    loss_l = F.smooth_l1_loss(loc[pos], loc_t[pos], reduction="sum") / N
    if conf is None:
        return loss_l
    x = conf.reshape(-1, conf.size(-1))
    xm = x.detach().max()
    s = (torch.log(torch.exp(x.detach() - xm).sum(1, keepdim=True)) + xm - x.detach().gather(1, conf_t.view(-1, 1)))
    s[pos.view(-1, 1)] = 0
    _, idx = s.view(B, -1).sort(1, descending=True)
    _, rank = idx.sort(1)
    neg = rank < torch.clamp(3 * pos.long().sum(1, keepdim=True), max=P - 1)
    used = pos | neg
    loss_c = F.cross_entropy(conf[used], conf_t[used], reduction="sum") / N
    return loss_l, loss_c


def step(kind, priors, targets, arm, odm, conf, arm_crit, crit):
    a, o, c = (t.detach().requires_grad_(True) for t in (arm, odm, conf))
    if kind == "ours":
        la = arm_crit(a, priors, targets)
        ll, lc = crit((o, c), priors, targets, arm_data=(a, None))
    else:
        la = torch_criterion(a, None, priors, targets)
        ll, lc = torch_criterion(o, c, priors, targets, a.detach())
    (la + ll + lc).backward()


def time_steps(kind, args, reps, warm=3):
    for _ in range(warm):
        step(kind, *args)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(kind, *args)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return ts


def traffic_bytes(B, P, num_pos, ntruth):
    """bytes the kernels move by shape: match reads priors (+ arm) and writes loc_t / conf_t per criterion; the ODM loss
    reads conf twice (row CE, mining score), the backward reads the selected rows again and writes grad_conf in full."""
    conf = B * P * C * 4
    match = 2 * (B * P * (16 + 16 + 16 + 4 + 8)) + ntruth * 20 * 2
    fwd = 2 * conf + B * P * (4 + 4 + 4 + 4 + 1) * 2 + num_pos * 32 * 2
    bwd = conf + 4 * (num_pos / (B * P)) * conf + B * P * 16 * 2 + B * P * (4 + 1) * 2
    return match + fwd + bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--ours-only", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    arm_crit = RefineMultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, device=DEV, only_loc=True)
    crit = RefineMultiBoxLoss(C, 0.5, True, 0, True, 3, 0.5, False, device=DEV)
    res = {"workload": "VOC_320 P=6375 C=21, ARM (only_loc) + ODM RefineMultiBoxLoss, forward + backward", "runs": {}}
    for B in [int(b) for b in a.batches.split(",")]:
        priors, targets, arm, odm, conf = inputs(B)
        args = (priors, targets, arm, odm, conf, arm_crit, crit)
        ours, yard = [], []
        for _ in range(3):                                    # alternate: ours, yardstick, ours, ...
            ours += time_steps("ours", args, a.reps // 3)
            if not a.ours_only:
                yard += time_steps("torch", args, max(1, a.reps // 9), warm=1)
        from tdrn_amd.layers.box_utils import match_targets
        _, ct = match_targets(targets, priors, 0.5, (0.1, 0.2), arm)
        num_pos = int((ct > 0).sum())
        nbytes = traffic_bytes(B, priors.size(0), num_pos, sum(int(t.size(0)) for t in targets))
        med = statistics.median(ours)
        r = {"B": B, "num_pos": num_pos, "ours_us_median": round(med, 1), "ours_us_min": round(min(ours), 1),
             "ours_us_all": [round(t, 1) for t in ours], "bytes_by_shape": int(nbytes),
             "hbm_share_at_8TBps": round(nbytes / (med * 1e-6) / HBM_BPS, 4)}
        if yard:
            r["torch_us_median"] = round(statistics.median(yard), 1)
            r["speedup"] = round(statistics.median(yard) / med, 1)
        res["runs"]["b%d" % B] = r
        print(json.dumps(r))
    with open(os.path.join(a.out, "loss_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
