"""TRN pair augmentation: device time of PairSSDAugmentation.batch (tdrn_hip.h section ii-d) beside the two single-frame
kernels launched twice on the same frames, and the numpy restatement of the pair chain on one CPU core (one DataLoader worker
running the reference's pull_translational_item + pairSSDAugmentation).

    python scripts/augment_pair_bench.py OUT_DIR [--sizes 320] [--batch 32] [--reps 51] [--cpu-images 16] [--device-only]

Workload: augment_bench.py's (B frames of 300 to 500 px a side, 1 to 8 truths each, Philox draws); the second frame is the
translated first.  Device times are the median over `reps` of event pairs around each call: the pair sampler, the pair apply,
the whole batch() (host-side table packing and uploads included), and SSDAugmentation's sample / apply called twice in a row.
Writes OUT_DIR/augment_pair_bench.json.  --device-only skips the CPU yardstick (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import _augment_pair_ref as P  # noqa: E402
from augment_bench import DEV, MEAN, timed, workload  # noqa: E402
from tdrn_amd.utils.augmentations import PairSSDAugmentation, SSDAugmentation  # noqa: E402


def device_run(S, B, reps):
    imgs, targets = workload(B)
    dimgs = [torch.from_numpy(im).to(DEV) for im in imgs]
    tt = [torch.from_numpy(t).float() for t in targets]
    pair, single = PairSSDAugmentation(S, MEAN, seed=1), SSDAugmentation(S, MEAN, seed=1)
    hw = [im.shape[:2] for im in imgs]
    ids = list(range(B))
    qparams = pair.sample(hw, tt, DEV, sample_ids=ids)[0]
    sparams = single.sample(hw, tt, DEV, sample_ids=ids)[0]
    out, out_t = torch.empty(B, 3, S, S, device=DEV), torch.empty(B, 3, S, S, device=DEV)
    for _ in range(5):
        pair.batch(dimgs, tt, ids)
        single.batch(dimgs, tt, ids)
    torch.cuda.synchronize()

    def twice(fn):
        return lambda: (fn(), fn())
    t = dict(pair_sample=timed(lambda: pair.sample(hw, tt, DEV, sample_ids=ids), reps),
             pair_apply=timed(lambda: pair.apply(dimgs, qparams, out=out, out_t=out_t), reps),
             pair_batch=timed(lambda: pair.batch(dimgs, tt, ids), reps),
             single_sample_x2=timed(twice(lambda: single.sample(hw, tt, DEV, sample_ids=ids)), reps),
             single_apply_x2=timed(twice(lambda: single.apply(dimgs, sparams, out=out)), reps),
             single_batch_x2=timed(twice(lambda: single.batch(dimgs, tt, ids)), reps))
    d = dict(S=S, B=B, out_MB=2 * B * 3 * S * S * 4 / 1e6, src_MB=sum(im.nbytes for im in imgs) / 1e6)
    for k, (med, lo) in t.items():
        d[k + "_us_median"], d[k + "_us_min"] = med, lo
    d["pairs_per_s_batch"] = B / (t["pair_batch"][0] * 1e-6)
    d["pair_apply_out_GBps"] = d["out_MB"] * 1e-3 / (t["pair_apply"][0] * 1e-6)
    return d


def cpu_run(S, n):
    torch.set_num_threads(1)
    imgs, targets = workload(n, seed=1)
    t0 = time.perf_counter()
    for i, (im, t) in enumerate(zip(imgs, targets)):
        p = P.sample_pair(im.shape[1], im.shape[0], t[:, :4], t[:, 4], np.random.RandomState(i))[0]
        P.apply_pair(im, p, S, MEAN, to_rgb=True)
    dt = time.perf_counter() - t0
    return dict(S=S, pairs=n, seconds=dt, pairs_per_s=n / dt, ms_per_pair=dt / n * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--sizes", default="320")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=51)
    ap.add_argument("--cpu-images", type=int, default=16)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    res = dict(device=torch.cuda.get_device_name(0), runs=[])
    for S in [int(s) for s in a.sizes.split(",")]:
        d = device_run(S, a.batch, a.reps)
        if not a.device_only:
            d["cpu_one_core"] = cpu_run(S, a.cpu_images)
        res["runs"].append(d)
        print(json.dumps(d))
    with open(os.path.join(a.out, "augment_pair_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
