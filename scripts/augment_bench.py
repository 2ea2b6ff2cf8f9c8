"""Training augmentation: device time of SSDAugmentation.batch (tdrn_hip.h section ii-c) against the numpy restatement on one
CPU core, the stand-in for one DataLoader worker running the reference's per-sample SSDAugmentation.

    python scripts/augment_bench.py OUT_DIR [--sizes 320,512] [--batch 32] [--reps 51] [--cpu-images 16] [--device-only]

Workload: B frames of mixed VOC-like sizes (300 to 500 px a side), 1 to 8 truths each, Philox draws.  Device times are the
median over `reps` of event pairs around each launch (sample alone, apply alone) and around the whole batch() call
(host-side table packing and the pinned uploads included).  The CPU yardstick runs tests/_augment_ref.py (the same
decisions from numpy's RandomState, and the pixels through a materialised distort / canvas / crop / resize, as the
reference does) on `cpu-images` frames with one thread.  Writes OUT_DIR/augment_bench.json.
--device-only skips the CPU yardstick (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _augment_ref as R  # noqa: E402
from tdrn_amd.utils.augmentations import SSDAugmentation  # noqa: E402

DEV = torch.device("cuda:0")
MEAN = (104, 117, 123)


def workload(B, seed=0):
    rs = np.random.RandomState(seed)
    imgs, targets = [], []
    for b in range(B):
        H, W = int(rs.randint(300, 501)), int(rs.randint(300, 501))
        imgs.append(R.case_image(H, W, seed * 1000 + b))
        targets.append(R.case_boxes(H, W, int(rs.randint(1, 9)), seed * 1000 + b))
    return imgs, targets


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


def device_run(S, B, reps):
    imgs, targets = workload(B)
    dimgs = [torch.from_numpy(im).to(DEV) for im in imgs]
    tt = [torch.from_numpy(t).float() for t in targets]
    aug = SSDAugmentation(S, MEAN, seed=1)
    hw = [im.shape[:2] for im in imgs]
    ids = list(range(B))
    params, _ = aug.sample(hw, tt, DEV, sample_ids=ids)
    out = torch.empty(B, 3, S, S, device=DEV)
    for _ in range(5):
        aug.batch(dimgs, tt, ids)
    torch.cuda.synchronize()
    sample_us = timed(lambda: aug.sample(hw, tt, DEV, sample_ids=ids), reps)
    apply_us = timed(lambda: aug.apply(dimgs, params, out=out), reps)
    batch_us = timed(lambda: aug.batch(dimgs, tt, ids), reps)
    out_mb = B * 3 * S * S * 4 / 1e6
    src_mb = sum(im.nbytes for im in imgs) / 1e6
    return dict(S=S, B=B, sample_us_median=sample_us[0], sample_us_min=sample_us[1], apply_us_median=apply_us[0],
                apply_us_min=apply_us[1], batch_us_median=batch_us[0], batch_us_min=batch_us[1],
                images_per_s_kernels=B / ((sample_us[0] + apply_us[0]) * 1e-6), images_per_s_batch=B / (batch_us[0] * 1e-6),
                out_MB=out_mb, src_MB=src_mb, apply_out_GBps=out_mb * 1e-3 / (apply_us[0] * 1e-6))


def cpu_run(S, n):
    torch.set_num_threads(1)
    imgs, targets = workload(n, seed=1)
    t0 = time.perf_counter()
    for i, (im, t) in enumerate(zip(imgs, targets)):
        p, _, _ = R.sample(im.shape[1], im.shape[0], t[:, :4], t[:, 4], np.random.RandomState(i))
        R.apply(im, p, S, MEAN, to_rgb=True)
    dt = time.perf_counter() - t0
    return dict(S=S, images=n, seconds=dt, images_per_s=n / dt, ms_per_image=dt / n * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--sizes", default="320,512")
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
            c = cpu_run(S, a.cpu_images)
            d["cpu_one_core"] = c
            d["speedup_per_image_vs_one_core"] = d["images_per_s_kernels"] / c["images_per_s"]
        res["runs"].append(d)
        print(json.dumps(d))
    with open(os.path.join(a.out, "augment_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
