"""What dynamic loss scaling adds to the optimizer step (tdrn_hip.h section i-m): one plain tdrn_amd.optim.SGD.step() against
scaler.step(optimizer) + scaler.update(), i.e. the check of all gradients, the scaled step and the update of the scale, on the
parameter list of dualrefinedet_vggbn, on the same card in the same process.

    python scripts/amp_bench.py OUT_DIR [--reps 7] [--inner 10]

The parameters come from build_net('train', 320, 21, multihead=True); the gradients are random, finite and stay in place; lr 4e-3,
momentum 0.9, weight_decay 5e-4, scale 65536.  Each variant owns a copy of the parameters.  One sample is `inner` consecutive
steps between two device events, divided by `inner`: it holds the host's share too, which is what a training loop pays;
`*_host_us` is the host's time to enqueue one step.  The two variants alternate sample by sample; the figure is the median of
`reps` samples after a discarded warm-up, with the smallest and the largest sample beside it.  Bytes are algorithmic: the plain
step reads p, g, b and writes p, b (5 x 4 x numel); the check reads g once more (6 x 4 x numel).  Writes OUT_DIR/amp.json and
OUT_DIR/amp.md, the table of DESIGN.md section 26.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tdrn_amd import _lib  # noqa: E402
from tdrn_amd.amp import GradScaler  # noqa: E402
from tdrn_amd.optim import SGD  # noqa: E402

DEV = torch.device("cuda:0")
HYPER = dict(lr=4e-3, momentum=0.9, weight_decay=5e-4)
MODEL, MODEL_KW = "dualrefinedet_vggbn", dict(multihead=True)


def make():
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3)
        net = importlib.import_module("tdrn_amd.model." + MODEL).build_net("train", 320, 21, **MODEL_KW)
    params = [torch.nn.Parameter(p.detach().to(DEV)) for p in net.parameters()]
    gen = torch.Generator(device=DEV).manual_seed(17)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device=DEV)
    return params, SGD(params, **HYPER)


def sample(step, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(inner):
        step()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner, host * 1e6 / inner


def run(reps, inner):
    (params, plain_opt), (_, scaled_opt) = make(), make()
    scaler = GradScaler().init(DEV)

    def scaled():
        scaler.step(scaled_opt)
        scaler.update()

    steps = {"plain": plain_opt.step, "scaled": scaled}
    numel = sum(p.numel() for p in params)
    times = {which: [] for which in steps}
    for step in steps.values():
        sample(step, 2)                                         # warm-up: momentum buffers, lazy initialisation
    for _ in range(reps):
        for which, step in steps.items():                       # the two alternate
            times[which].append(sample(step, inner))
    launches = -(-len(params) // _lib.SGD_TENSORS_PER_LAUNCH)
    r = {"model": MODEL, "tensors": len(params), "elements": numel, "launches_plain": launches, "launches_scaled": 2 * launches + 1,
         "bytes_plain": 5 * 4 * numel, "bytes_scaled": 6 * 4 * numel, "skipped_steps": scaler.skipped_steps(), "scale": scaler.get_scale()}
    for which, both in times.items():
        ts = [t for t, _ in both]
        r[which + "_us"], r[which + "_us_min"], r[which + "_us_max"] = statistics.median(ts), min(ts), max(ts)
        r[which + "_host_us"] = statistics.median(h for _, h in both)
        r[which + "_tbs"] = r["bytes_" + which] / r[which + "_us"] * 1e-6
    r["scaled_over_plain"] = r["scaled_us"] / r["plain_us"]
    return r


def table(r):
    return ("| variant | launches | us, median [min-max] | host us | algorithmic TB/s |\n|---|---|---|---|---|\n"
            "| plain `SGD.step()` | %d | %.1f [%.1f-%.1f] | %.0f | %.2f |\n"
            "| check + scaled step + update | %d | %.1f [%.1f-%.1f] | %.0f | %.2f |\n\nscaled / plain = %.2f\n"
            % (r["launches_plain"], r["plain_us"], r["plain_us_min"], r["plain_us_max"], r["plain_host_us"], r["plain_tbs"],
               r["launches_scaled"], r["scaled_us"], r["scaled_us_min"], r["scaled_us_max"], r["scaled_host_us"], r["scaled_tbs"],
               r["scaled_over_plain"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    r = run(a.reps, a.inner)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps, "inner": a.inner, "hyper": HYPER,
           "chunk": _lib.SGD_CHUNK, "tensors_per_launch": _lib.SGD_TENSORS_PER_LAUNCH, "result": r}
    with open(os.path.join(a.out_dir, "amp.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(a.out_dir, "amp.md"), "w") as f:
        f.write(table(r))
    print(table(r), flush=True)
    assert r["skipped_steps"] == 0, "the benchmark's gradients are finite: no step may have been skipped"


if __name__ == "__main__":
    main()
