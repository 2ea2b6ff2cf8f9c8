"""tdrn_amd.optim.SGD (tdrn_hip.h section i-j) on the five real parameter sets, against torch.optim.SGD(foreach=True) and
torch.optim.SGD(fused=True) on the same card in the same process.

    python scripts/sgd_bench.py OUT_DIR [--reps 9] [--inner 10] [--models dualrefinedet_vggbn,...]

Each model's parameters come from build_net('train', 320, 21) (dualrefinedet_vggbn with multihead=True as well); the gradients are
random and stay in place; lr 4e-3, momentum 0.9, weight_decay 5e-4, the reference's values.  Every optimizer owns a copy of the
parameters.  One sample is `inner` consecutive step() calls between two device events, divided by `inner`: it holds the host's
share too, which is what a training loop pays; `*_host_us` is the host's time to enqueue one step (perf_counter around the same
calls, before the synchronisation).  The three optimizers alternate sample by sample; the figure is the median of
`reps` samples after a discarded warm-up.  Bytes are algorithmic: p, g and b read, p and b written = 5 x 4 x numel; the rate is their
quotient with the step's time, against bench.py's HBM_PEAK_GBS.  A set below 256 MiB in total can be served from the Infinity
Cache (`fits_infinity_cache`).  Launches: ours is ceil(tensors / TDRN_SGD_TENSORS_PER_LAUNCH) by construction; for torch's the
script counts the device-side events of one step under torch's profiler after the timings (null when the profiler gives nothing).
That count is an upper bound on kernels: it has shown one event more than ours launches (`launches_ours_profiled`).  Writes
OUT_DIR/sgd.json and OUT_DIR/sgd.md, the table of DESIGN.md section 21.
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
from tdrn_amd.optim import SGD  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK_GBS = 8000.0           # bench.py's figure
HYPER = dict(lr=4e-3, momentum=0.9, weight_decay=5e-4)
MODELS = {"dualrefinedet_vggbn": dict(multihead=True), "dualrefinedet_mobilenet": {}, "ssd4scale_vgg": {}, "ssd4scale_mobile": {},
          "refinedet_vgg": {}}


def make(model, which):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3)
        net = importlib.import_module("tdrn_amd.model." + model).build_net("train", 320, 21, **MODELS[model])
    params = [torch.nn.Parameter(p.detach().to(DEV)) for p in net.parameters()]
    gen = torch.Generator(device=DEV).manual_seed(17)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device=DEV)
    if which == "ours":
        return params, SGD(params, **HYPER)
    return params, torch.optim.SGD(params, foreach=(which == "foreach"), fused=(which == "fused") or None, **HYPER)


def sample(opt, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(inner):
        opt.step()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner, host * 1e6 / inner


def kernel_launches(opt):
    """device-side events of one step, from torch's profiler (kernels, and whatever else it lists there); None when it gives nothing"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            opt.step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception as exc:          # a measurement aid only: the timings above stand without it
        print("profiler: %r" % (exc,), flush=True)
        return None


def run(model, reps, inner):
    sets = {which: make(model, which) for which in ("ours", "foreach", "fused")}
    params = sets["ours"][0]
    numel = sum(p.numel() for p in params)
    nbytes = 5 * 4 * numel
    times = {which: [] for which in sets}
    for which, (_, opt) in sets.items():
        sample(opt, 2)                                          # warm-up: momentum buffers, lazy initialisation
    for _ in range(reps):
        for which, (_, opt) in sets.items():                    # the three alternate
            times[which].append(sample(opt, inner))
    r = {"tensors": len(params), "elements": numel, "algorithmic_bytes": nbytes, "fits_infinity_cache": nbytes < (256 << 20),
         "launches_ours": -(-len(params) // _lib.SGD_TENSORS_PER_LAUNCH)}
    for which, both in times.items():
        ts = [t for t, _ in both]
        r[which + "_host_us"] = statistics.median(h for _, h in both)
        us = statistics.median(ts)
        r[which + "_us"], r[which + "_us_min"], r[which + "_us_max"] = us, min(ts), max(ts)
        r[which + "_tbs"] = nbytes / us * 1e-6
        r[which + "_fraction_of_hbm_peak"] = nbytes / us * 1e-3 / HBM_PEAK_GBS
    r["ours_over_foreach"], r["ours_over_fused"] = r["ours_us"] / r["foreach_us"], r["ours_us"] / r["fused_us"]
    return r, sets


def table(res):
    rows = ["| model | tensors | elements | ours us (launches; host us) | foreach us (profiled device events; host us) "
            "| fused us (profiled device events; host us) | ours TB/s | ours / fused |", "|---|---|---|---|---|---|---|---|"]
    for name, r in res["results"].items():
        rows.append("| %s | %d | %d | %.1f (%d; %.0f) | %.1f (%s; %.0f) | %.1f (%s; %.0f) | %.2f | %.2f |" % (
            name, r["tensors"], r["elements"], r["ours_us"], r["launches_ours"], r["ours_host_us"], r["foreach_us"],
            r.get("launches_foreach") or "n/a", r["foreach_host_us"], r["fused_us"], r.get("launches_fused") or "n/a",
            r["fused_host_us"], r["ours_tbs"], r["ours_over_fused"]))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-profiler", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps, "inner": a.inner,
           "hbm_peak_gbs": HBM_PEAK_GBS, "hyper": HYPER, "chunk": _lib.SGD_CHUNK, "tensors_per_launch": _lib.SGD_TENSORS_PER_LAUNCH,
           "results": {}}

    def write():
        with open(os.path.join(a.out_dir, "sgd.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "sgd.md"), "w") as f:
            f.write(table(res))

    for name in a.models.split(","):
        r, sets = run(name, a.reps, a.inner)
        res["results"][name] = r
        write()
        print("%-24s %3d tensors %9d el  ours %7.1f us (%d launches, %.2f TB/s, host %.0f)  foreach %7.1f us (host %.0f)  fused %7.1f us "
              "(host %.0f)  ours/fused %.2f" % (name, r["tensors"], r["elements"], r["ours_us"], r["launches_ours"], r["ours_tbs"],
                                                r["ours_host_us"], r["foreach_us"], r["foreach_host_us"], r["fused_us"], r["fused_host_us"],
                                                r["ours_over_fused"]), flush=True)
        if not a.no_profiler:
            for which in ("foreach", "fused", "ours"):
                r["launches_" + which + ("_profiled" if which == "ours" else "")] = kernel_launches(sets[which][1])
            write()
            print("%-24s launches profiled: ours %s foreach %s fused %s" % (name, r["launches_ours_profiled"], r["launches_foreach"],
                                                                           r["launches_fused"]), flush=True)
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
