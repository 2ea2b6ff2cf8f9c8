"""Transform-domain deformable conv (tdrn_hip.h section i-l) against the gather op, in one process.

    python scripts/deform_ts_bench.py OUT_DIR [--batches 8,32] [--reps 7] [--skip-step] [--skip-sets] [--step-only VARIANT]

Sets (scripts/deform_backward_bench.py's): the ODM heads of dualrefinedet_vggbn at 320 px (levels 40/20/10/5, Cin
256, G = 1; loc 12 and conf 63 columns; 3x3 alone, and 3x3 + 5x5 = multihead) and the two TRN sets (G = 8), which only confirm the
refusal.  Per set the Python ops run back to back on the same inputs, forward (with an autograd graph) and backward timed apart between
two device events: "gather" = conv_offset2d(compute="bf16") per head, the yardstick; "transform_paired" = one conv_offset2d_ts over the
concatenated loc + conf weight per (level, kernel), what forward_train(deform_algo="transform") runs; "transform_unpaired" = one call
per head; "transform_paired_recompute" = paired with ConvOffset2dTsFunction.save_y = False.  The variants alternate; the median of
`reps` samples after a discarded warm-up round is reported with min and max.
Step: one forward_train + backward of dualrefinedet_vggbn at 320 px, bf16, for deform_algo x resident.
Writes OUT_DIR/deform_ts.json."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tdrn_amd import _lib  # noqa: E402
from tdrn_amd.model import networks  # noqa: E402

DEV = torch.device("cuda:0")
LEVELS = (40, 20, 10, 5)
ODM_SETS = {"odm_3x3": (3,), "odm_3x3_5x5": (3, 5)}
TRN_SET = [(cin, s, c, 3, 8) for cin, s in ((512, 20), (1024, 10), (512, 5), (512, 3)) for c in (12, 63)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stats(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "samples": len(v)}


def set_bench(ks, B, reps):
    gen = torch.Generator().manual_seed(11)
    members = []
    for s in LEVELS:
        x = torch.randn(B, 256, s, s, generator=gen).to(DEV).requires_grad_(True)
        for k in ks:
            off = (0.5 * torch.randn(B, 2 * k * k, s, s, generator=gen)).to(DEV).requires_grad_(True)
            wl, wc = ((torch.randn(c, 256, k, k, generator=gen) * (256 * k * k) ** -0.5).to(DEV).requires_grad_(True) for c in (12, 63))
            gl, gc = (torch.randn(B, c, s, s, generator=gen).to(DEV) for c in (12, 63))
            members.append((x, off, wl, wc, gl, gc, k))

    def gather():
        return [(networks.conv_offset2d(x, off, w, 1, k // 2, 1, 1, "bf16"), g) for x, off, wl, wc, gl, gc, k in members
                for w, g in ((wl, gl), (wc, gc))]

    def unpaired():
        return [(networks.conv_offset2d_ts(x, off, w, 1, k // 2, 1, "bf16"), g) for x, off, wl, wc, gl, gc, k in members
                for w, g in ((wl, gl), (wc, gc))]

    def paired():
        return [(networks.conv_offset2d_ts(x, off, torch.cat([wl, wc]), 1, k // 2, 1, "bf16"), torch.cat([gl, gc], 1))
                for x, off, wl, wc, gl, gc, k in members]

    def recompute():
        networks.ConvOffset2dTsFunction.save_y = False
        try:
            return paired()
        finally:
            networks.ConvOffset2dTsFunction.save_y = True

    variants = {"gather": gather, "transform_paired": paired, "transform_unpaired": unpaired, "transform_paired_recompute": recompute}
    samples = {k: {"forward": [], "backward": [], "sum": []} for k in variants}
    for r in range(reps + 1):
        for name, fwd in variants.items():
            for m in members:
                for t in m[:4]:
                    t.grad = None
            kept = []
            tf = timed(lambda: kept.extend(fwd()))
            outs, gos = [o for o, _ in kept], [g for _, g in kept]
            tb = timed(lambda: torch.autograd.backward(outs, gos))
            if r:                                   # round 0 is the warm-up
                samples[name]["forward"].append(tf)
                samples[name]["backward"].append(tb)
                samples[name]["sum"].append(tf + tb)
    res = {name: {part: stats(v) for part, v in s.items()} for name, s in samples.items()}
    for name in res:
        res[name]["sum_vs_gather"] = res["gather"]["sum"]["median_us"] / res[name]["sum"]["median_us"]
    return res


def trn_refusal(B):
    lib = _lib.lib()
    return {"members": len(TRN_SET),
            "refused": sum(lib.tdrn_deform_conv_ts_workspace_bytes(B, cin, s, s, c, k, k, 1, 1, k // 2, k // 2, 1, 1, G, _lib.BF16) == 0
                           for cin, s, c, k, G in TRN_SET)}


def step_bench(B, reps, only=None):
    from tdrn_amd.model.dualrefinedet_vggbn import build_net
    from tdrn_amd.utils import synth
    net = build_net("train", 320, 21, 1024, 1, True, False)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(DEV).train()
    x = torch.from_numpy(synth.synth_frames(B, 320, seed=5)).to(DEV)
    P = 3 * sum(s * s for s in LEVELS)
    gen = torch.Generator().manual_seed(77)
    targets = [torch.randn(B, P, w, generator=gen).to(DEV) for w in (4, 4, 21)]

    def step(algo, resident):
        def run():
            net.zero_grad(set_to_none=True)
            out = net.forward_train(x, "bf16", resident=resident, deform_algo=algo)
            sum(((o - t) ** 2).mean() for o, t in zip((out[0], out[2], out[3]), targets)).backward()
        return run

    fns = {"%s_resident_%s" % (a, r): step(a, r) for a in ("gather", "transform") for r in (False, True)}
    if only:                                        # one variant alone: what a kernel trace of the step wants
        fns = {only: fns[only]}
    samples = {k: [] for k in fns}
    for r in range(reps + 1):
        for k, fn in fns.items():
            t = timed(fn)
            if r:
                samples[k].append(t)
    return {k: stats(v) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-sets", action="store_true")
    ap.add_argument("--step-only", default=None, help="time this step variant alone, e.g. transform_resident_True")
    a = ap.parse_args()
    assert a.reps >= 5
    os.makedirs(a.out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "library": _lib.lib().tdrn_version().decode(), "reps": a.reps, "sets": {}, "step": {}}
    for B in (int(b) for b in a.batches.split(",")):
        if not a.skip_sets:
            res["sets"]["batch_%d" % B] = {name: set_bench(ks, B, a.reps) for name, ks in ODM_SETS.items()}
            res["sets"]["batch_%d" % B]["trn"] = trn_refusal(B)
        if not a.skip_step:
            res["step"]["batch_%d" % B] = step_bench(B, a.reps, a.step_only)
        with open(os.path.join(a.out_dir, "deform_ts.json"), "w") as f:        # (kept after every batch)
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
