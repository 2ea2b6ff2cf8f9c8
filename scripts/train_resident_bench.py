"""The resident training path (tdrn_hip.h section i-k) against the fp32 NCHW path, in one process.

    python scripts/train_resident_bench.py OUT_DIR [--batches 8,32] [--reps 7] [--skip-step] [--skip-layers]

Step: one forward_train + backward of dualrefinedet_vggbn at 320 px in bf16 (synthetic weights and frames, the smooth loss of
tests/_train_model_ref.py: mean squared distance of the three outputs to fixed targets), resident=False and resident=True ALTERNATING,
each sample timed between two device events after a discarded warm-up pair; the median of `reps` samples, their spread, and
torch.cuda.max_memory_allocated of a step of each kind (the peak statistics reset before it).
Layers: the conv3_2 and conv4_2 forward, backward_input (dgrad) and backward_parameters (wgrad) entries of both ABIs on the same
values, alternating the same way, one sample = 20 consecutive calls of one entry between two device events (time per call):
tdrn_conv2d_* takes and returns fp32 NCHW (its times include the staging), tdrn_conv2d_nhwc_* resident tensors; both include the
zero-page fill, the weight repack and the bias staging of every call, so `entry_share_of_mfma_peak` (the layer's flop over the time of
the whole entry call, against the dense MFMA peak figure DESIGN 6 uses) is the rate of the ENTRY, a lower bound on its conv
kernel's.  The kernel each resident launch reaches comes from tdrn_conv2d_nhwc_route.  Writes OUT_DIR/train_resident.json.  Nothing here is gated by a test.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tdrn_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
MFMA_PEAK = 2500e12
LAYER_CALLS = 20                                                       # consecutive entry calls in one timed window
LAYERS = {"conv3_2": (256, 256, 80), "conv4_2": (512, 512, 40)}        # Cin, Cout, map; 3x3, pad 1


def timed(fn, calls):
    """`calls` back-to-back calls between two device events -> us per call.  With several calls in the window the device stays busy
    and the host's enqueue latency of the first launches is amortised; with one, it is part of the figure."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def alternate(fns, reps, calls=1):
    """{name: fn} -> {name: {median_us, min_us, max_us}} per call: one discarded warm-up round, then `reps` rounds in the same order,
    each sample `calls` consecutive calls"""
    for fn in fns.values():
        fn()
    samples = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            samples[k].append(timed(fn, calls))
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "samples": len(v)} for k, v in samples.items()}


def step_bench(B, reps):
    from tdrn_amd.model.dualrefinedet_vggbn import build_net
    from tdrn_amd.utils import synth
    net = build_net("train", 320, 21, 1024, 1, True, False)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(DEV).train()
    x = torch.from_numpy(synth.synth_frames(B, 320, seed=5)).to(DEV)
    P = 3 * (40 * 40 + 20 * 20 + 10 * 10 + 5 * 5)
    gen = torch.Generator().manual_seed(77)
    targets = [torch.randn(B, P, w, generator=gen).to(DEV) for w in (4, 4, 21)]

    def step(resident):
        def run():
            net.zero_grad(set_to_none=True)
            out = net.forward_train(x, "bf16", resident=resident)
            sum(((o - t) ** 2).mean() for o, t in zip((out[0], out[2], out[3]), targets)).backward()
        return run
    fns = {"resident_false": step(False), "resident_true": step(True)}
    res = alternate(fns, reps)
    for k, fn in fns.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        fn()
        torch.cuda.synchronize()
        res[k]["max_memory_allocated_bytes"] = int(torch.cuda.max_memory_allocated(DEV))
    res["speedup"] = res["resident_false"]["median_us"] / res["resident_true"]["median_us"]
    return res


def layer_bench(name, B, reps):
    from tdrn_amd.model import networks
    Cin, Cout, S = LAYERS[name]
    lib, dt, st = _lib.lib(), _lib.BF16, _lib.current_stream(DEV)
    dims = (B, Cin, S, S, Cout, 3, 3, 1, 1, 1, 1, 1, 1)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(B, Cin, S, S, generator=gen).to(DEV)
    w = (torch.randn(Cout, Cin, 3, 3, generator=gen) * (Cin * 9) ** -0.5).to(DEV)
    go = torch.randn(B, Cout, S, S, generator=gen).to(DEV)
    out, gi, gw = torch.empty_like(go), torch.empty_like(x), torch.zeros_like(w)
    xr, gor = networks.to_nhwc(x, "bf16"), networks.to_nhwc(go, "bf16")
    outr, gir = torch.empty_like(gor), torch.empty_like(xr)
    nb = lib.tdrn_conv2d_workspace_bytes(*dims, dt)
    nbr = lib.tdrn_conv2d_nhwc_workspace_bytes(*dims, dt, 0)
    assert nb > 0 and nbr > 0
    ws, wsr = torch.empty(nb, dtype=torch.uint8, device=DEV), torch.empty(nbr, dtype=torch.uint8, device=DEV)
    p = _lib.ptr
    fns = {
        "forward_nchw": lambda: _lib.check(lib.tdrn_conv2d_forward(p(x), p(w), None, p(out), *dims, dt, p(ws), nb, st)),
        "forward_nhwc": lambda: _lib.check(lib.tdrn_conv2d_nhwc_forward(p(xr), p(w), None, p(outr), *dims, dt, p(wsr), nbr, st, 0)),
        "dgrad_nchw": lambda: _lib.check(lib.tdrn_conv2d_backward_input(p(go), p(w), p(gi), *dims, dt, p(ws), nb, st)),
        "dgrad_nhwc": lambda: _lib.check(lib.tdrn_conv2d_nhwc_backward_input(p(gor), p(w), p(gir), *dims, dt, p(wsr), nbr, st, 0)),
        "wgrad_nchw": lambda: _lib.check(lib.tdrn_conv2d_backward_parameters(p(x), p(go), p(gw), None, *dims, 1.0, dt, p(ws), nb, st)),
        "wgrad_nhwc": lambda: _lib.check(lib.tdrn_conv2d_nhwc_backward_parameters(p(xr), p(gor), p(gw), None, *dims, 1.0, dt, p(wsr), nbr,
                                                                                  st, 0)),
    }
    res = alternate(fns, reps, LAYER_CALLS)
    flop = 2.0 * B * S * S * Cout * Cin * 9
    for v in res.values():
        v["entry_share_of_mfma_peak"] = flop / (v["median_us"] * 1e-6) / MFMA_PEAK        # of the whole entry call, not of its conv kernel
    res["route"] = {"forward": lib.tdrn_conv2d_nhwc_route(*dims, dt, 0, 0).decode(), "dgrad": lib.tdrn_conv2d_nhwc_route(*dims, dt, 0, 1).decode()}
    res["workspace_bytes"] = {"nchw": nb, "nhwc": nbr}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-layers", action="store_true")
    a = ap.parse_args()
    assert a.reps >= 5
    os.makedirs(a.out_dir, exist_ok=True)
    result = {"device": torch.cuda.get_device_name(0), "version": _lib.lib().tdrn_version().decode(), "reps": a.reps, "step": {}, "layers": {}}
    for B in (int(b) for b in a.batches.split(",")):
        if not a.skip_layers:
            result["layers"]["batch_%d" % B] = {name: layer_bench(name, B, a.reps) for name in LAYERS}
        if not a.skip_step:
            result["step"]["batch_%d" % B] = step_bench(B, a.reps)
        print(json.dumps({k: result[k].get("batch_%d" % B) for k in ("step", "layers")}), flush=True)
    with open(os.path.join(a.out_dir, "train_resident.json"), "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
