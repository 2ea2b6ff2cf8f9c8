"""The depthwise 3x3 conv with gradients (tdrn_hip.h section i-h): timings of forward, backward_input (dgrad) and
backward_parameters (wgrad) on the depthwise layers of the MobileNet trunk at 320 px, stride 1 and 2, against the vendor library
through torch in the same process; and one forward_train + backward step of dualrefinedet_mobilenet.  Reported, not gated.

    python scripts/dwconv_bench.py OUT_DIR [--batches 8,32] [--reps 5] [--layers dw32s1,...] [--step-batch 8] [--step-size 320]
                                           [--step-modes fp32,bf16] [--no-step]

Each entry is timed between two device events: the median of `reps` repeats after a discarded warm-up, ours and the yardstick
alternating.  The yardstick is F.conv2d(groups=C) and torch.ops.aten.convolution_backward with one output masked in, on the same
fp32 NCHW tensors.  The op is bandwidth-bound, so each entry also gets its achieved GB/s against the bytes it cannot avoid: forward
reads the input and writes the output; dgrad reads grad_output and writes grad_input; wgrad reads both (the nine weights per channel
are left out).  The training step runs every layer on fp32 NCHW tensors with the layout conversions of every dense op inside it: it
is the time of the composition as it stands, not of a tuned training path.  Writes OUT_DIR/dwconv.json.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tdrn_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")

# name: channels, input map at 320 px, stride -- the distinct depthwise layers of mobilenet_backbone and the two extras blocks
LAYERS = {"dw32s1": (32, 160, 1), "dw64s2": (64, 160, 2), "dw128s1": (128, 80, 1), "dw256s1": (256, 80, 1), "dw256s2": (256, 80, 2),
          "dw512s1": (512, 40, 1), "dw512s2": (512, 40, 2), "dw1024s1": (1024, 20, 1), "extras0s2": (256, 20, 2), "extras1s2": (256, 10, 2)}


def timed(fn, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


class Layer:
    def __init__(self, name, B, seed):
        C, S, s = LAYERS[name]
        So = (S - 1) // s + 1
        gen = torch.Generator(device="cpu").manual_seed(seed)
        self.C, self.s = C, s
        self.x = torch.randn(B, C, S, S, generator=gen).to(DEV)
        self.w = (torch.randn(C, 1, 3, 3, generator=gen) / 3).to(DEV)
        self.go = torch.randn(B, C, So, So, generator=gen).to(DEV)
        self.dims = (B, C, S, S, 3, 3, s, s, 1, 1, 1, 1)
        self.lib, self.dt = _lib.lib(), _lib.F32
        self.nb = self.lib.tdrn_dwconv2d_workspace_bytes(*self.dims, self.dt)
        assert self.nb > 0, self.dims
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)
        self.out, self.gi, self.gw = torch.empty_like(self.go), torch.empty_like(self.x), torch.zeros_like(self.w)
        self.st = _lib.current_stream(DEV)
        nx, ny = 4 * self.x.numel(), 4 * self.go.numel()
        self.bytes = {"forward": nx + ny, "dgrad": nx + ny, "wgrad": nx + ny}

    def fwd(self):
        _lib.check(self.lib.tdrn_dwconv2d_forward(_lib.ptr(self.x), _lib.ptr(self.w), None, _lib.ptr(self.out), *self.dims, self.dt,
                                                  _lib.ptr(self.ws), self.nb, self.st))

    def dgrad(self):
        _lib.check(self.lib.tdrn_dwconv2d_backward_input(_lib.ptr(self.go), _lib.ptr(self.w), _lib.ptr(self.gi), *self.dims, self.dt,
                                                         _lib.ptr(self.ws), self.nb, self.st))

    def wgrad(self):
        _lib.check(self.lib.tdrn_dwconv2d_backward_parameters(_lib.ptr(self.x), _lib.ptr(self.go), _lib.ptr(self.gw), None, *self.dims,
                                                              1.0, self.dt, _lib.ptr(self.ws), self.nb, self.st))

    def _bwd(self, mask):
        s = self.s
        return torch.ops.aten.convolution_backward(self.go, self.x, self.w, None, [s, s], [1, 1], [1, 1], False, [0, 0], self.C, mask)

    def t_fwd(self):
        return F.conv2d(self.x, self.w, None, self.s, 1, 1, self.C)

    def t_dgrad(self):
        return self._bwd([True, False, False])[0]

    def t_wgrad(self):
        return self._bwd([False, True, False])[1]


def run(name, B, reps):
    L = Layer(name, B, seed=7)
    pairs = (("forward", L.fwd, L.t_fwd), ("dgrad", L.dgrad, L.t_dgrad), ("wgrad", L.wgrad, L.t_wgrad))
    ts = {}
    for key, ours, yard in pairs:
        a, b = [], []
        for _ in range(reps):                 # ours and the yardstick alternate
            a.append(timed(ours))
            b.append(timed(yard))
        ts[key + "_us"], ts["torch_" + key + "_us"] = statistics.median(a), statistics.median(b)
        ts[key + "_gbps"] = L.bytes[key] / ts[key + "_us"] * 1e-3
        ts["torch_" + key + "_gbps"] = L.bytes[key] / ts["torch_" + key + "_us"] * 1e-3
        ts[key + "_over_torch"] = ts[key + "_us"] / ts["torch_" + key + "_us"]
    # agreement with the yardstick (not a test: the tests compare with float64)
    L.gw.zero_()
    L.fwd(); L.dgrad(); L.wgrad()
    diffs = {}
    for key, got, ref in (("forward", L.out, L.t_fwd()), ("dgrad", L.gi, L.t_dgrad()), ("wgrad", L.gw, L.t_wgrad())):
        diffs[key] = float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    ts["max_rel_diff_vs_torch"] = diffs
    ts["compulsory_bytes"], ts["workspace_bytes"] = L.bytes, L.nb
    return ts


def train_step(B, size, mode, reps):
    """one forward_train + backward of the smooth test loss (mean square of the outputs), synthetic weights"""
    from tdrn_amd.model.dualrefinedet_mobilenet import build_net
    from tdrn_amd.utils import synth
    net = build_net("train", 320, 21, 1, False)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(DEV)
    x = torch.from_numpy(synth.synth_frames(B, size, seed=5)).to(DEV)

    def step():
        net.zero_grad(set_to_none=True)
        out = net.forward_train(x, mode)
        (out[0].pow(2).mean() + out[2].pow(2).mean() + out[3].pow(2).mean()).backward()

    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ts = [timed(step, warm=0) for _ in range(reps)]
    return {"batch": B, "size": size, "compute": mode, "step_ms": statistics.median(ts) * 1e-3,
            "peak_memory_mib": torch.cuda.max_memory_allocated() / 2 ** 20}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--layers", default=",".join(LAYERS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--step-size", type=int, default=320)
    ap.add_argument("--step-modes", default="fp32,bf16")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "results": {}, "train_step": {}}

    def save():
        with open(os.path.join(a.out_dir, "dwconv.json"), "w") as f:
            json.dump(res, f, indent=1)

    for B in (int(v) for v in a.batches.split(",")):
        for name in a.layers.split(","):
            r = run(name, B, a.reps)
            res["results"]["%s_b%d" % (name, B)] = r
            print("%-9s b%-3d fwd %7.1f us %6.0f GB/s (torch %7.1f)  dgrad %7.1f %6.0f (%7.1f)  wgrad %7.1f %6.0f (%7.1f)  diff %s" % (
                name, B, r["forward_us"], r["forward_gbps"], r["torch_forward_us"], r["dgrad_us"], r["dgrad_gbps"], r["torch_dgrad_us"],
                r["wgrad_us"], r["wgrad_gbps"], r["torch_wgrad_us"], {k: "%.1e" % v for k, v in r["max_rel_diff_vs_torch"].items()}),
                flush=True)
            save()
    if not a.no_step:
        for mode in a.step_modes.split(","):
            r = train_step(a.step_batch, a.step_size, mode, a.reps)
            res["train_step"]["%dpx_b%d_%s" % (a.step_size, a.step_batch, mode)] = r
            print("forward_train + backward, %d px, batch %d, %s: %.1f ms, peak memory %.0f MiB" % (
                a.step_size, a.step_batch, mode, r["step_ms"], r["peak_memory_mib"]), flush=True)
            save()


if __name__ == "__main__":
    main()
