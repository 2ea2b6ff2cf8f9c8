"""The dense 3x3 stride-2 conv with gradients (tdrn_hip.h section i-g): timings of forward, backward_input (dgrad, by zero
insertion) and backward_parameters (wgrad) on the `extras` layer of dualrefinedet_vggbn (256 -> 512 channels, 10x10 -> 5x5 at
320 px, 16x16 -> 8x8 at 512 px), against the vendor library through torch in the same process; and one RefineSSD.forward_train +
backward step.  Reported, not gated.

    python scripts/conv_strided_bench.py OUT_DIR [--batches 8,32] [--modes bf16,fp32] [--reps 5] [--layers extras320,extras512]
                                                 [--step-batch 8] [--step-size 320] [--no-step]

Each entry is timed between two device events: the median of `reps` repeats after a discarded warm-up, ours and the yardstick
alternating.  Our entries take and return fp32 NCHW tensors, so their times include the layout conversions, the weight packing
and wgrad's reduce; the yardstick (F.conv2d, torch.ops.aten.convolution_backward with one output masked in) runs on the same values
held in the compute type (bf16 tensors for bf16, fp32 for fp32).  Rates: 2 N Ho Wo 9 Cout Cin flop per product (the useful ones:
the zero-inserted input gradient issues about four times as many), against the dense MFMA peak figures DESIGN 6 uses.
The training step runs every layer on fp32 NCHW tensors with the layout conversions of every op inside it: it is the time of the
composition as it stands, not of a tuned training path.  Writes OUT_DIR/conv_strided.json.
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
MFMA_PEAK = {"bf16": 2500e12, "fp16": 2500e12, "fp32": 157.3e12}       # the figures of DESIGN 6 / bench.py
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}

# name: Cin, Cout, S (the input map; the output is S/2 x S/2), pad
LAYERS = {"extras320": (256, 512, 10, 1), "extras512": (256, 512, 16, 1)}


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
    def __init__(self, name, B, mode, seed):
        Cin, Cout, S, pad = LAYERS[name]
        So = (S + 2 * pad - 3) // 2 + 1
        gen = torch.Generator(device="cpu").manual_seed(seed)
        self.mode, self.pad = mode, pad
        self.x = torch.randn(B, Cin, S, S, generator=gen).to(DEV)
        self.w = (torch.randn(Cout, Cin, 3, 3, generator=gen) * (9 * Cin) ** -0.5).to(DEV)
        self.go = torch.randn(B, Cout, So, So, generator=gen).to(DEV)
        self.dims = (B, Cin, S, S, Cout, 3, 3, 2, 2, pad, pad, 1, 1)
        self.lib, self.dt = _lib.lib(), _lib.DTYPES[mode]
        self.nb = self.lib.tdrn_conv2d_strided_workspace_bytes(*self.dims, self.dt)
        assert self.nb > 0, self.dims
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)
        self.out, self.gi, self.gw = torch.empty_like(self.go), torch.empty_like(self.x), torch.zeros_like(self.w)
        self.st = _lib.current_stream(DEV)
        td = TORCH_DT[mode]
        self.tx, self.tw, self.tgo = self.x.to(td), self.w.to(td), self.go.to(td)
        self.flop = 2.0 * B * So * So * 9 * Cout * Cin

    def fwd(self):
        _lib.check(self.lib.tdrn_conv2d_strided_forward(_lib.ptr(self.x), _lib.ptr(self.w), None, _lib.ptr(self.out), *self.dims,
                                                        self.dt, _lib.ptr(self.ws), self.nb, self.st))

    def dgrad(self):
        _lib.check(self.lib.tdrn_conv2d_strided_backward_input(_lib.ptr(self.go), _lib.ptr(self.w), _lib.ptr(self.gi), *self.dims,
                                                               self.dt, _lib.ptr(self.ws), self.nb, self.st))

    def wgrad(self):
        _lib.check(self.lib.tdrn_conv2d_strided_backward_parameters(_lib.ptr(self.x), _lib.ptr(self.go), _lib.ptr(self.gw), None,
                                                                    *self.dims, 1.0, self.dt, _lib.ptr(self.ws), self.nb, self.st))

    def _bwd(self, mask):
        p = self.pad
        return torch.ops.aten.convolution_backward(self.tgo, self.tx, self.tw, None, [2, 2], [p, p], [1, 1], False, [0, 0], 1, mask)

    def t_fwd(self):
        return F.conv2d(self.tx, self.tw, None, 2, self.pad)

    def t_dgrad(self):
        return self._bwd([True, False, False])[0]

    def t_wgrad(self):
        return self._bwd([False, True, False])[1]


def run(name, B, mode, reps):
    L = Layer(name, B, mode, seed=7)
    pairs = (("forward", L.fwd, L.t_fwd), ("dgrad", L.dgrad, L.t_dgrad), ("wgrad", L.wgrad, L.t_wgrad))
    ts = {}
    for key, ours, yard in pairs:
        a, b = [], []
        for _ in range(reps):                 # ours and the yardstick alternate
            a.append(timed(ours))
            b.append(timed(yard))
        ts[key + "_us"], ts["torch_" + key + "_us"] = statistics.median(a), statistics.median(b)
        ts[key + "_tflops"] = L.flop / ts[key + "_us"] * 1e-6
        ts["torch_" + key + "_tflops"] = L.flop / ts["torch_" + key + "_us"] * 1e-6
        ts[key + "_over_torch"] = ts[key + "_us"] / ts["torch_" + key + "_us"]
    # agreement with the yardstick (not a test: the tests compare with float64)
    L.gw.zero_()
    L.fwd(); L.dgrad(); L.wgrad()
    diffs = {}
    for key, got, ref in (("forward", L.out, L.t_fwd()), ("dgrad", L.gi, L.t_dgrad()), ("wgrad", L.gw, L.t_wgrad())):
        ref = ref.float()
        diffs[key] = float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    ts["max_rel_diff_vs_torch"] = diffs
    ts["flop_per_product"], ts["workspace_bytes"] = L.flop, L.nb
    return ts


def train_step(B, size, mode, reps):
    """one forward_train + backward of the smooth test loss (mean square of the outputs), synthetic weights"""
    from tdrn_amd.model.dualrefinedet_vggbn import build_net
    from tdrn_amd.utils import synth
    net = build_net("train", 320, 21, 1024, 1, True, False)
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
    ap.add_argument("--modes", default="bf16,fp32")
    ap.add_argument("--layers", default=",".join(LAYERS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--step-size", type=int, default=320)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "mfma_peak_flops": MFMA_PEAK, "results": {}, "train_step": {}}

    def save():
        with open(os.path.join(a.out_dir, "conv_strided.json"), "w") as f:
            json.dump(res, f, indent=1)

    for mode in a.modes.split(","):
        for B in (int(v) for v in a.batches.split(",")):
            for name in a.layers.split(","):
                r = run(name, B, mode, a.reps)
                res["results"]["%s_b%d_%s" % (name, B, mode)] = r
                print("%-9s b%-3d %-4s fwd %8.1f us (torch %8.1f)  dgrad %8.1f (%8.1f)  wgrad %8.1f (%8.1f)  diff %s" % (
                    name, B, mode, r["forward_us"], r["torch_forward_us"], r["dgrad_us"], r["torch_dgrad_us"], r["wgrad_us"],
                    r["torch_wgrad_us"], {k: "%.1e" % v for k, v in r["max_rel_diff_vs_torch"].items()}), flush=True)
                save()
    if not a.no_step:
        for mode in a.modes.split(","):
            r = train_step(a.step_batch, a.step_size, mode, a.reps)
            res["train_step"]["%dpx_b%d_%s" % (a.step_size, a.step_batch, mode)] = r
            print("forward_train + backward, %d px, batch %d, %s: %.1f ms, peak memory %.0f MiB" % (
                a.step_size, a.step_batch, mode, r["step_ms"], r["peak_memory_mib"]), flush=True)
            save()


if __name__ == "__main__":
    main()
