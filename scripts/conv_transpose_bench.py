"""ConvTranspose2d(kernel 2, stride 2) with gradients (tdrn_hip.h section i-f): timings of forward, backward_input (dgrad) and
backward_parameters (wgrad) on the three TCB up-sampling layers of dualrefinedet_vggbn at 320 (256 -> 256 channels at 5x5, 10x10
and 20x20), against the vendor library through torch in the same process.

    python scripts/conv_transpose_bench.py OUT_DIR [--batches 8,32] [--modes bf16,fp32] [--reps 5] [--layers up5,up10,up20]

Each entry is timed between two device events: the median of `reps` repeats after a discarded warm-up, ours and the yardstick
alternating.  Our entries take and return fp32 NCHW tensors, so their times include the layout conversions, the weight packing
and wgrad's reduce; the yardstick (F.conv_transpose2d, torch.ops.aten.convolution_backward with one output masked in) runs on the
same values held in the compute type (bf16 tensors for bf16, fp32 for fp32).  Rates: 2 N H W 4 Cout Cin flop per product, against
the dense MFMA peak figures DESIGN 6 uses.  Writes OUT_DIR/conv_transpose.json.
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

# name: Cin, Cout, S (the input map; the output is 2S x 2S)
LAYERS = {"up5": (256, 256, 5), "up10": (256, 256, 10), "up20": (256, 256, 20)}


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
        Cin, Cout, S = LAYERS[name]
        gen = torch.Generator(device="cpu").manual_seed(seed)
        self.mode = mode
        self.x = torch.randn(B, Cin, S, S, generator=gen).to(DEV)
        self.w = (torch.randn(Cin, Cout, 2, 2, generator=gen) * Cin ** -0.5).to(DEV)
        self.go = torch.randn(B, Cout, 2 * S, 2 * S, generator=gen).to(DEV)
        self.dims = (B, Cin, S, S, Cout, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1)
        self.lib, self.dt = _lib.lib(), _lib.DTYPES[mode]
        self.nb = self.lib.tdrn_conv_transpose2d_workspace_bytes(*self.dims, self.dt)
        assert self.nb > 0, self.dims
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)
        self.out, self.gi, self.gw = torch.empty_like(self.go), torch.empty_like(self.x), torch.zeros_like(self.w)
        self.st = _lib.current_stream(DEV)
        td = TORCH_DT[mode]
        self.tx, self.tw, self.tgo = self.x.to(td), self.w.to(td), self.go.to(td)
        self.flop = 2.0 * B * S * S * 4 * Cout * Cin

    def fwd(self):
        _lib.check(self.lib.tdrn_conv_transpose2d_forward(_lib.ptr(self.x), _lib.ptr(self.w), None, _lib.ptr(self.out), *self.dims,
                                                          self.dt, _lib.ptr(self.ws), self.nb, self.st))

    def dgrad(self):
        _lib.check(self.lib.tdrn_conv_transpose2d_backward_input(_lib.ptr(self.go), _lib.ptr(self.w), _lib.ptr(self.gi), *self.dims,
                                                                 self.dt, _lib.ptr(self.ws), self.nb, self.st))

    def wgrad(self):
        _lib.check(self.lib.tdrn_conv_transpose2d_backward_parameters(_lib.ptr(self.x), _lib.ptr(self.go), _lib.ptr(self.gw), None,
                                                                      *self.dims, 1.0, self.dt, _lib.ptr(self.ws), self.nb, self.st))

    def _bwd(self, mask):
        return torch.ops.aten.convolution_backward(self.tgo, self.tx, self.tw, None, [2, 2], [0, 0], [1, 1], True, [0, 0], 1, mask)

    def t_fwd(self):
        return F.conv_transpose2d(self.tx, self.tw, None, 2)

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--modes", default="bf16,fp32")
    ap.add_argument("--layers", default=",".join(LAYERS))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "mfma_peak_flops": MFMA_PEAK, "results": {}}
    for mode in a.modes.split(","):
        for B in (int(v) for v in a.batches.split(",")):
            for name in a.layers.split(","):
                r = run(name, B, mode, a.reps)
                res["results"]["%s_b%d_%s" % (name, B, mode)] = r
                print("%-5s b%-3d %-4s fwd %8.1f us (torch %8.1f)  dgrad %8.1f (%8.1f)  wgrad %8.1f (%8.1f)  diff %s" % (
                    name, B, mode, r["forward_us"], r["torch_forward_us"], r["dgrad_us"], r["torch_dgrad_us"], r["wgrad_us"],
                    r["torch_wgrad_us"], {k: "%.1e" % v for k, v in r["max_rel_diff_vs_torch"].items()}), flush=True)
                with open(os.path.join(a.out_dir, "conv_transpose.json"), "w") as f:
                    json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
