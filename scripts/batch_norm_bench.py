"""BatchNorm2d with a fused ReLU (tdrn_hip.h section i-d): timings of the training forward and of the backward on five BN layers of
dualrefinedet_vggbn at 320, against torch in the same process.

    python scripts/batch_norm_bench.py OUT_DIR [--batches 8,32] [--reps 5] [--layers conv1_2,...]

Each entry is timed between two device events: the median of `reps` repeats after a discarded warm-up, ours and the yardstick
alternating.  The yardstick is F.relu(F.batch_norm(..., training=True)) and its autograd backward (input, weight and bias
gradients) on the same tensors.  Bytes are algorithmic: 3 passes over an fp32 tensor of the layer's size forward (read, read,
write), 5 backward (two reads twice, one write); the rate is their quotient with the entry's time, against bench.py's HBM_PEAK_GBS.
A tensor below 256 MiB can be served from the Infinity Cache on its second pass (`fits_infinity_cache`).
Writes OUT_DIR/batch_norm.json.
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
HBM_PEAK_GBS = 8000.0           # bench.py's figure
EPS, MOMENTUM = 1e-5, 0.1

# name: C, S
LAYERS = {"conv1_2": (64, 320), "conv2_2": (128, 160), "conv3_3": (256, 80), "conv4_3": (512, 40), "conv7": (1024, 10)}


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
        C, S = LAYERS[name]
        gen = torch.Generator(device="cpu").manual_seed(seed)
        self.dims = (B, C, S, S)
        self.x = torch.randn(B, C, S, S, generator=gen).to(DEV)
        self.go = torch.randn(B, C, S, S, generator=gen).to(DEV)
        self.w = (0.5 + torch.rand(C, generator=gen)).to(DEV)
        self.b = (0.2 * torch.randn(C, generator=gen)).to(DEV)
        self.rm, self.rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        self.lib = _lib.lib()
        self.nb = self.lib.tdrn_batch_norm_workspace_bytes(*self.dims)
        assert self.nb > 0, self.dims
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)
        self.out, self.gi = torch.empty_like(self.x), torch.empty_like(self.x)
        self.mean, self.invstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        self.gw, self.gb = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        self.st = _lib.current_stream(DEV)
        self.tensor_bytes = 4 * self.x.numel()
        self.tx, self.tw, self.tb = (t.clone().requires_grad_(True) for t in (self.x, self.w, self.b))
        self.ty = None

    def fwd(self):
        _lib.check(self.lib.tdrn_batch_norm_forward(_lib.ptr(self.x), _lib.ptr(self.w), _lib.ptr(self.b), _lib.ptr(self.rm), _lib.ptr(self.rv),
                                                    _lib.ptr(self.out), _lib.ptr(self.mean), _lib.ptr(self.invstd), *self.dims, 1, MOMENTUM,
                                                    EPS, 1, _lib.ptr(self.ws), self.nb, self.st))

    def bwd(self):
        _lib.check(self.lib.tdrn_batch_norm_backward(_lib.ptr(self.x), _lib.ptr(self.go), _lib.ptr(self.w), _lib.ptr(self.b),
                                                     _lib.ptr(self.mean), _lib.ptr(self.invstd), _lib.ptr(self.gi), _lib.ptr(self.gw),
                                                     _lib.ptr(self.gb), *self.dims, 1, 1, 1.0, _lib.ptr(self.ws), self.nb, self.st))

    def t_fwd(self):
        self.ty = F.relu(F.batch_norm(self.tx, self.rm, self.rv, self.tw, self.tb, True, MOMENTUM, EPS))

    def t_bwd(self):
        return torch.autograd.grad(self.ty, (self.tx, self.tw, self.tb), self.go, retain_graph=True)


def run(name, B, reps):
    L = Layer(name, B, seed=7)
    L.fwd()
    L.t_fwd()
    ts = {}
    for key, ours, yard, passes in (("forward", L.fwd, L.t_fwd, 3), ("backward", L.bwd, L.t_bwd, 5)):
        a, b = [], []
        for _ in range(reps):                 # ours and the yardstick alternate
            a.append(timed(ours))
            b.append(timed(yard))
        us, tus = statistics.median(a), statistics.median(b)
        nbytes = passes * L.tensor_bytes
        ts[key + "_us"], ts["torch_" + key + "_us"] = us, tus
        ts[key + "_bytes"] = nbytes
        ts[key + "_tbs"], ts["torch_" + key + "_tbs"] = nbytes / us * 1e-6, nbytes / tus * 1e-6
        ts[key + "_fraction_of_hbm_peak"] = nbytes / us * 1e-3 / HBM_PEAK_GBS
        ts[key + "_over_torch"] = us / tus
    # agreement with the yardstick (not a test: the tests compare with float64)
    L.gw.zero_()
    L.gb.zero_()
    L.fwd()
    L.bwd()
    L.t_fwd()
    tg = L.t_bwd()
    diffs = {}
    for key, got, ref in (("output", L.out, L.ty), ("grad_input", L.gi, tg[0]), ("grad_weight", L.gw, tg[1]), ("grad_bias", L.gb, tg[2])):
        ref = ref.detach()
        diffs[key] = float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    ts["max_rel_diff_vs_torch"] = diffs
    ts["tensor_bytes"], ts["fits_infinity_cache"], ts["workspace_bytes"] = L.tensor_bytes, L.tensor_bytes < (256 << 20), L.nb
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--layers", default=",".join(LAYERS))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "hbm_peak_gbs": HBM_PEAK_GBS, "results": {}}
    for B in (int(v) for v in a.batches.split(",")):
        for name in a.layers.split(","):
            r = run(name, B, a.reps)
            res["results"]["%s_b%d" % (name, B)] = r
            print("%-8s b%-3d fwd %8.1f us (torch %8.1f) %5.2f TB/s  bwd %8.1f us (torch %8.1f) %5.2f TB/s  diff %s" % (
                name, B, r["forward_us"], r["torch_forward_us"], r["forward_tbs"], r["backward_us"], r["torch_backward_us"],
                r["backward_tbs"], {k: "%.1e" % v for k, v in r["max_rel_diff_vs_torch"].items()}), flush=True)
            with open(os.path.join(a.out_dir, "batch_norm.json"), "w") as f:
                json.dump(res, f, indent=1)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
