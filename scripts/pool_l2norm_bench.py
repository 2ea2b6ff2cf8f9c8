"""Trainable MaxPool2d and L2Norm (tdrn_hip.h section i-e): timings of the forward and of the backward on the five pools and the two
L2Norm layers of dualrefinedet_vggbn at 320, against torch in the same process.

    python scripts/pool_l2norm_bench.py OUT_DIR [--batches 8,32] [--reps 5] [--layers pool1,...]

Each entry is timed between two device events: the median of `reps` repeats after a discarded warm-up, ours and the yardstick
alternating.  Yardsticks, on the same GPU tensors: F.max_pool2d and its autograd backward; the torch formula of
layers/modules/l2norm.py and its autograd backward (input and weight gradients).  Bytes are algorithmic, what the entry has to move
once: pool forward = input + output + codes (1/4 of the output), pool backward = grad_output + codes + grad_input, L2Norm forward =
2 tensors + norm, L2Norm backward = 3 tensors + norm (the partial sums of grad_weight not counted); the rate is their quotient with
the entry's time, against bench.py's HBM_PEAK_GBS.  A tensor below 256 MiB can be served from the Infinity Cache
(`fits_infinity_cache`).  Writes OUT_DIR/pool_l2norm.json.
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
EPS = 1e-10

# name: kind, C, S, (kernel, stride, pad, ceil_mode)
LAYERS = {"pool1": ("pool", 64, 320, (2, 2, 0, 0)), "pool2": ("pool", 128, 160, (2, 2, 0, 0)), "pool3": ("pool", 256, 80, (2, 2, 0, 1)),
          "pool4": ("pool", 512, 40, (2, 2, 0, 0)), "pool5": ("pool", 512, 20, (3, 1, 1, 0)),
          "l2norm_conv4_3": ("l2norm", 512, 40, None), "l2norm_conv5_3": ("l2norm", 512, 20, None)}


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


class Pool:
    def __init__(self, name, B, seed):
        _, C, S, self.geo = LAYERS[name]
        k, s, p, ceil = self.geo
        gen = torch.Generator(device="cpu").manual_seed(seed)
        self.lib, self.dims = _lib.lib(), (B, C, S, S)
        So = self.lib.tdrn_max_pool_output_size(S, *self.geo)
        assert So > 0
        # behind BN + ReLU: about half the values are zero, so ties are common
        self.x = torch.randn(B, C, S, S, generator=gen).clamp_min_(0).to(DEV)
        self.go = torch.randn(B, C, So, So, generator=gen).to(DEV)
        self.out, self.code = torch.empty_like(self.go), torch.empty(self.go.shape, dtype=torch.uint8, device=DEV)
        self.gi = torch.empty_like(self.x)
        self.st = _lib.current_stream(DEV)
        self.tensor_bytes = 4 * self.x.numel()
        out_bytes = 4 * self.go.numel()
        self.bytes = {"forward": self.tensor_bytes + out_bytes + out_bytes // 4, "backward": out_bytes + out_bytes // 4 + self.tensor_bytes}
        self.tx = self.x.clone().requires_grad_(True)
        self.ty = None

    def fwd(self):
        _lib.check(self.lib.tdrn_max_pool_forward(_lib.ptr(self.x), _lib.ptr(self.out), _lib.ptr(self.code), *self.dims, *self.geo, self.st))

    def bwd(self):
        _lib.check(self.lib.tdrn_max_pool_backward(_lib.ptr(self.go), _lib.ptr(self.code), _lib.ptr(self.gi), *self.dims, *self.geo, self.st))

    def t_fwd(self):
        k, s, p, ceil = self.geo
        self.ty = F.max_pool2d(self.tx, k, s, p, ceil_mode=bool(ceil))

    def t_bwd(self):
        return torch.autograd.grad(self.ty, (self.tx,), self.go, retain_graph=True)

    def diffs(self):
        self.fwd()
        self.bwd()
        self.t_fwd()
        tg, = self.t_bwd()
        # bitwise in the forward; the backward of 3x3 sums up to nine terms in another order than torch
        return {"output_bitwise_equal": bool(torch.equal(self.out.view(torch.int32), self.ty.detach().view(torch.int32))),
                "grad_input": float((self.gi - tg).abs().max()) / max(1.0, float(tg.abs().max()))}


class L2:
    def __init__(self, name, B, seed):
        _, C, S, _ = LAYERS[name]
        gen = torch.Generator(device="cpu").manual_seed(seed)
        self.lib, self.dims = _lib.lib(), (B, C, S, S)
        self.x = torch.randn(B, C, S, S, generator=gen).to(DEV)
        self.go = torch.randn(B, C, S, S, generator=gen).to(DEV)
        self.w = (8 + 4 * torch.rand(C, generator=gen)).to(DEV)
        self.nb = self.lib.tdrn_l2norm_workspace_bytes(*self.dims)
        assert self.nb > 0, self.dims
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)
        self.out, self.gi = torch.empty_like(self.x), torch.empty_like(self.x)
        self.norm, self.gw = torch.empty(B, S, S, device=DEV), torch.zeros(C, device=DEV)
        self.st = _lib.current_stream(DEV)
        self.tensor_bytes = 4 * self.x.numel()
        self.bytes = {"forward": 2 * self.tensor_bytes + 4 * self.norm.numel(), "backward": 3 * self.tensor_bytes + 4 * self.norm.numel()}
        self.tx, self.tw = self.x.clone().requires_grad_(True), self.w.clone().requires_grad_(True)
        self.ty = None

    def fwd(self):
        _lib.check(self.lib.tdrn_l2norm_forward(_lib.ptr(self.x), _lib.ptr(self.w), _lib.ptr(self.out), _lib.ptr(self.norm), *self.dims, EPS,
                                                self.st))

    def bwd(self):
        _lib.check(self.lib.tdrn_l2norm_backward(_lib.ptr(self.x), _lib.ptr(self.go), _lib.ptr(self.w), _lib.ptr(self.norm), _lib.ptr(self.gi),
                                                 _lib.ptr(self.gw), *self.dims, EPS, 1.0, _lib.ptr(self.ws), self.nb, self.st))

    def t_fwd(self):
        norm = self.tx.pow(2).sum(dim=1, keepdim=True).sqrt() + EPS
        self.ty = self.tw.view(1, -1, 1, 1) * (self.tx / norm)

    def t_bwd(self):
        return torch.autograd.grad(self.ty, (self.tx, self.tw), self.go, retain_graph=True)

    def diffs(self):
        self.gw.zero_()
        self.fwd()
        self.bwd()
        self.t_fwd()
        tg = self.t_bwd()
        return {key: float((got - ref.detach()).abs().max()) / max(1.0, float(ref.detach().abs().max()))
                for key, got, ref in (("output", self.out, self.ty), ("grad_input", self.gi, tg[0]), ("grad_weight", self.gw, tg[1]))}


def run(name, B, reps):
    L = (Pool if LAYERS[name][0] == "pool" else L2)(name, B, seed=7)
    L.fwd()
    L.t_fwd()
    ts = {}
    for key, ours, yard in (("forward", L.fwd, L.t_fwd), ("backward", L.bwd, L.t_bwd)):
        a, b = [], []
        for _ in range(reps):                 # ours and the yardstick alternate
            a.append(timed(ours))
            b.append(timed(yard))
        us, tus = statistics.median(a), statistics.median(b)
        nbytes = L.bytes[key]
        ts[key + "_us"], ts["torch_" + key + "_us"] = us, tus
        ts[key + "_bytes"] = nbytes
        ts[key + "_tbs"], ts["torch_" + key + "_tbs"] = nbytes / us * 1e-6, nbytes / tus * 1e-6
        ts[key + "_fraction_of_hbm_peak"] = nbytes / us * 1e-3 / HBM_PEAK_GBS
        ts[key + "_over_torch"] = us / tus
    # agreement with the yardstick (not a test: the tests compare with the CPU)
    ts["diff_vs_torch"] = L.diffs()
    ts["tensor_bytes"], ts["fits_infinity_cache"] = L.tensor_bytes, L.tensor_bytes < (256 << 20)
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
            print("%-15s b%-3d fwd %8.1f us (torch %8.1f) %5.2f TB/s  bwd %8.1f us (torch %8.1f) %5.2f TB/s  diff %s" % (
                name, B, r["forward_us"], r["torch_forward_us"], r["forward_tbs"], r["backward_us"], r["torch_backward_us"],
                r["backward_tbs"], r["diff_vs_torch"]), flush=True)
            with open(os.path.join(a.out_dir, "pool_l2norm.json"), "w") as f:
                json.dump(res, f, indent=1)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
