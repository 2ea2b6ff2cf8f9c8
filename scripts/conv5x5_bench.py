"""The dense 5x5 conv with gradients (tdrn_hip.h section i-i): timings of forward, backward_input (dgrad) and backward_parameters
(wgrad, five kernel-row passes) on odm_loc_2 / odm_conf_2 of refinedet_vgg (256 -> 12 and 256 -> 63 channels on the 40x40 and 10x10
maps of a 320 px frame), against the vendor library through torch in the same process; one TRN training step (static ssd4scale_vgg
on the engine, temporal forward_train, RefineMultiBoxLoss, backward) with the loc / conf heads of a level paired in one
conv_offset2d call and as two calls; and one refinedet_vgg multihead training step.  Reported, not gated.

    python scripts/conv5x5_bench.py OUT_DIR [--batches 8,32] [--modes bf16,fp32] [--reps 5] [--layers loc40,conf40,loc10,conf10]
                                            [--step-batch 8] [--step-size 320] [--no-step]

Each entry is timed between two device events: the median of `reps` repeats after a discarded warm-up, ours and the yardstick
alternating.  Our entries take and return fp32 NCHW tensors, so their times include the layout conversions, the weight packing
and wgrad's reduce; the yardstick (F.conv2d, torch.ops.aten.convolution_backward with one output masked in) runs on the same values
held in the compute type (bf16 tensors for bf16, fp32 for fp32).  Rates: 2 N H W 25 Cout Cin flop per product.
The training steps run every layer on fp32 NCHW tensors with the layout conversions of every op inside it: the time of the
composition as it stands, not of a tuned training path.  Writes OUT_DIR/conv5x5.json.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tdrn_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}

# name: Cin, Cout, S
LAYERS = {"loc40": (256, 12, 40), "conf40": (256, 63, 40), "loc10": (256, 12, 10), "conf10": (256, 63, 10)}


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
        self.w = (torch.randn(Cout, Cin, 5, 5, generator=gen) * (25 * Cin) ** -0.5).to(DEV)
        self.go = torch.randn(B, Cout, S, S, generator=gen).to(DEV)
        self.dims = (B, Cin, S, S, Cout, 5, 5, 1, 1, 2, 2, 1, 1)
        self.lib, self.dt = _lib.lib(), _lib.DTYPES[mode]
        self.nb = self.lib.tdrn_conv5x5_workspace_bytes(*self.dims, self.dt)
        assert self.nb > 0, self.dims
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)
        self.out, self.gi, self.gw = torch.empty_like(self.go), torch.empty_like(self.x), torch.zeros_like(self.w)
        self.st = _lib.current_stream(DEV)
        td = TORCH_DT[mode]
        self.tx, self.tw, self.tgo = self.x.to(td), self.w.to(td), self.go.to(td)
        self.flop = 2.0 * B * S * S * 25 * Cout * Cin

    def fwd(self):
        _lib.check(self.lib.tdrn_conv5x5_forward(_lib.ptr(self.x), _lib.ptr(self.w), None, _lib.ptr(self.out), *self.dims, self.dt,
                                                 _lib.ptr(self.ws), self.nb, self.st))

    def dgrad(self):
        _lib.check(self.lib.tdrn_conv5x5_backward_input(_lib.ptr(self.go), _lib.ptr(self.w), _lib.ptr(self.gi), *self.dims, self.dt,
                                                        _lib.ptr(self.ws), self.nb, self.st))

    def wgrad(self):
        _lib.check(self.lib.tdrn_conv5x5_backward_parameters(_lib.ptr(self.x), _lib.ptr(self.go), _lib.ptr(self.gw), None, *self.dims,
                                                             1.0, self.dt, _lib.ptr(self.ws), self.nb, self.st))

    def _bwd(self, mask):
        return torch.ops.aten.convolution_backward(self.tgo, self.tx, self.tw, None, [1, 1], [2, 2], [1, 1], False, [0, 0], 1, mask)

    def t_fwd(self):
        return F.conv2d(self.tx, self.tw, None, 1, 2)

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


def _load(net, seed):
    from tdrn_amd.utils import synth
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(DEV)


def _priors_and_targets(B, size):
    from tdrn_amd.data import mb_cfg
    from tdrn_amd.layers import PriorBox
    maps = [size // 8, size // 16, size // 32, size // 64]
    priors = PriorBox(dict(mb_cfg["VOC_320"], min_dim=size, feature_maps=maps, name="VOC_%d" % size)).forward().to(DEV)
    rs = np.random.RandomState(3)
    targets = []
    for _ in range(B):
        n = int(rs.randint(1, 6))
        c, wh = rs.uniform(0.25, 0.75, (n, 2)), rs.uniform(0.1, 0.4, (n, 2))
        rows = np.concatenate([c - wh / 2, c + wh / 2, rs.randint(0, 20, (n, 1)).astype(np.float64)], 1)
        targets.append(torch.from_numpy(rows.astype(np.float32)).to(DEV))
    return priors, targets


def _measure(step, reps):
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ts = [timed(step, warm=0) for _ in range(reps)]
    return statistics.median(ts) * 1e-3, torch.cuda.max_memory_allocated() / 2 ** 20


def trn_step(B, size, mode, reps):
    """train_trn.py's default path with --deform: the static net on the engine, the temporal net through forward_train, the refine
    loss on the static net's ARM output, backward; paired and separate heads alternating"""
    from tdrn_amd.layers import RefineMultiBoxLoss
    from tdrn_amd.model.ssd4scale_vgg import build_net
    from tdrn_amd.utils import synth
    static = _load(build_net("train", 320, 21, 1024, True, False), 1).eval()
    net = _load(build_net("train", 320, 21, 1024, True, True), 0)
    x = torch.from_numpy(synth.synth_frames(B, size, seed=5)).to(DEV)
    priors, targets = _priors_and_targets(B, size)
    criterion = RefineMultiBoxLoss(21, 0.5, True, 0, True, 3, 0.5, False, device=DEV)

    def step():
        net.zero_grad(set_to_none=True)
        with torch.no_grad():
            static_out = list(static(x, ret_loc=True))
        out = net.forward_train(x, static_out[2], mode)
        loss_l, loss_c = criterion(out, priors, targets, arm_data=static_out[:2])
        (loss_l + loss_c).backward()

    res = {"batch": B, "size": size, "compute": mode}
    times = {True: [], False: []}
    for paired in (True, False):
        net._paired_heads = paired
        _, res["peak_memory_mib_%s" % ("paired" if paired else "separate")] = _measure(step, 1)
    for _ in range(reps):                     # the two forms alternate
        for paired in (True, False):
            net._paired_heads = paired
            times[paired].append(timed(step, warm=0))
    res["step_ms_paired"], res["step_ms_separate"] = statistics.median(times[True]) * 1e-3, statistics.median(times[False]) * 1e-3
    return res


def refinedet_step(B, size, mode, reps):
    """train.py's RefineDet loop with --refine True --multihead True: forward_train, the two refine losses, backward"""
    from tdrn_amd.layers import RefineMultiBoxLoss
    from tdrn_amd.model.refinedet_vgg import build_net
    from tdrn_amd.utils import synth
    net = _load(build_net("train", 320, 21, True, 1024, True, True), 0)
    x = torch.from_numpy(synth.synth_frames(B, size, seed=5)).to(DEV)
    priors, targets = _priors_and_targets(B, size)
    arm_criterion = RefineMultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, device=DEV, only_loc=True)
    criterion = RefineMultiBoxLoss(21, 0.5, True, 0, True, 3, 0.5, False, device=DEV)

    def step():
        net.zero_grad(set_to_none=True)
        out = net.forward_train(x, mode)
        loss_l, loss_c = criterion(out[2:], priors, targets, arm_data=out[:2])
        (arm_criterion(out[0], priors, targets) + loss_l + loss_c).backward()

    ms, mib = _measure(step, reps)
    return {"batch": B, "size": size, "compute": mode, "step_ms": ms, "peak_memory_mib": mib}


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
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "results": {}, "trn_step": {}, "refinedet_step": {}}

    def save():
        with open(os.path.join(a.out_dir, "conv5x5.json"), "w") as f:
            json.dump(res, f, indent=1)

    for mode in a.modes.split(","):
        for B in (int(v) for v in a.batches.split(",")):
            for name in a.layers.split(","):
                r = run(name, B, mode, a.reps)
                res["results"]["%s_b%d_%s" % (name, B, mode)] = r
                print("%-7s b%-3d %-4s fwd %8.1f us (torch %8.1f)  dgrad %8.1f (%8.1f)  wgrad %8.1f (%8.1f)  diff %s" % (
                    name, B, mode, r["forward_us"], r["torch_forward_us"], r["dgrad_us"], r["torch_dgrad_us"], r["wgrad_us"],
                    r["torch_wgrad_us"], {k: "%.1e" % v for k, v in r["max_rel_diff_vs_torch"].items()}), flush=True)
                save()
    if not a.no_step:
        for mode in a.modes.split(","):
            key = "%dpx_b%d_%s" % (a.step_size, a.step_batch, mode)
            r = trn_step(a.step_batch, a.step_size, mode, a.reps)
            res["trn_step"][key] = r
            print("TRN step (ssd4scale_vgg), %s: paired heads %.1f ms, separate %.1f ms; peak memory %.0f / %.0f MiB" % (
                key, r["step_ms_paired"], r["step_ms_separate"], r["peak_memory_mib_paired"], r["peak_memory_mib_separate"]), flush=True)
            save()
            r = refinedet_step(a.step_batch, a.step_size, mode, a.reps)
            res["refinedet_step"][key] = r
            print("refinedet_vgg multihead step, %s: %.1f ms, peak memory %.0f MiB" % (key, r["step_ms"], r["peak_memory_mib"]), flush=True)
            save()


if __name__ == "__main__":
    main()
