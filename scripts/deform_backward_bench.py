"""Deformable conv v1 backward: timings of the fp32 forward, backward_input and backward_parameters (tdrn_hip.h sections i
and i-b) on the two head sets, a torch yardstick in the same process, gradient agreement, and rates derived from shapes.

    python scripts/deform_backward_bench.py OUT_DIR [--sets odm,trn] [--batches 8,32] [--reps 7]

Shape sets: the ODM heads of dualrefinedet_vggbn at 320 (levels 40/20/10/5; loc 12 and conf 63; 3x3 and 5x5; Cin 256,
G = 1) and the deformable heads of ssd4scale_mobile's temporal net (Cin 512/1024/512/512 at 20/10/5/3, G = 8, Cout 12 and
63).  Each (set, batch) is timed as a whole: every member's op runs back to back between two device events, the median of
`reps` repeats after a warm-up.  The yardstick is the reference's forward rule written as torch ops (fp32 on the GPU),
differentiated by torch autograd, timed alternately with ours.  Writes OUT_DIR/deform_backward.json.
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
MFMA_F32_PEAK = 157.3e12
ATOMIC_RATE = 1.3e12

# (Cin, H, Cout, k, G) members; padding k // 2, stride 1, dilation 1
SETS = {
    "odm": [(256, s, c, k, 1) for s in (40, 20, 10, 5) for c in (12, 63) for k in (3, 5)],
    "trn": [(cin, s, c, 3, 8) for cin, s in ((512, 20), (1024, 10), (512, 5), (512, 3)) for c in (12, 63)],
}


def torch_deform(x, off, w, pad, G):
    """the reference's forward rule (deform_conv_cuda_kernel.cu:15-51, 189-203) as torch ops, fp32, autograd-able"""
    N, Cin, H, W = x.shape
    Cout, _, kh, kw = w.shape
    Ho, Wo = H + 2 * pad - kh + 1, W + 2 * pad - kw + 1
    taps, cpg = kh * kw, Cin // G
    h_in = (torch.arange(Ho, device=x.device) - pad).view(1, Ho, 1)
    w_in = (torch.arange(Wo, device=x.device) - pad).view(1, 1, Wo)
    xf = x.reshape(N, Cin, H * W)
    cols = []
    for g in range(G):
        xg = xf[:, g * cpg:(g + 1) * cpg]
        for t in range(taps):
            ti, tj = divmod(t, kw)
            oh, ow = off[:, g * 2 * taps + 2 * t], off[:, g * 2 * taps + 2 * t + 1]
            h_im, w_im = (h_in + ti).float() + oh, (w_in + tj).float() + ow
            valid = ((h_im >= 0) & (w_im >= 0) & (h_im < H) & (w_im < W)).float()
            hm, wm = ti + oh, tj + ow
            height, width = H - h_in, W - w_in
            hl, wl = torch.floor(hm.detach()).long(), torch.floor(wm.detach()).long()
            ch, cw = hl >= height - 1, wl >= width - 1
            hl = torch.where(ch, (height - 1).expand_as(hl), hl)
            wl = torch.where(cw, (width - 1).expand_as(wl), wl)
            hh_ = torch.where(ch, hl, hl + 1)
            wh_ = torch.where(cw, wl, wl + 1)
            lh = torch.where(ch, torch.zeros_like(hm), hm - hl.float())
            lw = torch.where(cw, torch.zeros_like(wm), wm - wl.float())
            r0, r1 = (h_in + hl).clamp(0, H - 1), (h_in + hh_).clamp(0, H - 1)
            q0, q1 = (w_in + wl).clamp(0, W - 1), (w_in + wh_).clamp(0, W - 1)

            def corner(r, q):
                return torch.gather(xg, 2, (r * W + q).reshape(N, 1, -1).expand(N, cpg, Ho * Wo)).reshape(N, cpg, Ho, Wo)

            val = (((1 - lh) * (1 - lw)).unsqueeze(1) * corner(r0, q0) + ((1 - lh) * lw).unsqueeze(1) * corner(r0, q1)
                   + (lh * (1 - lw)).unsqueeze(1) * corner(r1, q0) + (lh * lw).unsqueeze(1) * corner(r1, q1))
            cols.append(val * valid.unsqueeze(1))
    col = torch.stack(cols, 1).reshape(N, G, taps, cpg, Ho * Wo).permute(0, 1, 3, 2, 4).reshape(N, Cin * taps, Ho * Wo)
    return torch.matmul(w.reshape(Cout, Cin * taps), col).reshape(N, Cout, Ho, Wo)


class Member:
    def __init__(self, B, Cin, S, Cout, k, G, seed):
        gen = torch.Generator(device="cpu").manual_seed(seed)
        self.pad, self.G = k // 2, G
        self.x = torch.randn(B, Cin, S, S, generator=gen).to(DEV)
        self.w = (torch.randn(Cout, Cin, k, k, generator=gen) * (Cin * k * k) ** -0.5).to(DEV)
        self.off = (torch.randn(B, G * 2 * k * k, S, S, generator=gen) * 2.0).to(DEV)
        self.gout = torch.randn(B, Cout, S, S, generator=gen).to(DEV)
        self.dims = (B, Cin, S, S, Cout, k, k, 1, 1, self.pad, self.pad, 1, 1, G)
        lib = _lib.lib()
        self.nf = lib.tdrn_deform_conv_workspace_bytes(B, Cin, S, S, Cout, k, k, 1, 1, self.pad, self.pad, 1, 1, G, 0)
        self.nb = lib.tdrn_deform_conv_backward_workspace_bytes(B, Cin, S, S, Cout, k, k, 1, 1, self.pad, self.pad, 1, 1, G)
        self.wsf = torch.empty(self.nf, dtype=torch.uint8, device=DEV)
        self.wsb = torch.empty(self.nb, dtype=torch.uint8, device=DEV)
        self.out = torch.empty_like(self.gout)
        self.gi, self.goff, self.gw = torch.zeros_like(self.x), torch.empty_like(self.off), torch.zeros_like(self.w)
        M, taps = B * S * S, k * k
        self.flop_gemm = 2.0 * M * Cout * Cin * taps                     # one of the three GEMM-shaped products
        self.atomic_bytes = M * taps * G * _cpg64(Cin // G) * 4 * 4      # 4 corner adds per column element (incl. pad lanes)

    def fwd(self, lib, st):
        _lib.check(lib.tdrn_deform_conv_forward(_lib.ptr(self.x), _lib.ptr(self.w), _lib.ptr(self.off), _lib.ptr(self.out), *self.dims,
                                                0, _lib.ptr(self.wsf), self.nf, st))

    def bwd_in(self, lib, st):
        _lib.check(lib.tdrn_deform_conv_backward_input(_lib.ptr(self.x), _lib.ptr(self.off), _lib.ptr(self.gout), _lib.ptr(self.gi),
                                                       _lib.ptr(self.goff), _lib.ptr(self.w), *self.dims, _lib.ptr(self.wsb), self.nb, st))

    def bwd_par(self, lib, st):
        _lib.check(lib.tdrn_deform_conv_backward_parameters(_lib.ptr(self.x), _lib.ptr(self.off), _lib.ptr(self.gout), _lib.ptr(self.gw),
                                                            *self.dims, 1.0, _lib.ptr(self.wsb), self.nb, st))

    def yard(self):
        x, off, w = (t.detach().clone().requires_grad_(True) for t in (self.x, self.off, self.w))
        y = torch_deform(x, off, w, self.pad, self.G)
        return torch.autograd.grad(y, (x, off, w), self.gout)


def _cpg64(cpg):
    return (cpg + 63) // 64 * 64


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def run_set(name, B, reps, check, yard=True):
    lib = _lib.lib()
    st = _lib.current_stream(DEV)
    ms = [Member(B, *m, seed=i) for i, m in enumerate(SETS[name])]
    every = lambda f: (lambda: [f(m, lib, st) for m in ms])
    t = {"forward_us": [], "backward_input_us": [], "backward_parameters_us": [], "torch_yardstick_fwd_bwd_us": []}
    for _ in range(reps):          # ours and the yardstick alternate
        t["forward_us"].append(timed(every(Member.fwd), 1))
        t["backward_input_us"].append(timed(every(Member.bwd_in), 1))
        t["backward_parameters_us"].append(timed(every(Member.bwd_par), 1))
        if yard:
            t["torch_yardstick_fwd_bwd_us"].append(timed(lambda: [m.yard() for m in ms], 1, warm=1))
    if not yard:
        del t["torch_yardstick_fwd_bwd_us"]
    r = {k: statistics.median(v) for k, v in t.items()}
    r["backward_total_us"] = r["backward_input_us"] + r["backward_parameters_us"]
    r["backward_over_forward"] = r["backward_total_us"] / r["forward_us"]
    flop = sum(m.flop_gemm for m in ms)
    atom = sum(m.atomic_bytes for m in ms)
    r["flop_per_gemm"] = flop
    r["forward_tflops"] = flop / r["forward_us"] * 1e-6
    r["backward_input_tflops"] = flop / r["backward_input_us"] * 1e-6
    r["backward_parameters_tflops"] = flop / r["backward_parameters_us"] * 1e-6
    r["fp32_mfma_peak_tflops"] = MFMA_F32_PEAK * 1e-12
    r["atomic_bytes"] = atom
    r["backward_input_atomic_tbps"] = atom / r["backward_input_us"] * 1e-6
    r["atomic_rate_tbps"] = ATOMIC_RATE * 1e-12
    if yard:
        r["yardstick_over_ours"] = r["torch_yardstick_fwd_bwd_us"] / (r["forward_us"] + r["backward_total_us"])
    if check:
        diffs = {"grad_input": 0.0, "grad_offset": 0.0, "grad_weight": 0.0}
        for m in ms:
            m.gi.zero_(); m.gw.zero_()
            m.bwd_in(lib, st); m.bwd_par(lib, st)
            ref = m.yard()
            for key, got, rf in zip(diffs, (m.gi, m.goff, m.gw), ref):
                diffs[key] = max(diffs[key], float((got - rf).abs().max()) / max(1.0, float(rf.abs().max())))
        torch.cuda.synchronize()
        r["max_rel_diff_vs_yardstick"] = diffs
    r["members"] = len(ms)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--sets", default="odm,trn")
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--ours-only", action="store_true", help="no yardstick at all (profiler runs): implies --no-check")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "results": {}}
    for s in a.sets.split(","):
        for b in (int(v) for v in a.batches.split(",")):
            r = run_set(s, b, a.reps, not (a.no_check or a.ours_only), not a.ours_only)
            res["results"]["%s_b%d" % (s, b)] = r
            print("%s b%-3d fwd %8.1f us  bwd_in %8.1f  bwd_par %8.1f  (bwd/fwd %.2f)  torch %9.1f us  diff %s" % (
                s, b, r["forward_us"], r["backward_input_us"], r["backward_parameters_us"], r["backward_over_forward"],
                r.get("torch_yardstick_fwd_bwd_us", float("nan")), r.get("max_rel_diff_vs_yardstick")), flush=True)
    with open(os.path.join(a.out_dir, "deform_backward.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
