"""Gradient oracle for deformable conv v1 (test helper; product code never imports it).

A restatement, in torch fp64 on the CPU, of the reference's forward rule -- deformable_im2col_bilinear
(utils/deformconv/deform_conv_cuda_kernel.cu:15-51), the rejection test and coordinates of
deformable_im2col_gpu_kernel (:189-203) and the column GEMM of deform_conv_forward_cuda
(deform_conv_cuda.c:157-193) -- differentiated by torch.autograd.

The sample coordinates are formed in fp32 exactly as the device forms them (h_im = (float)(h_in + i*dil) + off for the
rejection test, map_h = (float)(i*dil) + off for the floor and the [H-1, H) clamp), so every floor / border decision
agrees with the product's; everything after that (the fractions, the blend, the GEMM) is fp64 and differentiable.
Away from those measure-zero decision points its gradients equal the reference's backward kernels
(get_gradient_weight / get_coordinate_weight, deform_conv_cuda_kernel.cu:53-154; deformable_col2im :247-298;
deformable_col2im_coord :337-400): a rejected coordinate contributes nothing, the clamp band puts all of the weight on
row H-1 and has a zero offset derivative, an exact integer has the one-sided (v_high - v_low) derivative.
"""
import torch


def _pr(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def deform_conv(x, off, w, stride=1, padding=0, dilation=1, G=1, with_coords=False, tap_cols=None):
    """x (N,Cin,H,W), off (N,G*2*kh*kw,Ho,Wo), w (Cout,Cin,kh,kw): fp64 CPU tensors (may require grad).
    Returns out (N,Cout,Ho,Wo) fp64; with_coords=True also the fp32 sample coordinates (h_im, w_im) of every
    (n, g, tap, ho, wo) -- what the tests use to find the measure-zero points.
    tap_cols: None is the op (tap t sits at divmod(t, kw)); another divisor restates a kernel that splits its taps wrongly, for the
    tests that show such a kernel could not pass (tests/test_deform_ts_ref.py)."""
    (sh, sw), (ph, pw), (dh, dw) = _pr(stride), _pr(padding), _pr(dilation)
    N, Cin, H, W = x.shape
    Cout, _, kh, kw = w.shape
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    taps, cpg = kh * kw, Cin // G
    h_in = (torch.arange(Ho) * sh - ph).view(1, Ho, 1)
    w_in = (torch.arange(Wo) * sw - pw).view(1, 1, Wo)
    xf = x.reshape(N, Cin, H * W)
    cols = []
    coords = []
    for g in range(G):
        xg = xf[:, g * cpg:(g + 1) * cpg]
        gcols = []
        for t in range(taps):
            ti, tj = divmod(t, kw if tap_cols is None else tap_cols)
            oh = off[:, g * 2 * taps + 2 * t]
            ow = off[:, g * 2 * taps + 2 * t + 1]
            oh32, ow32 = oh.detach().float(), ow.detach().float()
            # fp32 coordinates, as deform_conv_cuda_kernel.cu:189-198 forms them
            h_im = (h_in + ti * dh).float() + oh32
            w_im = (w_in + tj * dw).float() + ow32
            valid = (h_im >= 0) & (w_im >= 0) & (h_im < H) & (w_im < W)
            hm = torch.tensor(float(ti * dh), dtype=torch.float32) + oh32            # map_h, relative to h_in
            wm = torch.tensor(float(tj * dw), dtype=torch.float32) + ow32
            height, width = H - h_in, W - w_in
            h_low, w_low = torch.floor(hm).long(), torch.floor(wm).long()
            ch, cw = h_low >= height - 1, w_low >= width - 1                        # the [H-1, H) clamp (:24-36)
            h_low = torch.where(ch, (height - 1).expand_as(h_low), h_low)
            w_low = torch.where(cw, (width - 1).expand_as(w_low), w_low)
            h_high = torch.where(ch, h_low, h_low + 1)
            w_high = torch.where(cw, w_low, w_low + 1)
            lh = torch.where(ch, torch.zeros_like(oh), (ti * dh + oh) - h_low.double())
            lw = torch.where(cw, torch.zeros_like(ow), (tj * dw + ow) - w_low.double())
            hh, hw = 1 - lh, 1 - lw
            r0 = (h_in + h_low).clamp(0, H - 1)
            r1 = (h_in + h_high).clamp(0, H - 1)
            q0 = (w_in + w_low).clamp(0, W - 1)
            q1 = (w_in + w_high).clamp(0, W - 1)

            def corner(r, q):
                idx = (r * W + q).reshape(N, 1, Ho * Wo).expand(N, cpg, Ho * Wo)
                return torch.gather(xg, 2, idx).reshape(N, cpg, Ho, Wo)

            val = ((hh * hw).unsqueeze(1) * corner(r0, q0) + (hh * lw).unsqueeze(1) * corner(r0, q1)
                   + (lh * hw).unsqueeze(1) * corner(r1, q0) + (lh * lw).unsqueeze(1) * corner(r1, q1))
            gcols.append(val * valid.unsqueeze(1).double())
            coords.append((h_im, w_im))
        cols.append(torch.stack(gcols, 2))                  # (N, cpg, taps, Ho, Wo)
    col = torch.cat(cols, 1)                                # (N, Cin, taps, Ho, Wo)
    out = torch.einsum("nctp,oct->nop", col.reshape(N, Cin, taps, Ho * Wo), w.reshape(Cout, Cin, taps))
    out = out.reshape(N, Cout, Ho, Wo)
    if with_coords:
        hs = torch.stack([c[0] for c in coords], 1).reshape(N, G, taps, Ho, Wo)
        ws = torch.stack([c[1] for c in coords], 1).reshape(N, G, taps, Ho, Wo)
        return out, hs, ws
    return out


def grads(x, off, w, grad_out, stride=1, padding=0, dilation=1, G=1, tap_cols=None):
    """(out, grad_input, grad_offset, grad_weight), all fp64 CPU tensors, for numpy / torch inputs."""
    t = lambda a: torch.as_tensor(a).detach().double().clone().requires_grad_(True)
    x, off, w = t(x), t(off), t(w)
    out = deform_conv(x, off, w, stride, padding, dilation, G, tap_cols=tap_cols)
    gx, go, gw = torch.autograd.grad(out, (x, off, w), torch.as_tensor(grad_out).double())
    return out.detach(), gx, go, gw


def near_decision(off, x_shape, w_shape, stride=1, padding=0, dilation=1, G=1, eps=1e-5):
    """Boolean (N, G*2*taps, Ho, Wo) mask of offset entries whose fp32 sample coordinate (either axis of the sample)
    lies within eps of an integer or of the map border: the measure-zero points where the derivative jumps."""
    N, Cin, H, W = x_shape
    kh, kw = w_shape[2], w_shape[3]
    _, hs, ws = deform_conv(torch.zeros(x_shape, dtype=torch.float64), torch.as_tensor(off).double(),
                            torch.zeros(w_shape, dtype=torch.float64), stride, padding, dilation, G, with_coords=True)
    hs, ws = hs.double(), ws.double()
    near = lambda c: (c - torch.round(c)).abs() < eps
    bad = near(hs) | near(ws)                               # integers include the borders 0 and H / W
    bad = bad.unsqueeze(3).expand(-1, -1, -1, 2, -1, -1)    # both axes of the sample
    return bad.reshape(N, G * 2 * kh * kw, hs.shape[-2], hs.shape[-1])


# ------------------------------------------------------------------------------------------------------------------
# Shapes of the backward fuzz (tests/test_gpu_train_fuzz.py); tests/test_deform_grad_ref.py asserts on the CPU that they
# reach the branches of deform_bwd.hip they are meant to reach.
# ------------------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = tuple(range(24))
FUZZ_CPG = (1, 2, 3, 8, 63, 64, 65, 100, 130)        # channels per group: below a wave, a chunk, chunks with a ragged last one
FUZZ_COUT = (1, 4, 31, 32, 33, 75, 128, 129, 140)    # around the weight kernel's switch (32) and its 128-wide blocks
FUZZ_OFFSET_SCALE = (0.0, 0.5, 2.0, 6.0)


def _schedule(values, n, seed):
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    while len(out) < n:
        out += [values[i] for i in rng.permutation(len(values))]
    return out[:n]


def fuzz_shape(seed):
    """dict(N, Cin, H, W, Cout, k=(kh, kw), stride, pad, dil, G, osc, Ho, Wo, M): test_deform_conv_fuzz_matches_oracle's
    distribution with the channels per group and Cout run through FUZZ_CPG / FUZZ_COUT.  Wide inputs get small kernels and
    maps, so the fp64 oracle stays in seconds."""
    import numpy as np
    n = len(FUZZ_SEEDS)
    rng = np.random.Generator(np.random.PCG64(5000 + seed))
    cpg, Cout = _schedule(FUZZ_CPG, n, 11)[seed], _schedule(FUZZ_COUT, n, 12)[seed]
    G = int(rng.choice([1, 2, 4, 8]))
    while G * cpg > 520:
        G = int(rng.choice([1, 2, 4, 8]))
    Cin = G * cpg
    kmax, span = (3, 8) if Cin >= 200 else (5, 13)
    kh, kw = int(rng.integers(1, kmax + 1)), int(rng.integers(1, kmax + 1))
    sh, sw = int(rng.integers(1, 3)), int(rng.integers(1, 3))
    dh, dw = int(rng.integers(1, 3)), int(rng.integers(1, 3))
    ph, pw = int(rng.integers(0, 3)), int(rng.integers(0, 3))
    N = int(rng.integers(1, 4))
    H = int(rng.integers(dh * (kh - 1) + 1, dh * (kh - 1) + 1 + span))
    W = int(rng.integers(dw * (kw - 1) + 1, dw * (kw - 1) + 1 + span))
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    return dict(N=N, Cin=Cin, H=H, W=W, Cout=Cout, k=(kh, kw), stride=(sh, sw), pad=(ph, pw), dil=(dh, dw), G=G, cpg=cpg,
                osc=float(_schedule(FUZZ_OFFSET_SCALE, n, 13)[seed]), Ho=Ho, Wo=Wo, M=N * Ho * Wo)
