"""Cases, inputs and float64 references of test_gpu_train_large.py (the training ops on tensors of more than 2^30 elements: past
2^31 bytes in the 16-bit compute type's staging, past 2^32 bytes in fp32).  No GPU is needed here; test_train_large_ref.py asserts
what the construction relies on.

Construction.  A big tensor is R replicas, along N, of a small base (N = 1) whose reference is computed on the CPU.  Per-element
results (outputs, input gradients, batch statistics) are the base's, replicated; sums over the batch (parameter gradients) are R
times the base's.  The period -- the elements of one replica in any layout a kernel walks, the conv's channel-padded NHWC staging
included -- divides none of 2^29, 2^30, 2^31: an offset that wrapped at 2^31 or 2^32 bytes (fp32: 2^29, 2^30 elements; 16-bit:
2^30, 2^31 elements) or at 2^31 elements lands on another position of a replica, whose value differs.

The five conv families (tdrn_hip.h sections i-c conv2d, i-f ConvTranspose2d 2x2 / stride 2, i-g 3x3 conv at stride 2, i-h depthwise
3x3, i-i 5x5 conv) share one description: FAMILIES names each one's entry prefix, cases and modes, and op_dims, op_shapes,
op_forward, op_inputs and op_reference serve all of them.  The stagings of the four later ones: the space-to-depth image
[N][H][W][4][CoPad] of grad_output (i-f), the zero-inserted image [N][Hd][Wd][CoPad] of grad_output with Hd = H + 2 pad - 2 (i-g), the
channel-padded NHWC images of x and grad_output (i-f, i-g, i-i); the depthwise kernels walk the NCHW planes themselves.
"""
import functools

import torch
import torch.nn.functional as F

R = 80
EPS, MOMENTUM = 1e-5, 0.1                      # batch_norm
L2_EPS = 1e-10
torch.set_num_threads(min(16, torch.get_num_threads()))      # (float64 references: the GPU hosts' threads oversubscribe)

# C, H, W, relu
BN_CASES = {"bn_500_relu": (64, 500, 500, 1), "bn_501": (64, 501, 501, 0)}
FLOOR, CEIL, K3 = (2, 2, 0, 0), (2, 2, 0, 1), (3, 1, 1, 0)       # kernel, stride, pad, ceil_mode
# C, H, W, geometry
POOL_CASES = {"pool_500_floor": (64, 500, 500, FLOOR), "pool_501_floor": (64, 501, 501, FLOOR), "pool_501_ceil": (64, 501, 501, CEIL),
              "pool_500_k3": (64, 500, 500, K3), "pool_501_k3": (64, 501, 501, K3)}
L2_CASES = {"l2_500": (64, 500, 500)}
# Cin, H, W, Cout, k, pad, dil
CONV_CASES = {"conv_big_output": (3, 500, 500, 64, 3, 1, 1),          # big output, big padded NHWC input
              "conv_big_grad_input": (64, 500, 500, 3, 3, 1, 1)}      # big input, big input gradient
CONV_MODES = {"fp32": None, "bf16": torch.bfloat16}
# ConvTranspose2d 2x2 at stride 2 (i-f): Cin, H, W, Cout
CONVT_CASES = {"convt_big_output": (3, 250, 250, 64),          # big output and space-to-depth staging; W even: the s2d kernel's 16-byte path
               "convt_big_grad_input": (256, 251, 251, 3)}     # big input, input gradient and both stagings; W odd: the dword path
# 3x3 conv at stride 2 (i-g): Cin, H, W, Cout, pad
S2_CASES = {"s2_big_grad_input": (64, 506, 506, 3, 0),         # big input and input gradient, D = 64 x 504 x 504; Wo = 252: the dilate kernel's quad
                                                               # path; input row and column 505 are touched by no output pixel
            "s2_big_dilated": (3, 501, 501, 64, 1)}            # big D = 64 x 501 x 501 (Hd = 2 Ho - 1) and x staging; Wo = 251: the dword path
# depthwise 3x3, pad 1 (i-h): C, H, W, stride
DW_CASES = {"dw_500_s1": (64, 500, 500, 1), "dw_501_s2": (64, 501, 501, 2)}       # (501 at stride 2: an odd map, Ho = 251)
# 5x5 conv, pad 2 (i-i): Cin, H, W, Cout
K5_CASES = {"k5_big_output": (3, 500, 500, 64), "k5_big_grad_input": (64, 500, 500, 3)}
DW_MODES = {"fp32": None}                                      # the depthwise op has no 16-bit mode
# family -> (entry prefix, cases, modes)
FAMILIES = {"conv": ("tdrn_conv2d", CONV_CASES, CONV_MODES), "convt": ("tdrn_conv_transpose2d", CONVT_CASES, CONV_MODES),
            "s2": ("tdrn_conv2d_strided", S2_CASES, CONV_MODES), "dw": ("tdrn_dwconv2d", DW_CASES, DW_MODES),
            "k5": ("tdrn_conv5x5", K5_CASES, CONV_MODES)}
NEW_FAMILIES = ("convt", "s2", "dw", "k5")


def cpad(c):
    return -(-c // 64) * 64


def family(case):
    return next(f for f, (_, cases, _) in FAMILIES.items() if case in cases)


def periods(case):
    """elements of one replica in every big layout of the case"""
    if case in CONVT_CASES:                                      # x, output / grad_output, the NHWC image of x, the space-to-depth image
        Cin, H, W, Cout = CONVT_CASES[case]
        return sorted({Cin * H * W, Cout * 4 * H * W, cpad(Cin) * H * W, 4 * cpad(Cout) * H * W})
    if case in S2_CASES:                                         # x, output, their NHWC images, the zero-inserted image D
        Cin, H, W, Cout, pad = S2_CASES[case]
        Ho, Wo, Hd, Wd = (H + 2 * pad - 3) // 2 + 1, (W + 2 * pad - 3) // 2 + 1, H + 2 * pad - 2, W + 2 * pad - 2
        return sorted({Cin * H * W, Cout * Ho * Wo, cpad(Cin) * H * W, cpad(Cout) * Ho * Wo, cpad(Cout) * Hd * Wd})
    if case in DW_CASES:                                         # the NCHW planes of x and of the output: no staging
        C, H, W, s = DW_CASES[case]
        return sorted({C * H * W, C * ((H - 1) // s + 1) * ((W - 1) // s + 1)})
    if case in K5_CASES:                                         # x, output, their NHWC images (Ho x Wo = H x W)
        Cin, H, W, Cout = K5_CASES[case]
        return sorted({Cin * H * W, Cout * H * W, cpad(Cin) * H * W, cpad(Cout) * H * W})
    if case in CONV_CASES:
        Cin, H, W, Cout, k, pad, dil = CONV_CASES[case]
        Ho, Wo = H + 2 * pad - dil * (k - 1), W + 2 * pad - dil * (k - 1)
        return sorted({Cin * H * W, Cout * Ho * Wo, cpad(Cin) * H * W, cpad(Cout) * Ho * Wo})
    C, H, W = (BN_CASES.get(case) or POOL_CASES.get(case) or L2_CASES.get(case))[:3]
    return [C * H * W]


def big_elements(case):
    """the element count of the largest tensor, staging included"""
    return R * max(periods(case))


def _gen(case):
    # (the later families follow the first four's names, whose seeds stay what they were)
    names = sorted(list(BN_CASES) + list(POOL_CASES) + list(L2_CASES) + list(CONV_CASES)) + \
        [c for f in NEW_FAMILIES for c in FAMILIES[f][1]]
    return torch.Generator().manual_seed(names.index(case) + 101)


# ---------------------------------------------------------------------------------------------
# batch_norm
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bn_inputs(case):
    """base x (1, C, H, W), gamma, beta, base grad_output, starting running_mean and running_var (CPU, fp32)"""
    C, H, W, _ = BN_CASES[case]
    gen = _gen(case)
    x = 0.5 + torch.randn(1, C, H, W, generator=gen)
    w = 0.5 + torch.rand(C, generator=gen)
    b = 0.2 * torch.randn(C, generator=gen)
    go = torch.randn(1, C, H, W, generator=gen)
    rm = 0.5 * torch.randn(C, generator=gen)
    rv = 0.5 + torch.rand(C, generator=gen)
    return x, w, b, go, rm, rv


@functools.lru_cache(maxsize=None)
def bn_reference(case):
    """float64, for R replicas of the base: computed once, never changed.  The ReLU kink is handled by test_gpu_batch_norm.py's rule:
    grad_output is exactly 0 where the float64 pre-activation lies within tau = 1e-4 * max(1, max|y|) of zero; `kink_share` is the
    share of those elements."""
    C, H, W, relu = BN_CASES[case]
    x, w, b, go, rm, rv = bn_inputs(case)
    x64, w64, b64 = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    z = F.batch_norm(x64, None, None, w64, b64, True, MOMENTUM, EPS)
    y = F.relu(z) if relu else z
    go_used, share = go.clone(), 0.0
    if relu:
        tau = 1e-4 * max(1.0, float(y.detach().abs().max()))
        near = z.detach().abs() <= tau
        share = float(near.double().mean())
        go_used[near] = 0.0
    gx, gw, gb = torch.autograd.grad(y, (x64, w64, b64), go_used.double())
    xd = x.double()
    mean, var = xd.mean((0, 2, 3)), xd.var((0, 2, 3), unbiased=False)
    n = R * H * W                                                # the unbiased factor of running_var uses the full count
    # grad_input of the replicated batch: the batch means inside it are the base's means, and autograd on the base alone divides
    # by the base's count: the same values
    return {"output": y.detach(), "grad_input": gx, "grad_weight": R * gw, "grad_bias": R * gb, "go": go_used, "kink_share": share,
            "save_mean": mean, "save_invstd": (var + EPS).rsqrt(),
            "running_mean": (1 - MOMENTUM) * rm.double() + MOMENTUM * mean,
            "running_var": (1 - MOMENTUM) * rv.double() + MOMENTUM * var * n / (n - 1)}


# ---------------------------------------------------------------------------------------------
# max_pool2d
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_inputs(case):
    """base x and base grad_output (CPU, fp32)"""
    C, H, W, geo = POOL_CASES[case]
    gen = _gen(case)
    x = torch.randn(1, C, H, W, generator=gen)
    k, s, p, ceil = geo
    Ho, Wo = F.max_pool2d(x[:, :1], k, s, p, ceil_mode=bool(ceil)).shape[2:]
    return x, torch.randn(1, C, Ho, Wo, generator=gen)


@functools.lru_cache(maxsize=None)
def pool_reference(case):
    """torch on the CPU: output and grad_input in fp32 (compared bit for bit), the window codes from torch's indices, and the
    float64 grad_input for 3/1/1, where up to nine windows add into one element (test_gpu_max_pool.py)"""
    C, H, W, (k, s, p, ceil) = POOL_CASES[case]
    x, go = pool_inputs(case)

    def oracle(dtype):
        xr = x.to(dtype).clone().requires_grad_(True)
        y, idx = F.max_pool2d(xr, k, s, p, ceil_mode=bool(ceil), return_indices=True)
        gi, = torch.autograd.grad(y, xr, go.to(dtype))
        return y.detach(), idx, gi
    y, idx, gi = oracle(torch.float32)
    Ho, Wo = y.shape[2:]
    ho, wo = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    dy, dx = idx // W - (ho * s - p), idx % W - (wo * s - p)
    assert int(dy.min()) >= 0 and int(dy.max()) < k and int(dx.min()) >= 0 and int(dx.max()) < k
    ref = {"output": y, "code": (dy * k + dx).to(torch.uint8), "grad_input": gi}
    if k == 3:
        ref["grad_input64"] = oracle(torch.float64)[2]
    return ref


# ---------------------------------------------------------------------------------------------
# l2norm
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def l2_inputs(case):
    C, H, W = L2_CASES[case]
    gen = _gen(case)
    x = torch.randn(1, C, H, W, generator=gen)
    w = 8 + 4 * torch.rand(C, generator=gen)
    go = torch.randn(1, C, H, W, generator=gen)
    return x, w, go


@functools.lru_cache(maxsize=None)
def l2_reference(case):
    x, w, go = l2_inputs(case)
    x64, w64 = x.double().clone().requires_grad_(True), w.double().clone().requires_grad_(True)
    norm = x64.pow(2).sum(dim=1, keepdim=True).sqrt() + L2_EPS
    y = w64.view(1, -1, 1, 1) * (x64 / norm)
    gx, gw = torch.autograd.grad(y, (x64, w64), go.double())
    return {"output": y.detach(), "norm": norm.detach()[:, 0], "grad_input": gx, "grad_weight": R * gw}


# ---------------------------------------------------------------------------------------------
# conv2d
# ---------------------------------------------------------------------------------------------
def conv_out_hw(case):
    Cin, H, W, Cout, k, pad, dil = CONV_CASES[case]
    return H + 2 * pad - dil * (k - 1), W + 2 * pad - dil * (k - 1)


def conv_round(t, mode):
    return t if CONV_MODES[mode] is None else t.to(CONV_MODES[mode]).float()


# ---------------------------------------------------------------------------------------------
# the five conv families: conv2d, conv_transpose2d, conv2d at stride 2, depthwise conv2d, conv5x5
# ---------------------------------------------------------------------------------------------
def op_dims(case, N=R):
    """the argument tuple of the family's four entries, in the header's order"""
    f = family(case)
    if f == "convt":
        Cin, H, W, Cout = CONVT_CASES[case]
        return (N, Cin, H, W, Cout, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1)
    if f == "s2":
        Cin, H, W, Cout, pad = S2_CASES[case]
        return (N, Cin, H, W, Cout, 3, 3, 2, 2, pad, pad, 1, 1)
    if f == "dw":
        C, H, W, s = DW_CASES[case]
        return (N, C, H, W, 3, 3, s, s, 1, 1, 1, 1)
    if f == "k5":
        Cin, H, W, Cout = K5_CASES[case]
        return (N, Cin, H, W, Cout, 5, 5, 1, 1, 2, 2, 1, 1)
    Cin, H, W, Cout, k, pad, dil = CONV_CASES[case]
    return (N, Cin, H, W, Cout, k, k, 1, 1, pad, pad, dil, dil)


def op_shapes(case):
    """base shapes (N = 1) -> (x, weight, output, fan-in of the forward sum)"""
    f = family(case)
    if f == "convt":
        Cin, H, W, Cout = CONVT_CASES[case]
        return (1, Cin, H, W), (Cin, Cout, 2, 2), (1, Cout, 2 * H, 2 * W), Cin              # one tap per output pixel
    if f == "s2":
        Cin, H, W, Cout, pad = S2_CASES[case]
        return (1, Cin, H, W), (Cout, Cin, 3, 3), (1, Cout, (H + 2 * pad - 3) // 2 + 1, (W + 2 * pad - 3) // 2 + 1), 9 * Cin
    if f == "dw":
        C, H, W, s = DW_CASES[case]
        return (1, C, H, W), (C, 1, 3, 3), (1, C, (H - 1) // s + 1, (W - 1) // s + 1), 1    # (plain randn: test_gpu_dwconv.py)
    if f == "k5":
        Cin, H, W, Cout = K5_CASES[case]
        return (1, Cin, H, W), (Cout, Cin, 5, 5), (1, Cout, H, W), 25 * Cin
    Cin, H, W, Cout, k, pad, dil = CONV_CASES[case]
    return (1, Cin, H, W), (Cout, Cin, k, k), (1, Cout) + conv_out_hw(case), Cin * k * k


def op_forward(case):
    """torch's op of the family: (x, w, b) -> y"""
    f = family(case)
    if f == "convt":
        return lambda x, w, b: F.conv_transpose2d(x, w, b, 2)
    if f == "s2":
        return lambda x, w, b: F.conv2d(x, w, b, 2, S2_CASES[case][4])
    if f == "dw":
        return lambda x, w, b: F.conv2d(x, w, b, DW_CASES[case][3], 1, 1, DW_CASES[case][0])
    if f == "k5":
        return lambda x, w, b: F.conv2d(x, w, b, 1, 2)
    Cin, H, W, Cout, k, pad, dil = CONV_CASES[case]
    return lambda x, w, b: F.conv2d(x, w, b, 1, pad, dil)


def untouched(case):
    """the input rows and columns that no output pixel touches: grad_input is exactly 0 there"""
    if case not in S2_CASES:
        return [], []
    Cin, H, W, Cout, pad = S2_CASES[case]
    last_h, last_w = 2 * ((H + 2 * pad - 3) // 2) + 2 - pad, 2 * ((W + 2 * pad - 3) // 2) + 2 - pad
    return list(range(last_h + 1, H)), list(range(last_w + 1, W))


@functools.lru_cache(maxsize=None)
def op_inputs(case):
    """base x, weight, bias and grad_output (CPU, fp32): unit-scale normals, the dense families' weights scaled by fan-in^-0.5"""
    xs, ws, ys, fan_in = op_shapes(case)
    gen = _gen(case)
    x = torch.randn(xs, generator=gen)
    w = torch.randn(ws, generator=gen) * fan_in ** -0.5
    b = torch.randn(ys[1], generator=gen)
    go = torch.randn(ys, generator=gen)
    return x, w, b, go


@functools.lru_cache(maxsize=None)
def op_reference(case, mode):
    """test_gpu_conv_grad.py's oracle on the base, for any family: float64 autograd on the inputs as the op uses them (rounded to
    the 16-bit type first, bias not), and the same op on absolute values for the 16-bit bound -> ((y, gx, gw, gb), (Sy, Sgx, Sgw,
    Sgb)), the parameter gradients times R"""
    x, w, b, go = op_inputs(case)
    xr, wr, gr = (conv_round(t, mode).double() for t in (x, w, go))
    op = op_forward(case)

    def run(xx, ww, bb, gg):
        xx, ww, bb = (t.clone().requires_grad_(True) for t in (xx, ww, bb))
        y = op(xx, ww, bb)
        gx, gw, gb = torch.autograd.grad(y, (xx, ww, bb), gg)
        return y.detach(), gx, R * gw, R * gb
    return run(xr, wr, b.double(), gr), run(xr.abs(), wr.abs(), b.double().abs(), gr.abs())
