"""The training ops (tdrn_hip.h sections i-c to i-i) on tensors of more than 2^30 elements: past 2^32 bytes in fp32, past 2^31
bytes in the convs' 16-bit staging.  The ABI admits up to 2^31 elements; conv1_2's activation at batch 32 and 512 pixels has 2^29.

Construction, cases and float64 references: tests/_train_large_cases.py (80 replicas along N of a base with N = 1, whose period
divides no power of two; tests/test_train_large_ref.py asserts that without a GPU).  Every element of every replica is compared, on
the GPU, replica by replica in float64.  No element is exempted.

Bounds: the per-op files', unchanged.
  batch_norm (test_gpu_batch_norm.py)  output, gradients: 1e-4 * max(1, max|ref|); save_mean, running_mean: 1e-5 * max(1, |ref|);
                                       save_invstd, running_var: 1e-5 relative
  max_pool2d (test_gpu_max_pool.py)    output, codes, the 2/2 grad_input: bit for bit torch's CPU result; the 3/1/1 grad_input: 1e-4 *
                                       max(1, max|ref|) of float64, and every replica bit for bit the first one
  l2norm (test_gpu_l2norm.py)          output, gradients: 1e-4 * max(1, max|ref|); norm: 1e-5 relative
  conv2d (test_gpu_conv_grad.py)       fp32: 1e-4 * max(1, max|ref|); bf16: 2e-6 * S elementwise, S the conv of absolute values
  conv_transpose2d (i-f), conv2d at stride 2 (i-g), conv5x5 (i-i)       conv2d's two bounds (_conv_train_harness.py)
  dwconv2d (i-h, test_gpu_dwconv.py)   1e-4 * max(1, max|ref|); output and grad_input also bit for bit the first replica in every replica
                                       (the header fixes their tap order)
The later families' cases (tests/_train_large_cases.py): convt_big_output (W even: the space-to-depth kernel's 16-byte path; the
output and the [N][H][W][4][CoPad] staging are big) and convt_big_grad_input (W odd: the dword path; x, grad_input and both stagings);
s2_big_grad_input (Wo = 252: the dilate kernel's quad path; x, grad_input and the zero-inserted image D are big, and row and column
505 of grad_input, which no output pixel touches, must be exactly +0.0 in all 80 replicas) and s2_big_dilated (Wo = 251: the dword
path with Hd = 2 Ho - 1; only D and the x staging are big); dw_500_s1 and dw_501_s2; k5_big_output and k5_big_grad_input.  One
routine, _conv_family, runs the three entries of any of the five conv families from its entry prefix and dims tuple.
The sums over the whole batch (parameter gradients, batch statistics) add 2 * 10^7 terms per value, a count at which nobody has
measured fp32 accumulation.  For those the bound is max(the bound above, 4 x the error of torch's own fp32 GPU reductions of the
same quantity against the same float64 reference), test_short_training_run_with_pool_and_l2norm_follows_float64's rule, taken
elementwise.  Both errors are printed.  torch's side is built from reductions over the whole tensor (var_mean, sum) and, for the
conv's weight gradient, one fp32 matrix product per tap.  Measured on an MI355X: no sum of the library's uses more than 0.0225 of
the project bound alone (the conv's fp32 grad_weight), no replicated result more than 0.0135 (l2norm's norm).  torch's reductions
stay below 0.011 of the project bound, its matrix products of 2 * 10^7 terms do not: 0.39 to 1.32 of it, so for the conv's
grad_weight the rule allows up to 5.3 times the project bound on some elements.  The library does not need that room.
The later families, measured on an MI355X, largest share of the project bound (replicated results: fp32 / bf16; sums: ours, torch's):
  conv_transpose2d  replicated 0.0065 / 0.070   summed 0.1154 (fp32 grad_weight of convt_big_grad_input), torch 0.33 to 1.15
  conv2d stride 2   replicated 0.0081 / 0.099   summed 0.0124 (fp32 grad_weight of s2_big_grad_input), torch 0.37 to 1.07
  dwconv2d          replicated 0.0014           summed 0.0063 (grad_bias of dw_500_s1), torch 0.0012 (sums, no matrix product)
  conv5x5           replicated 0.0158 / 0.080   summed 0.0804 (fp32 grad_weight of k5_big_output), torch 0.49 to 1.73
so the rule allows up to 6.9 times the project bound on some elements of the 5x5 grad_weight, and again the library needs none of it:
every sum of these families passes the project bound alone.

Memory: each test works out an upper bound of what it needs and skips only if torch.cuda.mem_get_info() shows less (measured
peaks: conv fp32 24.4 GiB, bf16 19.6 GiB; batch_norm 19.6 GiB; max_pool 3/1/1 20.8 GiB; l2norm 19.7 GiB; conv_transpose2d fp32
24.6 GiB, bf16 19.8 GiB; conv2d stride 2 fp32 24.6 GiB, bf16 19.7 GiB; dwconv2d 19.6 GiB; conv5x5 fp32 24.4 GiB, bf16 19.6 GiB);
everything is released at the end of each test.

Durations (pytest --durations=0, call phase, one MI355X run of the whole file; the float64 reference on the CPU is part of each):
conv2d 0.7 to 1.9 s; conv_transpose2d 0.4 to 0.5 s; conv2d stride 2 0.3 to 0.8 s; dwconv2d 0.6 and 0.9 s; conv5x5 1.2 to 1.4 s
(k5_big_output) and 4.5 to 4.6 s (k5_big_grad_input, whose two float64 passes of a 64 -> 3 channel 5x5 conv over 500 x 500 pixels
take about 4 s on the CPU; its GPU side takes as long as the other cases').
"""
import gc

import pytest
import torch

import _train_large_cases as L
from tdrn_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = L.R
NAN = float("nan")
C_ACC = {"bf16": 2e-6}                          # test_gpu_conv_grad.py
GIB = float(2 ** 30)


def _reserve(tag, nbytes):
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    print("%s: needs %.1f GiB, %.1f GiB free" % (tag, nbytes / GIB, free / GIB))
    if free < nbytes:
        pytest.skip("%s needs %.1f GiB of device memory, %.1f GiB are free" % (tag, nbytes / GIB, free / GIB))
    torch.cuda.reset_peak_memory_stats()


def _release(tag):
    print("%s: peak device memory %.1f GiB" % (tag, torch.cuda.max_memory_allocated() / GIB))
    gc.collect()
    torch.cuda.empty_cache()


def _rep(base):
    """R replicas of base (1, ...) along N, on the device"""
    return base.to(DEV).expand(R, *base.shape[1:]).contiguous()


def _nan(shape):
    return torch.full(shape, NAN, device=DEV)


def _worst(big, ref, scale=None):
    """max over every element of every replica of |big[r] - ref| (/ scale), in float64 on the device; NaN if anything is not finite"""
    ref = ref.to(DEV).double()[0]
    scale = None if scale is None else scale.to(DEV).double()[0]
    m = torch.zeros((), dtype=torch.float64, device=DEV)
    for r in range(R):
        d = (big[r].double() - ref).abs()
        m = torch.maximum(m, (d if scale is None else d / scale).max())
    return float(m)


def _replicated_fp32(tag, name, big, ref):
    """the project's fp32 bound on a replicated result"""
    assert big.shape[0] == R and big.shape[1:] == ref.shape[1:]
    d, bound = _worst(big, ref), 1e-4 * max(1.0, float(ref.abs().max()))
    print("%s %-12s max|d| %.3e  share of the bound %.4f" % (tag, name, d, d / bound))
    assert d <= bound, (tag, name, d, bound)                # (NaN fails)


def _same_bits(big, ref):
    """every replica bit for bit ref[0] (any 1-, 4-byte type)"""
    ref = ref.to(DEV)[0].contiguous()
    bits = torch.int32 if ref.element_size() == 4 else torch.uint8
    ref = ref.view(bits)
    ok = torch.ones((), dtype=torch.bool, device=DEV)
    for r in range(R):
        ok = ok & (big[r].view(bits) == ref).all()
    return bool(ok)


def _summed(tag, name, got, ref, kind, torch_got):
    """a sum over the whole batch: max(project bound, 4 x torch's own fp32 error), elementwise.  kind: fp32 | abs5 | rel5 | (c, S)"""
    g, t, r = got.detach().cpu().double(), torch_got.detach().cpu().double(), ref
    d, dt = (g - r).abs(), (t - r).abs()
    assert torch.isfinite(d).all(), "%s %s: non-finite values" % (tag, name)
    if kind == "fp32":
        project = torch.full_like(r, 1e-4 * max(1.0, float(r.abs().max())))
    elif kind == "abs5":
        project = 1e-5 * r.abs().clamp_min(1.0)
    elif kind == "rel5":
        project = 1e-5 * r.abs()
    else:
        project = kind[0] * kind[1]
    bound = torch.maximum(project, 4 * dt)
    print("%s %-12s max|d| %.3e  share of the project bound: ours %.4f, torch's fp32 GPU reduction %.4f; share of the bound used %.4f"
          % (tag, name, float(d.max()), float((d / project).max()), float((dt / project).max()), float((d / bound).max())))
    assert bool((d <= bound).all()), (tag, name, float(d.max()), float((d / bound).max()))


# ---------------------------------------------------------------------------------------------
# batch_norm
# ---------------------------------------------------------------------------------------------
def _batch_norm(case):
    C, H, W, relu = L.BN_CASES[case]
    ref = L.bn_reference(case)
    lib, dims, st = _lib.lib(), (R, C, H, W), _lib.current_stream(DEV)
    nb = lib.tdrn_batch_norm_workspace_bytes(*dims)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    xb, w, b, _, rm0, rv0 = L.bn_inputs(case)
    x, go = _rep(xb), _rep(ref["go"])
    w, b, rm, rv = (t.to(DEV).clone() for t in (w, b, rm0, rv0))
    out, gi = _nan(x.shape), _nan(x.shape)
    sm, si, gw, gb = _nan((C,)), _nan((C,)), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    _lib.check(lib.tdrn_batch_norm_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(rm), _lib.ptr(rv), _lib.ptr(out), _lib.ptr(sm),
                                           _lib.ptr(si), *dims, 1, L.MOMENTUM, L.EPS, relu, _lib.ptr(ws), nb, st))
    _lib.check(lib.tdrn_batch_norm_backward(_lib.ptr(x), _lib.ptr(go), _lib.ptr(w), _lib.ptr(b), _lib.ptr(sm), _lib.ptr(si), _lib.ptr(gi),
                                            _lib.ptr(gw), _lib.ptr(gb), *dims, 1, relu, 1.0, _lib.ptr(ws), nb, st))
    torch.cuda.synchronize()
    _replicated_fp32(case, "output", out, ref["output"])
    _replicated_fp32(case, "grad_input", gi, ref["grad_input"])
    del gi
    # torch's own fp32 reductions of the same sums
    n = R * H * W
    var_t, mean_t = torch.var_mean(x, (0, 2, 3), unbiased=False)
    si_t = (var_t + L.EPS).rsqrt()
    rm_t = (1 - L.MOMENTUM) * rm0.to(DEV) + L.MOMENTUM * mean_t
    rv_t = (1 - L.MOMENTUM) * rv0.to(DEV) + L.MOMENTUM * var_t * (n / (n - 1.0))
    if relu:
        go.mul_(out > 0)                        # (out is the library's: the mask of the fused ReLU)
    del out
    gb_t = go.sum((0, 2, 3))
    x.sub_(mean_t.view(1, C, 1, 1)).mul_(si_t.view(1, C, 1, 1)).mul_(go)
    gw_t = x.sum((0, 2, 3))
    for name, got, kind, t in (("save_mean", sm, "abs5", mean_t), ("save_invstd", si, "rel5", si_t), ("running_mean", rm, "abs5", rm_t),
                               ("running_var", rv, "rel5", rv_t), ("grad_weight", gw, "fp32", gw_t), ("grad_bias", gb, "fp32", gb_t)):
        _summed(case, name, got, ref[name], kind, t)


@pytest.mark.parametrize("case", list(L.BN_CASES))
def test_batch_norm_training_past_4gib(case):
    C, H, W, _ = L.BN_CASES[case]
    _reserve(case, (4 + 1) * 4 * R * C * H * W + 2 ** 30)       # x, grad_output, output, grad_input; one temporary
    try:
        _batch_norm(case)
    finally:
        _release(case)


# ---------------------------------------------------------------------------------------------
# max_pool2d
# ---------------------------------------------------------------------------------------------
def _max_pool(case):
    C, H, W, geo = L.POOL_CASES[case]
    ref = L.pool_reference(case)
    lib, st = _lib.lib(), _lib.current_stream(DEV)
    xb, gob = L.pool_inputs(case)
    x, go = _rep(xb), _rep(gob)
    out = _nan(go.shape)
    code = torch.full(go.shape, 255, dtype=torch.uint8, device=DEV)
    gi = _nan(x.shape)
    _lib.check(lib.tdrn_max_pool_forward(_lib.ptr(x), _lib.ptr(out), _lib.ptr(code), R, C, H, W, *geo, st))
    _lib.check(lib.tdrn_max_pool_backward(_lib.ptr(go), _lib.ptr(code), _lib.ptr(gi), R, C, H, W, *geo, st))
    torch.cuda.synchronize()
    assert _same_bits(out, ref["output"]), "%s: output bits" % case
    assert _same_bits(code, ref["code"]), "%s: codes" % case
    if geo[0] == 2:
        assert _same_bits(gi, ref["grad_input"]), "%s: grad_input bits" % case
    else:
        _replicated_fp32(case, "grad_input", gi, ref["grad_input64"])
        assert _same_bits(gi, gi[:1]), "%s: a replica's grad_input differs from the first one's" % case


@pytest.mark.parametrize("case", list(L.POOL_CASES))
def test_max_pool_past_4gib(case):
    C, H, W, geo = L.POOL_CASES[case]
    _reserve(case, (4 * 4 + 1) * R * C * H * W + 2 ** 30)       # at most (3/1/1): x, grad_input, output, grad_output, and the codes
    try:
        _max_pool(case)
    finally:
        _release(case)


# ---------------------------------------------------------------------------------------------
# l2norm
# ---------------------------------------------------------------------------------------------
def _l2norm(case):
    C, H, W = L.L2_CASES[case]
    ref = L.l2_reference(case)
    lib, dims, st = _lib.lib(), (R, C, H, W), _lib.current_stream(DEV)
    nb = lib.tdrn_l2norm_workspace_bytes(*dims)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    xb, w, gob = L.l2_inputs(case)
    x, go, w = _rep(xb), _rep(gob), w.to(DEV)
    out, norm, gi, gw = _nan(x.shape), _nan((R, H, W)), _nan(x.shape), torch.zeros(C, device=DEV)
    _lib.check(lib.tdrn_l2norm_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(out), _lib.ptr(norm), *dims, L.L2_EPS, st))
    _lib.check(lib.tdrn_l2norm_backward(_lib.ptr(x), _lib.ptr(go), _lib.ptr(w), _lib.ptr(norm), _lib.ptr(gi), _lib.ptr(gw), *dims, L.L2_EPS,
                                        1.0, _lib.ptr(ws), nb, st))
    torch.cuda.synchronize()
    _replicated_fp32(case, "output", out, ref["output"])
    _replicated_fp32(case, "grad_input", gi, ref["grad_input"])
    share = _worst(norm, ref["norm"], 1e-5 * ref["norm"].abs())
    print("%s %-12s worst share of the bound %.4f" % (case, "norm", share))
    assert share <= 1.0, (case, "norm", share)
    del out, gi
    # torch's own fp32 evaluation of grad_weight[c] = sum go x / (|x| + eps)
    norm_t = x.pow(2).sum(dim=1, keepdim=True).sqrt_().add_(L.L2_EPS)
    gw_t = x.mul_(go).div_(norm_t).sum((0, 2, 3))
    _summed(case, "grad_weight", gw, ref["grad_weight"], "fp32", gw_t)


@pytest.mark.parametrize("case", list(L.L2_CASES))
def test_l2norm_past_4gib(case):
    C, H, W = L.L2_CASES[case]
    _reserve(case, (4 + 1) * 4 * R * C * H * W + 2 ** 30)       # x, grad_output, output, grad_input; one of torch's temporaries
    try:
        _l2norm(case)
    finally:
        _release(case)


# ---------------------------------------------------------------------------------------------
# the conv families: conv2d (i-c), conv_transpose2d (i-f), conv2d at stride 2 (i-g), depthwise conv2d (i-h), conv5x5 (i-i)
# ---------------------------------------------------------------------------------------------
def _torch_grad_weight(fam, dims, xr, gr, wshape):
    """torch's fp32 GPU ops on the inputs as the op uses them: per tap one fp32 matrix product over N Ho Wo terms (a convolution
    through MIOpen would spend ten seconds a shape on its kernel search); depthwise: per tap one product and one sum"""
    Ho, Wo = gr.shape[2:]
    if fam == "convt":                          # weight (Cin, Cout, 2, 2): x[h][w] meets grad_output[2h + i][2w + j]
        taps = [torch.einsum("nchw,ndhw->cd", xr, gr[:, :, i::2, j::2]) for i in range(2) for j in range(2)]
        return torch.stack(taps, 2).reshape(wshape)
    if fam == "dw":
        k, s, pad, dil = dims[4], dims[6], dims[8], dims[10]
    else:
        k, s, pad, dil = dims[5], dims[7], dims[9], dims[11]
    xr = torch.nn.functional.pad(xr, (pad, pad, pad, pad))
    tap = lambda ky, kx: xr[:, :, ky * dil:ky * dil + s * (Ho - 1) + 1:s, kx * dil:kx * dil + s * (Wo - 1) + 1:s]
    if fam == "dw":
        return torch.stack([(gr * tap(ky, kx)).sum((0, 2, 3)) for ky in range(k) for kx in range(k)], 1).reshape(wshape)
    return torch.stack([torch.einsum("nchw,ndhw->cd", gr, tap(ky, kx)) for ky in range(k) for kx in range(k)], 2).reshape(wshape)


def _conv_family(fam, case, mode, nb):
    """the three entries of one family on R replicas: prefix and dims from tests/_train_large_cases.py"""
    prefix, dims = L.FAMILIES[fam][0], L.op_dims(case)
    tag = "%s %s" % (case, mode)
    ref, S = L.op_reference(case, mode)
    lib, dt, st = _lib.lib(), _lib.DTYPES[mode], _lib.current_stream(DEV)
    entry = lambda name: getattr(lib, "%s_%s" % (prefix, name))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    xb, w, b, gob = L.op_inputs(case)
    x, go, w, b = _rep(xb), _rep(gob), w.to(DEV), b.to(DEV)
    out, gi, gw, gb = _nan(go.shape), _nan(x.shape), torch.zeros_like(w), torch.zeros_like(b)
    _lib.check(entry("forward")(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(out), *dims, dt, _lib.ptr(ws), nb, st))
    _lib.check(entry("backward_input")(_lib.ptr(go), _lib.ptr(w), _lib.ptr(gi), *dims, dt, _lib.ptr(ws), nb, st))
    _lib.check(entry("backward_parameters")(_lib.ptr(x), _lib.ptr(go), _lib.ptr(gw), _lib.ptr(gb), *dims, 1.0, dt, _lib.ptr(ws), nb, st))
    torch.cuda.synchronize()
    del ws
    for name, big, i in (("output", out, 0), ("grad_input", gi, 1)):
        if mode == "fp32":
            _replicated_fp32(tag, name, big, ref[i])
        else:
            ratio = _worst(big, ref[i], S[i].clamp_min(1e-300))
            print("%s %-12s max|d|/S %.3e  c %.1e" % (tag, name, ratio, C_ACC[mode]))
            assert ratio <= C_ACC[mode], (tag, name, ratio)
    rows, cols = L.untouched(case)
    for r in rows:                              # an input row or column that no output pixel touches: exactly +0.0, in every replica
        assert bool((gi[:, :, r, :].contiguous().view(torch.int32) == 0).all()), "%s: grad_input row %d is not +0.0 everywhere" % (tag, r)
    for c in cols:
        assert bool((gi[:, :, :, c].contiguous().view(torch.int32) == 0).all()), "%s: grad_input column %d is not +0.0 everywhere" % (tag, c)
    if fam == "dw":                             # the header fixes the tap order of forward and backward_input
        assert _same_bits(out, out[:1]), "%s: a replica's output differs from the first one's" % tag
        assert _same_bits(gi, gi[:1]), "%s: a replica's grad_input differs from the first one's" % tag
    del out, gi, big                            # (the loop variable holds grad_input)
    xr, gr = (x, go) if mode == "fp32" else (x.to(L.CONV_MODES[mode]).float(), go.to(L.CONV_MODES[mode]).float())
    del x, go
    gb_t = gr.sum((0, 2, 3))
    gw_t = _torch_grad_weight(fam, dims, xr, gr, w.shape)
    del xr, gr
    for name, got, i, t in (("grad_weight", gw, 2, gw_t), ("grad_bias", gb, 3, gb_t)):
        _summed(tag, name, got, ref[i], "fp32" if mode == "fp32" else (C_ACC[mode], S[i]), t)


def _conv_family_test(fam, case, mode):
    xs, _, ys, _ = L.op_shapes(case)
    nb = getattr(_lib.lib(), L.FAMILIES[fam][0] + "_workspace_bytes")(*L.op_dims(case), _lib.DTYPES[mode])
    assert nb > 0
    caller = 2 * 4 * R * (xs[1] * xs[2] * xs[3] + ys[1] * ys[2] * ys[3])       # x, grad_input, output, grad_output
    _reserve("%s %s" % (case, mode), nb + caller + 2 ** 31)      # + the comparisons' temporaries (torch's side runs after the workspace is freed)
    try:
        _conv_family(fam, case, mode, nb)
    finally:
        _release("%s %s" % (case, mode))


def _cases_and_modes(fam):
    return [(c, m) for c in L.FAMILIES[fam][1] for m in L.FAMILIES[fam][2]]


@pytest.mark.parametrize("mode", list(L.CONV_MODES))
@pytest.mark.parametrize("case", list(L.CONV_CASES))
def test_conv2d_past_4gib(case, mode):
    _conv_family_test("conv", case, mode)


@pytest.mark.parametrize("case,mode", _cases_and_modes("convt"))
def test_conv_transpose2d_past_4gib(case, mode):
    _conv_family_test("convt", case, mode)


@pytest.mark.parametrize("case,mode", _cases_and_modes("s2"))
def test_conv2d_strided_past_4gib(case, mode):
    _conv_family_test("s2", case, mode)


@pytest.mark.parametrize("case,mode", _cases_and_modes("dw"))
def test_dwconv_past_4gib(case, mode):
    _conv_family_test("dw", case, mode)


@pytest.mark.parametrize("case,mode", _cases_and_modes("k5"))
def test_conv5x5_past_4gib(case, mode):
    _conv_family_test("k5", case, mode)
