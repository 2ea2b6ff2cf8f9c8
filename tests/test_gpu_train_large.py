"""The training ops (tdrn_hip.h sections i-c, i-d, i-e) on tensors of more than 2^30 elements: past 2^32 bytes in fp32, past 2^31
bytes in the conv's 16-bit staging.  The ABI admits up to 2^31 elements; conv1_2's activation at batch 32 and 512 pixels has 2^29.

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
The sums over the whole batch (parameter gradients, batch statistics) add 2 * 10^7 terms per value, a count at which nobody has
measured fp32 accumulation.  For those the bound is max(the bound above, 4 x the error of torch's own fp32 GPU reductions of the
same quantity against the same float64 reference), test_short_training_run_with_pool_and_l2norm_follows_float64's rule, taken
elementwise.  Both errors are printed.  torch's side is built from reductions over the whole tensor (var_mean, sum) and, for the
conv's weight gradient, one fp32 matrix product per tap.  Measured on an MI355X: no sum of the library's uses more than 0.0225 of
the project bound alone (the conv's fp32 grad_weight), no replicated result more than 0.0135 (l2norm's norm).  torch's reductions
stay below 0.011 of the project bound, its matrix products of 2 * 10^7 terms do not: 0.39 to 1.32 of it, so for the conv's
grad_weight the rule allows up to 5.3 times the project bound on some elements.  The library does not need that room.

Memory: each test works out an upper bound of what it needs and skips only if torch.cuda.mem_get_info() shows less (measured
peaks: conv fp32 24.3 GiB, bf16 19.5 GiB; batch_norm 19.6 GiB; max_pool 3/1/1 20.8 GiB; l2norm 19.7 GiB); everything is released
at the end of each test.
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
# conv2d
# ---------------------------------------------------------------------------------------------
def _conv_dims(case):
    Cin, H, W, Cout, k, pad, dil = L.CONV_CASES[case]
    return (R, Cin, H, W, Cout, k, k, 1, 1, pad, pad, dil, dil)


def _conv2d(case, mode, nb):
    Cin, H, W, Cout, k, pad, dil = L.CONV_CASES[case]
    tag = "%s %s" % (case, mode)
    ref, S = L.conv_reference(case, mode)
    lib, dims, dt, st = _lib.lib(), _conv_dims(case), _lib.DTYPES[mode], _lib.current_stream(DEV)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    xb, w, b, gob = L.conv_inputs(case)
    x, go, w, b = _rep(xb), _rep(gob), w.to(DEV), b.to(DEV)
    out, gi, gw, gb = _nan(go.shape), _nan(x.shape), torch.zeros_like(w), torch.zeros_like(b)
    _lib.check(lib.tdrn_conv2d_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(out), *dims, dt, _lib.ptr(ws), nb, st))
    _lib.check(lib.tdrn_conv2d_backward_input(_lib.ptr(go), _lib.ptr(w), _lib.ptr(gi), *dims, dt, _lib.ptr(ws), nb, st))
    _lib.check(lib.tdrn_conv2d_backward_parameters(_lib.ptr(x), _lib.ptr(go), _lib.ptr(gw), _lib.ptr(gb), *dims, 1.0, dt, _lib.ptr(ws), nb, st))
    torch.cuda.synchronize()
    del ws
    for name, big, i in (("output", out, 0), ("grad_input", gi, 1)):
        if mode == "fp32":
            _replicated_fp32(tag, name, big, ref[i])
        else:
            ratio = _worst(big, ref[i], S[i].clamp_min(1e-300))
            print("%s %-12s max|d|/S %.3e  c %.1e" % (tag, name, ratio, C_ACC[mode]))
            assert ratio <= C_ACC[mode], (tag, name, ratio)
    del out, gi
    # torch's fp32 GPU ops on the inputs as the op uses them: per tap one fp32 matrix product [Cout, N Ho Wo] x [N Ho Wo, Cin] (a
    # convolution through MIOpen would spend ten seconds a shape on its kernel search)
    xr, gr = (x, go) if mode == "fp32" else (x.to(L.CONV_MODES[mode]).float(), go.to(L.CONV_MODES[mode]).float())
    del x, go
    gb_t = gr.sum((0, 2, 3))
    xr = torch.nn.functional.pad(xr, (pad, pad, pad, pad))
    Ho, Wo = gr.shape[2:]
    gw_t = torch.stack([torch.einsum("nchw,ndhw->cd", gr, xr[:, :, ky * dil:ky * dil + Ho, kx * dil:kx * dil + Wo])
                        for ky in range(k) for kx in range(k)], 2).reshape(w.shape)
    for name, got, i, t in (("grad_weight", gw, 2, gw_t), ("grad_bias", gb, 3, gb_t)):
        _summed(tag, name, got, ref[i], "fp32" if mode == "fp32" else (C_ACC[mode], S[i]), t)


@pytest.mark.parametrize("mode", list(L.CONV_MODES))
@pytest.mark.parametrize("case", list(L.CONV_CASES))
def test_conv2d_past_4gib(case, mode):
    Cin, H, W, Cout, k, pad, dil = L.CONV_CASES[case]
    Ho, Wo = L.conv_out_hw(case)
    nb = _lib.lib().tdrn_conv2d_workspace_bytes(*_conv_dims(case), _lib.DTYPES[mode])
    assert nb > 0
    caller = 2 * 4 * R * (Cin * H * W + Cout * Ho * Wo)          # x, grad_input, output, grad_output
    _reserve("%s %s" % (case, mode), nb + caller + 2 ** 31)      # + the comparisons' temporaries (torch's side runs after the workspace is freed)
    try:
        _conv2d(case, mode, nb)
    finally:
        _release("%s %s" % (case, mode))
