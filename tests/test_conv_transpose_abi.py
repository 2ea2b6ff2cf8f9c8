"""C ABI of ConvTranspose2d(kernel 2, stride 2) with gradients (tdrn_hip.h section i-f), no GPU needed: the workspace query and
the entries decide every error before any launch, and the plan behind the query is restated here in plain Python.

The forward is launch_conv with phases = 4 (four 1x1 GEMMs of M = N H W rows, one per output phase), the input gradient a 1x1 conv
over the space-to-depth image of grad_output (4 CoPad input channels), the weight gradient the one-tap wgrad GEMM over the same
image (4 CoPad "output channels").  conv_igemm.hip's rules are test_conv_grad_variants.py's; the library multiplies the workgroup
counts of its two thresholds (the 256x128 tile, split-K) by the number of phases, which the restatement here does as well.
"""
import pytest
import torch

import test_gpu_conv_transpose as G
from test_conv_grad_variants import ES, ZERO_PAGE, cdiv, cpad, n_pad, splitk, tile, up
from tdrn_amd import _lib
from tdrn_amd.model import networks

# N Cin H W Cout kH kW dH dW padH padW opadH opadW dilH dilW
GOOD = (2, 6, 5, 7, 10, 2, 2, 2, 2, 0, 0, 0, 0, 1, 1)
TYPES = (_lib.F32, _lib.BF16, _lib.F16)


def _entries(lib, dims, dt, nb, p=256):
    """all three entries on fake non-null pointers.  Pointers are only compared with NULL before any launch, so this is called
    only where a check ahead of the first launch fails (bad geometry or a short workspace): a fake pointer never reaches a kernel."""
    q = lib.tdrn_conv_transpose2d_workspace_bytes(*dims, dt)
    assert q == 0 or nb < q
    return (lib.tdrn_conv_transpose2d_forward(p, p, None, p, *dims, dt, p, nb, None),
            lib.tdrn_conv_transpose2d_backward_input(p, p, p, *dims, dt, p, nb, None),
            lib.tdrn_conv_transpose2d_backward_parameters(p, p, p, None, *dims, 1.0, dt, p, nb, None))


def _with(**kw):
    names = "N Cin H W Cout kH kW dH dW padH padW opadH opadW dilH dilW".split()
    d = dict(zip(names, GOOD))
    d.update(kw)
    return tuple(d[n] for n in names)


def test_query_positive_for_every_case():
    lib = _lib.lib()
    for case in G.CASES:
        for dt in TYPES:
            assert lib.tdrn_conv_transpose2d_workspace_bytes(*G._dims(case), dt) > 0, (case, dt)
    # the three TCB levels at batch 32
    for hw in (5, 10, 20):
        for dt in TYPES:
            assert lib.tdrn_conv_transpose2d_workspace_bytes(*_with(N=32, Cin=256, Cout=256, H=hw, W=hw), dt) > 0
    # 2^30 padded elements on both sides: half the limit
    assert all(lib.tdrn_conv_transpose2d_workspace_bytes(*_with(N=64, Cin=256, H=256, W=256, Cout=64), dt) > 0 for dt in TYPES)


@pytest.mark.parametrize("dims", [_with(N=0), _with(Cin=0), _with(H=-1), _with(W=0), _with(Cout=0), _with(kH=0), _with(kW=-2),
                                  _with(dH=0), _with(dW=-1), _with(dilH=0), _with(dilW=-1), _with(padH=-1), _with(padW=-1),
                                  _with(opadH=-1)])
def test_bad_sizes_are_shape_errors(dims):
    lib = _lib.lib()
    for dt in TYPES:
        assert lib.tdrn_conv_transpose2d_workspace_bytes(*dims, dt) == 0
        assert _entries(lib, dims, dt, 1 << 20) == (-2, -2, -2)


@pytest.mark.parametrize("dims", [
    _with(dH=1, dW=1),                                   # stride 1
    _with(kH=3, kW=3),                                   # k = 3
    _with(padH=1, padW=1),                               # pad 1
    _with(opadH=1, opadW=1),                             # output_padding 1
    _with(dilH=2, dilW=2),                               # dilation 2
    _with(kH=2, kW=3), _with(kH=1, kW=2),                # not square
    _with(dH=2, dW=1),                                   # per-axis stride
    _with(N=128, Cin=256, H=256, W=256, Cout=8),         # N H W CiPad = 2^31
    _with(N=32, Cin=8, H=256, W=256, Cout=256),          # N H W 4 CoPad = 2^31
])
def test_uncovered_geometry_is_unsupported(dims):
    lib = _lib.lib()
    for dt in TYPES:
        assert lib.tdrn_conv_transpose2d_workspace_bytes(*dims, dt) == 0
        assert _entries(lib, dims, dt, 1 << 20) == (-4, -4, -4)


def test_short_workspace_and_null_pointers():
    lib = _lib.lib()
    p = 256
    for dt in TYPES:
        nb = lib.tdrn_conv_transpose2d_workspace_bytes(*GOOD, dt)
        assert _entries(lib, GOOD, dt, nb - 1) == (-3, -3, -3)
        assert lib.tdrn_conv_transpose2d_forward(p, p, None, p, *GOOD, dt, None, nb, None) == -3            # no workspace at all
        assert lib.tdrn_conv_transpose2d_backward_input(p, p, p, *GOOD, dt, None, nb, None) == -3
        assert lib.tdrn_conv_transpose2d_backward_parameters(p, p, p, None, *GOOD, 1.0, dt, None, nb, None) == -3
        # a null tensor pointer is refused first, whatever else is passed: every call below has one
        assert lib.tdrn_conv_transpose2d_forward(None, p, None, p, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv_transpose2d_forward(p, None, None, p, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv_transpose2d_forward(p, p, None, None, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv_transpose2d_backward_input(None, p, p, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv_transpose2d_backward_input(p, None, p, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv_transpose2d_backward_input(p, p, None, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv_transpose2d_backward_parameters(None, p, p, None, *GOOD, 1.0, dt, p, nb, None) == -1
        assert lib.tdrn_conv_transpose2d_backward_parameters(p, None, p, None, *GOOD, 1.0, dt, p, nb, None) == -1
        assert lib.tdrn_conv_transpose2d_backward_parameters(p, p, None, None, *GOOD, 1.0, dt, p, nb, None) == -1
        # ... also in front of a bad geometry and of a short workspace
        assert lib.tdrn_conv_transpose2d_forward(None, p, None, p, *_with(N=0), dt, None, 0, None) == -1
        assert lib.tdrn_conv_transpose2d_backward_input(p, p, None, *_with(kH=3, kW=3), dt, None, 0, None) == -1


def test_module_has_nn_conv_transpose2d_parameters():
    m, r = networks.ConvTranspose2d(5, 7, 2, 2), torch.nn.ConvTranspose2d(5, 7, 2, 2, 0)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in r.state_dict().items()}
    assert tuple(m.weight.shape) == (5, 7, 2, 2)
    assert networks.ConvTranspose2d(5, 7, bias=False).bias is None
    m.load_state_dict(r.state_dict())
    # reset_parameters is nn.ConvTranspose2d's: the same draws from the same generator state
    torch.manual_seed(3)
    r.reset_parameters()
    torch.manual_seed(3)
    m.reset_parameters()
    assert torch.equal(m.weight, r.weight) and torch.equal(m.bias, r.bias)


def test_rejects_cpu_tensors():
    x, w, b = torch.zeros(1, 3, 4, 4), torch.zeros(3, 4, 2, 2), torch.zeros(4)
    with pytest.raises(NotImplementedError):
        networks.ConvTranspose2dFunction.apply(x, w, None, 2)
    with pytest.raises(NotImplementedError):
        networks.conv_transpose2d(x, w, b)
    with pytest.raises(NotImplementedError):
        networks.ConvTranspose2d(3, 4)(x)
    with pytest.raises(ValueError):
        networks.conv_transpose2d(torch.zeros(3, 4, 4), w)


# ---- the plan, restated ---------------------------------------------------------------------------------------------------------
def problem(case, dgrad):
    """the implicit GEMM of the forward (four phases) or of the input gradient"""
    N, Cin, H, W, Cout = G.CASES[case]
    if not dgrad:
        return dict(B=N, H=H, W=W, Cin=cpad(Cin), Ho=H, Wo=W, Cout=Cout, Npad=n_pad(Cout), k=1, pad=0, phases=4)
    return dict(B=N, H=H, W=W, Cin=4 * cpad(Cout), Ho=H, Wo=W, Cout=Cin, Npad=n_pad(Cin), k=1, pad=0, phases=1)


def splitk_phases(p, es):
    """igemm_splitk_choice with its workgroup count multiplied by the phases"""
    if p["phases"] == 1:
        return splitk(p, es)
    nk = p["k"] * p["k"] * (p["Cin"] // (128 // es))
    bn = 128 if p["Npad"] % 128 == 0 else (64 if p["Npad"] % 64 == 0 else 32)
    blocks = cdiv(p["B"] * p["Ho"] * p["Wo"], 128) * (p["Npad"] // bn) * p["phases"]
    if blocks >= 160 or nk < 8:
        return 1
    s = min(cdiv(384, blocks), nk // 4, 16)
    return 1 if s < 2 else s


def tile_phases(p):
    """launch_dt's choice: big_tiles counts the phases"""
    if p["phases"] == 1:
        return tile(p)
    M = p["B"] * p["Ho"] * p["Wo"]
    if p["Npad"] % 128 == 0 and cdiv(M, 256) * (p["Npad"] // 128) * p["phases"] >= 512:
        return "256x128"
    return "128x128" if p["Npad"] % 128 == 0 else ("128x64" if p["Npad"] % 64 == 0 else "128x32")


def wgrad_splits(case):
    """conv_wgrad_splits on ConvBwdGeom{N, Cin, H, W, 4 CoPad, 1, 0, 1, H, W} -> (splits, per_split, M)"""
    N, Cin, H, W, Cout = G.CASES[case]
    M = N * H * W
    tiles = (cpad(Cin) // 64) * (4 * cpad(Cout) // 64)
    S = max(1, min(cdiv(512, tiles), cdiv(M, 4 * 64)))
    per = up(cdiv(M, S), 64)
    return cdiv(M, per), per, M


def workspace_bytes(case, mode):
    """conv_train_layout on convt2d_plan's two launches (api.hip), from the restated rules"""
    N, Cin, H, W, Cout = G.CASES[case]
    es, C4 = ES[mode], 4 * cpad(Cout)
    f, d = problem(case, False), problem(case, True)
    o = ZERO_PAGE + up(N * H * W * cpad(Cin) * es, 256) + up(N * H * W * C4 * es, 256)
    S = wgrad_splits(case)[0]
    slab_end = o + up(S * C4 * cpad(Cin) * 4, 256) + up(S * C4 * 4, 256)
    o += up(max(4 * f["Npad"] * cpad(Cin), d["Npad"] * C4) * es, 256)
    o += up(max(f["Npad"], d["Npad"]) * 4, 256)
    o += up(max(N * 4 * H * W * Cout, N * H * W * Cin) * 4, 256)
    partial = 0
    for p in (f, d):
        s = splitk_phases(p, es)
        partial = max(partial, s * p["phases"] * p["B"] * p["Ho"] * p["Wo"] * p["Npad"] * 4 if s > 1 else 0)
    return max(o + up(partial, 256), slab_end)


@pytest.mark.parametrize("mode", list(ES))
@pytest.mark.parametrize("case", list(G.CASES))
def test_restated_plan_reproduces_the_workspace_query(case, mode):
    assert _lib.lib().tdrn_conv_transpose2d_workspace_bytes(*G._dims(case), _lib.DTYPES[mode]) == workspace_bytes(case, mode)


def test_the_phase_aware_restatements_agree_with_the_imported_rules_at_one_phase():
    for case in G.CASES:
        p = problem(case, True)
        assert p["phases"] == 1
        for es in ES.values():
            assert splitk_phases(dict(p, phases=4), es) <= splitk(p, es) == splitk_phases(p, es)
        assert tile_phases(p) == tile(p)


@pytest.mark.parametrize("mode", list(ES))
def test_each_case_reaches_its_variant(mode):
    es = ES[mode]
    # deep_fwd: the 256x128 tile at the threshold exactly (512 workgroups over the four phases), the last M-tile holding one row,
    # columns past Cout, whole K
    p = problem("deep_fwd", False)
    M = p["B"] * p["Ho"] * p["Wo"]
    assert tile_phases(p) == "256x128" and M == 3841 and M % 256 == 1
    assert cdiv(M, 256) * (p["Npad"] // 128) * 4 == 512 and p["Cout"] < p["Npad"] == 1024 and splitk_phases(p, es) == 1
    # no other case reaches the deep tile, in either direction
    for case in G.CASES:
        for dgrad in (False, True):
            if (case, dgrad) != ("deep_fwd", False):
                assert tile_phases(problem(case, dgrad)) != "256x128", (case, dgrad)
    # split-K: forward through four phases, the input gradient of the real channels
    assert splitk_phases(problem("splitk_fwd", False), es) > 1
    assert splitk_phases(problem("tcb_small", True), es) > 1
    # the scalar epilogue with phases: o_pc = Cout is no multiple of 4
    assert G.CASES["odd_ragged"][4] % 4 != 0 and G.CASES["odd_ragged"][3] % 2 == 1
    assert G.CASES["deep_fwd"][4] % 4 == 0 and G.CASES["tcb_small"][4] % 4 == 0          # ... and the 16-byte stores
    # wgrad splits
    assert wgrad_splits("k_split")[0] == 7
    S, per, M = wgrad_splits("k_ragged")
    assert (S, M, M - (S - 1) * per) == (4, 798, 30)
    assert wgrad_splits("one_pixel") == (1, 64, 3)
    # several cin tiles, and padding rows inside each phase block of the space-to-depth image
    N, Cin, H, W, Cout = G.CASES["ragged_tiles"]
    assert cpad(Cin) // 64 == 3 and 4 * cpad(Cout) == 768 and cpad(Cout) - Cout == 62


def test_split_k_slices():
    assert [splitk_phases(problem("splitk_fwd", False), ES[m]) for m in ("fp32", "bf16", "fp16")] == [4, 2, 2]
    assert [splitk_phases(problem("tcb_small", True), ES[m]) for m in ("fp32", "bf16", "fp16")] == [8, 4, 4]
