"""C ABI of the dense 5x5 conv with gradients (tdrn_hip.h section i-i), no GPU needed: the workspace query and the entries decide
every error before any launch, and the plan behind the query is restated in plain Python (test_conv_grad_variants.py's dense_*, the
one restatement of the three dense families, called here at k = 5, stride 1, pad 2, dilation 1).

The forward and the input gradient (pad' = 4 - 2 = 2) are launch_conv at 25 taps; the weight gradient is conv_wgrad_kernel<DT, 5, 5>,
five kernel-row passes side by side, with a split rule of its own that counts the five workgroups of a split.  conv_igemm.hip's rules
are test_conv_grad_variants.py's too.
"""
import pytest
import torch

import test_gpu_conv5x5 as G
from test_conv_grad_variants import ES, ZERO_PAGE, cdiv, cpad, dense_problem, dense_wgrad_splits, dense_workspace_bytes, splitk, tile, up
from tdrn_amd import _lib
from tdrn_amd.model import networks

# N Cin H W Cout kH kW dH dW padH padW dilH dilW
GOOD = (2, 6, 9, 7, 4, 5, 5, 1, 1, 2, 2, 1, 1)
NAMES = "N Cin H W Cout kH kW dH dW padH padW dilH dilW".split()
TYPES = (_lib.F32, _lib.BF16, _lib.F16)
FAMILY = ("tdrn_conv5x5_workspace_bytes", "tdrn_conv5x5_forward", "tdrn_conv5x5_backward_input", "tdrn_conv5x5_backward_parameters")


def _entries(lib, dims, dt, nb, p=256, family="tdrn_conv5x5"):
    """all three entries on fake non-null pointers.  Pointers are only compared with NULL before any launch, so this is called
    only where a check ahead of the first launch fails (bad geometry or a short workspace): a fake pointer never reaches a kernel."""
    q = getattr(lib, family + "_workspace_bytes")(*dims, dt)
    assert q == 0 or nb < q
    return (getattr(lib, family + "_forward")(p, p, None, p, *dims, dt, p, nb, None),
            getattr(lib, family + "_backward_input")(p, p, p, *dims, dt, p, nb, None),
            getattr(lib, family + "_backward_parameters")(p, p, p, None, *dims, 1.0, dt, p, nb, None))


def _with(**kw):
    d = dict(zip(NAMES, GOOD))
    d.update(kw)
    return tuple(d[n] for n in NAMES)


def test_symbols_exist():
    lib = _lib.lib()
    for name in FAMILY:
        assert name in _lib.EXPORTS and getattr(lib, name) is not None


def test_query_positive_for_every_case_and_for_the_models_layers():
    lib = _lib.lib()
    for case in G.CASES:
        for dt in TYPES:
            assert lib.tdrn_conv5x5_workspace_bytes(*G._dims(case), dt) > 0, (case, dt)
    # odm_loc_2 (12) and odm_conf_2 for 21, 31 and 81 classes, on the pyramids of 320 px and 192 px frames, batch 1 to 32
    for cout in (12, 63, 93, 243):
        for hw in (40, 20, 10, 5, 24, 12, 6, 3):
            for n in (1, 2, 8, 32):
                for dt in TYPES:
                    assert lib.tdrn_conv5x5_workspace_bytes(*_with(N=n, Cin=256, Cout=cout, H=hw, W=hw), dt) > 0, (cout, hw, n, dt)
    # 2^30 padded input elements: half the limit
    assert all(lib.tdrn_conv5x5_workspace_bytes(*_with(N=64, Cin=256, H=256, W=256, Cout=64), dt) > 0 for dt in TYPES)


@pytest.mark.parametrize("dims", [_with(N=0), _with(Cin=0), _with(H=-1), _with(W=0), _with(Cout=0), _with(kH=0), _with(kW=-2),
                                  _with(dH=0), _with(dW=-1), _with(dilH=0), _with(dilW=-1), _with(padH=-1), _with(padW=-1),
                                  _with(H=2, W=2, padH=0, padW=0),          # an output smaller than 1 x 1
                                  _with(H=9, W=2, padH=2, padW=0)])
def test_bad_sizes_are_shape_errors(dims):
    lib = _lib.lib()
    for dt in TYPES:
        assert lib.tdrn_conv5x5_workspace_bytes(*dims, dt) == 0
        assert _entries(lib, dims, dt, 1 << 20) == (-2, -2, -2)


def test_a_bad_type_is_an_argument_error_between_shape_and_geometry():
    lib = _lib.lib()
    p = 256
    for dt in (-1, 3):
        assert lib.tdrn_conv5x5_workspace_bytes(*GOOD, dt) == 0
        assert _entries(lib, GOOD, dt, 1 << 20) == (-1, -1, -1)
        assert lib.tdrn_conv5x5_forward(p, p, None, p, *_with(N=0), dt, p, 1 << 20, None) == -2          # a bad size comes first
        assert lib.tdrn_conv5x5_forward(p, p, None, p, *_with(kH=3, kW=3), dt, p, 1 << 20, None) == -1    # the type before the geometry


UNCOVERED = [
    _with(kH=3, kW=3, padH=1, padW=1),                   # k = 3: section i-c's
    _with(kH=3, kW=3),                                   # k = 3 at pad 2
    _with(kH=1, kW=1, padH=0, padW=0),                   # k = 1
    _with(kH=7, kW=7, padH=3, padW=3),                   # k = 7
    _with(dH=2, dW=2),                                   # stride 2
    _with(dH=1, dW=2),                                   # per-axis stride
    _with(padH=1, padW=1), _with(padH=3, padW=3),        # pad 1, pad 3
    _with(padH=0, padW=0),                               # pad 0
    _with(padH=2, padW=1),                               # per-axis pad
    _with(dilH=2, dilW=2), _with(dilH=2, dilW=2, padH=4, padW=4),    # dilation 2
    _with(kH=5, kW=3), _with(kH=3, kW=5),                # not square
    _with(N=128, Cin=256, H=256, W=256, Cout=8),         # N H W CiPad = 2^31
    _with(N=128, Cin=8, H=256, W=256, Cout=256),         # N H W CoPad = 2^31, N H W CiPad below it
]


@pytest.mark.parametrize("dims", UNCOVERED)
def test_uncovered_geometry_is_unsupported(dims):
    lib = _lib.lib()
    for dt in TYPES:
        assert lib.tdrn_conv5x5_workspace_bytes(*dims, dt) == 0
        assert _entries(lib, dims, dt, 1 << 20) == (-4, -4, -4)


def test_the_size_limits_are_where_the_comments_say():
    lib = _lib.lib()
    for dims, big, small in ((UNCOVERED[-2], "Cin", "Cout"), (UNCOVERED[-1], "Cout", "Cin")):
        d = dict(zip(NAMES, dims))
        assert d["N"] * d["H"] * d["W"] * cpad(d[big]) == 2 ** 31 and d["N"] * d["H"] * d["W"] * cpad(d[small]) < 2 ** 31
        # one image less is inside the limit
        assert all(lib.tdrn_conv5x5_workspace_bytes(*_with(**dict(d, N=127)), dt) > 0 for dt in TYPES)


def test_the_two_families_are_disjoint():
    lib = _lib.lib()
    for dt in TYPES:
        # section i-c still refuses k = 5 ...
        assert lib.tdrn_conv2d_workspace_bytes(*GOOD, dt) == 0
        assert _entries(lib, GOOD, dt, 1 << 20, family="tdrn_conv2d") == (-4, -4, -4)
        # ... and serves k = 3, which this family refuses
        k3 = _with(kH=3, kW=3, padH=1, padW=1)
        assert lib.tdrn_conv2d_workspace_bytes(*k3, dt) > 0 and lib.tdrn_conv5x5_workspace_bytes(*k3, dt) == 0
    x, w = torch.zeros(1, 3, 8, 8), torch.zeros(4, 3, 5, 5)
    with pytest.raises(NotImplementedError):
        networks.conv2d(x, w, None, 2)


def test_short_workspace_and_null_pointers():
    lib = _lib.lib()
    p = 256
    for dt in TYPES:
        nb = lib.tdrn_conv5x5_workspace_bytes(*GOOD, dt)
        assert _entries(lib, GOOD, dt, nb - 1) == (-3, -3, -3)
        assert lib.tdrn_conv5x5_forward(p, p, None, p, *GOOD, dt, None, nb, None) == -3            # no workspace at all
        assert lib.tdrn_conv5x5_backward_input(p, p, p, *GOOD, dt, None, nb, None) == -3
        assert lib.tdrn_conv5x5_backward_parameters(p, p, p, None, *GOOD, 1.0, dt, None, nb, None) == -3
        # a null tensor pointer is refused first, whatever else is passed: every call below has one
        assert lib.tdrn_conv5x5_forward(None, p, None, p, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv5x5_forward(p, None, None, p, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv5x5_forward(p, p, None, None, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv5x5_backward_input(None, p, p, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv5x5_backward_input(p, None, p, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv5x5_backward_input(p, p, None, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv5x5_backward_parameters(None, p, p, None, *GOOD, 1.0, dt, p, nb, None) == -1
        assert lib.tdrn_conv5x5_backward_parameters(p, None, p, None, *GOOD, 1.0, dt, p, nb, None) == -1
        assert lib.tdrn_conv5x5_backward_parameters(p, p, None, None, *GOOD, 1.0, dt, p, nb, None) == -1
        # ... also in front of a bad geometry and of a short workspace
        assert lib.tdrn_conv5x5_forward(None, p, None, p, *_with(N=0), dt, None, 0, None) == -1
        assert lib.tdrn_conv5x5_backward_input(p, p, None, *_with(kH=3, kW=3), dt, None, 0, None) == -1
        # a shape error comes before an uncovered geometry, that before the workspace
        assert lib.tdrn_conv5x5_forward(p, p, None, p, *_with(N=0, kH=3, kW=3), dt, None, 0, None) == -2
        assert lib.tdrn_conv5x5_forward(p, p, None, p, *_with(kH=3, kW=3), dt, None, 0, None) == -4


def test_module_has_nn_conv2d_parameters():
    m, r = networks.Conv5x5(5, 7), torch.nn.Conv2d(5, 7, 5, padding=2)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in r.state_dict().items()}
    assert networks.Conv5x5(5, 7, bias=False).bias is None
    assert list(networks.Conv5x5(5, 7, bias=False).state_dict()) == list(torch.nn.Conv2d(5, 7, 5, padding=2, bias=False).state_dict())
    m.load_state_dict(r.state_dict())
    assert torch.equal(m.weight, r.weight) and torch.equal(m.bias, r.bias)
    torch.manual_seed(3)
    r.reset_parameters()
    torch.manual_seed(3)
    m.reset_parameters()
    assert torch.equal(m.weight, r.weight) and torch.equal(m.bias, r.bias)


def test_cpu_tensors_and_other_weights_raise():
    x, w, b = torch.zeros(1, 3, 8, 8), torch.zeros(4, 3, 5, 5), torch.zeros(4)
    with pytest.raises(NotImplementedError):
        networks.conv5x5(x, w, b)
    with pytest.raises(NotImplementedError):
        networks.Conv5x5Function.apply(x, w, None, "fp32")
    with pytest.raises(NotImplementedError):
        networks.Conv5x5(3, 4)(x)
    with pytest.raises(ValueError):
        networks.conv5x5(x[0], w, b)
    # the geometry check needs no device: another kernel raises and names what is covered
    for shape in ((4, 3, 3, 3), (4, 3, 5, 3), (4, 3, 1, 1), (4, 3, 7, 7)):
        with pytest.raises(RuntimeError, match="kernel 5 x 5, stride 1, padding 2, dilation 1"):
            networks._conv5x5_geometry(x, torch.zeros(shape))
    with pytest.raises(RuntimeError, match="invalid number of input planes"):
        networks._conv5x5_geometry(x, torch.zeros(4, 2, 5, 5))
    assert networks._conv5x5_geometry(x, w) == ((1, 3, 8, 8, 4, 5, 5, 1, 1, 2, 2, 1, 1), (1, 4, 8, 8))


# ---- the plan, restated ---------------------------------------------------------------------------------------------------------
def _dense(case):
    """a case as the arguments of test_conv_grad_variants.py's dense_*: N, Cin, H, W, Cout, k = 5, stride 1, pad 2, dil 1"""
    return G.CASES[case] + (5, 1, 2, 1)


def problem(case, dgrad):
    """the implicit GEMM of the forward or of the input gradient, both 5x5 at pad 2 (pad' = 4 - 2) over H x W pixels"""
    p = dense_problem(*_dense(case), dgrad)
    assert (p["H"], p["W"], p["Ho"], p["Wo"], p["pad"]) == G.CASES[case][2:4] * 2 + (2,)
    return p


def wgrad_splits(case):
    """conv_wgrad_splits at k = 5: five workgroups (the kernel rows) per split and tile -> (splits, per_split, M)"""
    return dense_wgrad_splits(*_dense(case))


def workspace_bytes(case, mode):
    return dense_workspace_bytes(*_dense(case), mode)


@pytest.mark.parametrize("mode", list(ES))
@pytest.mark.parametrize("case", list(G.CASES))
def test_restated_plan_reproduces_the_workspace_query(case, mode):
    assert _lib.lib().tdrn_conv5x5_workspace_bytes(*G._dims(case), _lib.DTYPES[mode]) == workspace_bytes(case, mode)


def test_the_split_rule_of_the_other_kernel_sizes_did_not_move():
    """k = 1 | 3 keep cdiv(512, tiles): their restated workspace (test_conv_grad_variants.py, test_conv_strided_abi.py) still matches,
    and a layer whose split count the two rules tell apart sits where the old rule puts it.  The arithmetic is written out here, not
    taken from dense_wgrad_splits: that restatement must tell the two rules apart the same way."""
    lib = _lib.lib()
    # 256 -> 256 on 40 x 40, batch 8: tiles = 16, M = 12800: the old rule asks for 32 splits and gets 29 of 448 pixels; counting five
    # workgroups per split would ask for 7
    dims = (8, 256, 40, 40, 256, 3, 3, 1, 1, 1, 1, 1, 1)
    M, S = 12800, 29
    assert min(cdiv(512, 16), cdiv(M, 256)) == 32 and cdiv(M, up(cdiv(M, 32), 64)) == S and cdiv(512, 5 * 16) == 7
    assert dense_wgrad_splits(8, 256, 40, 40, 256, 3, 1, 1, 1) == (S, 448, M) and dense_wgrad_splits(8, 256, 40, 40, 256, 5, 1, 2, 1)[0] == 7
    slab = up(S * 9 * 256 * 256 * 4, 256) + up(S * 256 * 4, 256)
    head = ZERO_PAGE + 2 * up(M * 256 * 4, 256)
    assert lib.tdrn_conv2d_workspace_bytes(*dims, _lib.F32) == head + slab        # the slabs are the larger branch of the layout


def test_each_case_reaches_its_variant():
    # the kernel is larger than the image: whole taps and whole kernel rows lie in the padding
    for case, hw in (("one_pixel", 1), ("two_by_two", 2), ("three_by_three", 3)):
        assert G.CASES[case][2:4] == (hw, hw) and hw < 5
    # chunks cross image boundaries
    N, Cin, H, W, Cout = G.CASES["five_n3"]
    assert (N, H * W) == (3, 25) and N * H * W > 64
    # padded channels: Cin 6, Cout 12 / 63 / 75 (the last in two cout tiles); two cin tiles
    assert {G.CASES[c][1] for c in ("one_pixel", "three_by_three", "five_n3")} == {6}
    assert {G.CASES[c][4] for c in ("one_pixel", "three_by_three", "five_n3")} == {12, 63, 75}
    assert cpad(75) // 64 == 2 and cpad(G.CASES["two_by_two"][1]) // 64 == 2
    # wgrad splits: a ragged last split; more than one K split
    S, per, M = wgrad_splits("m800")
    assert (S, per, M, M % 64) == (4, 256, 800, 32)
    assert wgrad_splits("k_split") == (25, 256, 6400)
    assert wgrad_splits("one_pixel") == (1, 64, 2)
    # the model's eight layers at 192 px, batch 2
    for lvl in (24, 12, 6, 3):
        assert G.CASES["loc_%d" % lvl] == (2, 256, lvl, lvl, 12) and G.CASES["conf_%d" % lvl] == (2, 256, lvl, lvl, 63)
    # the small maps run the forward and the input gradient split-K at 25 taps
    for mode in ES:
        for lvl in (6, 3):
            assert splitk(problem("conf_%d" % lvl, False), ES[mode]) > 1 and splitk(problem("conf_%d" % lvl, True), ES[mode]) > 1
    # no case reaches the deep tile
    for case in G.CASES:
        for dgrad in (False, True):
            assert tile(problem(case, dgrad)) != "256x128", (case, dgrad)
