"""C ABI of the dense 3x3 stride-2 conv with gradients (tdrn_hip.h section i-g), no GPU needed: the workspace query and the entries
decide every error before any launch, and the plan behind the query is restated in plain Python (test_conv_grad_variants.py's
dense_*, the one restatement of the three dense families, called here at k = 3, stride 2, dilation 1).

The forward is launch_conv at stride 2, the input gradient a stride-1 3x3 conv with pad' = 2 - pad over the zero-inserted image of
grad_output (CoPad input channels, H + 2 pad - 2 rows and W + 2 pad - 2 columns), the weight gradient conv_wgrad_kernel<DT, 9> with
the output pixel stepped by 2 (K = N Ho Wo).  conv_igemm.hip's rules are test_conv_grad_variants.py's too.
"""
import pytest
import torch

import test_gpu_conv_strided as G
from test_conv_grad_variants import ES, cpad, dense_geometry, dense_problem, dense_wgrad_splits, dense_workspace_bytes, splitk, tile
from tdrn_amd import _lib
from tdrn_amd.model import networks

# N Cin H W Cout kH kW dH dW padH padW dilH dilW
GOOD = (2, 6, 9, 7, 4, 3, 3, 2, 2, 1, 1, 1, 1)
NAMES = "N Cin H W Cout kH kW dH dW padH padW dilH dilW".split()
TYPES = (_lib.F32, _lib.BF16, _lib.F16)
FAMILY = ("tdrn_conv2d_strided_workspace_bytes", "tdrn_conv2d_strided_forward", "tdrn_conv2d_strided_backward_input",
          "tdrn_conv2d_strided_backward_parameters")


def _entries(lib, dims, dt, nb, p=256, family="tdrn_conv2d_strided"):
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


def test_query_positive_for_every_case():
    lib = _lib.lib()
    for case in G.CASES:
        for dt in TYPES:
            assert lib.tdrn_conv2d_strided_workspace_bytes(*G._dims(case), dt) > 0, (case, dt)
    # the extras layer at 320 and 512 px, batch 32; pads 0, 1, 2
    for hw in (10, 16):
        for pad in (0, 1, 2):
            for dt in TYPES:
                assert lib.tdrn_conv2d_strided_workspace_bytes(*_with(N=32, Cin=256, Cout=512, H=hw, W=hw, padH=pad, padW=pad), dt) > 0
    # the smallest input of every pad: a 1 x 1 output
    for pad, hw in ((0, 3), (1, 1), (2, 1)):
        assert all(lib.tdrn_conv2d_strided_workspace_bytes(*_with(H=hw, W=hw, padH=pad, padW=pad), dt) > 0 for dt in TYPES)
    # 2^30 padded input elements: half the limit
    assert all(lib.tdrn_conv2d_strided_workspace_bytes(*_with(N=64, Cin=256, H=256, W=256, Cout=64), dt) > 0 for dt in TYPES)


@pytest.mark.parametrize("dims", [_with(N=0), _with(Cin=0), _with(H=-1), _with(W=0), _with(Cout=0), _with(kH=0), _with(kW=-2),
                                  _with(dH=0), _with(dW=-1), _with(dilH=0), _with(dilW=-1), _with(padH=-1), _with(padW=-1),
                                  _with(H=2, W=2, padH=0, padW=0),          # an output smaller than 1 x 1
                                  _with(H=1, W=9, padH=0, padW=0)])
def test_bad_sizes_are_shape_errors(dims):
    lib = _lib.lib()
    for dt in TYPES:
        assert lib.tdrn_conv2d_strided_workspace_bytes(*dims, dt) == 0
        assert _entries(lib, dims, dt, 1 << 20) == (-2, -2, -2)


UNCOVERED = [
    _with(dH=1, dW=1),                                   # stride 1: section i-c's
    _with(kH=1, kW=1, padH=0, padW=0),                   # k = 1
    _with(kH=5, kW=5, padH=2, padW=2),                   # k = 5
    _with(dilH=2, dilW=2, padH=2, padW=2),               # dilation 2
    _with(padH=3, padW=3),                               # pad 3
    _with(dH=2, dW=1), _with(dH=1, dW=2),                # per-axis stride
    _with(dH=3, dW=3),                                   # stride 3
    _with(padH=1, padW=0),                               # per-axis pad
    _with(kH=3, kW=1),                                   # not square
    _with(N=128, Cin=256, H=256, W=256, Cout=8),         # N H W CiPad = 2^31
    _with(N=128, Cin=8, H=511, W=511, Cout=256),         # N Ho Wo CoPad = 2^31 (Ho = Wo = 256), N H W CiPad below it
    _with(N=128, Cin=8, H=258, W=258, Cout=256, padH=0, padW=0),     # the zero-inserted image alone: N Hd Wd CoPad = 2^31
]


@pytest.mark.parametrize("dims", UNCOVERED)
def test_uncovered_geometry_is_unsupported(dims):
    lib = _lib.lib()
    for dt in TYPES:
        assert lib.tdrn_conv2d_strided_workspace_bytes(*dims, dt) == 0
        assert _entries(lib, dims, dt, 1 << 20) == (-4, -4, -4)


def test_the_size_limits_are_where_the_comments_say():
    d = dict(zip(NAMES, UNCOVERED[-2]))
    Ho = (d["H"] + 2 * d["padH"] - 3) // 2 + 1
    assert Ho == 256 and d["N"] * Ho * ((d["W"] + 2 * d["padW"] - 3) // 2 + 1) * 256 == 2 ** 31
    assert d["N"] * d["H"] * d["W"] * 64 < 2 ** 31
    d = dict(zip(NAMES, UNCOVERED[-1]))
    Ho, Hd = (d["H"] - 3) // 2 + 1, d["H"] - 2
    assert d["N"] * Hd * Hd * 256 == 2 ** 31 and d["N"] * Ho * Ho * 256 < 2 ** 31 and d["N"] * d["H"] * d["W"] * 64 < 2 ** 31


def test_the_two_families_are_disjoint():
    lib = _lib.lib()
    for dt in TYPES:
        # section i-c still refuses stride 2 ...
        assert lib.tdrn_conv2d_workspace_bytes(*GOOD, dt) == 0
        assert _entries(lib, GOOD, dt, 1 << 20, family="tdrn_conv2d") == (-4, -4, -4)
        # ... and serves stride 1, which this family refuses
        s1 = _with(dH=1, dW=1)
        assert lib.tdrn_conv2d_workspace_bytes(*s1, dt) > 0 and lib.tdrn_conv2d_strided_workspace_bytes(*s1, dt) == 0


def test_short_workspace_and_null_pointers():
    lib = _lib.lib()
    p = 256
    for dt in TYPES:
        nb = lib.tdrn_conv2d_strided_workspace_bytes(*GOOD, dt)
        assert _entries(lib, GOOD, dt, nb - 1) == (-3, -3, -3)
        assert lib.tdrn_conv2d_strided_forward(p, p, None, p, *GOOD, dt, None, nb, None) == -3            # no workspace at all
        assert lib.tdrn_conv2d_strided_backward_input(p, p, p, *GOOD, dt, None, nb, None) == -3
        assert lib.tdrn_conv2d_strided_backward_parameters(p, p, p, None, *GOOD, 1.0, dt, None, nb, None) == -3
        # a null tensor pointer is refused first, whatever else is passed: every call below has one
        assert lib.tdrn_conv2d_strided_forward(None, p, None, p, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv2d_strided_forward(p, None, None, p, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv2d_strided_forward(p, p, None, None, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv2d_strided_backward_input(None, p, p, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv2d_strided_backward_input(p, None, p, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv2d_strided_backward_input(p, p, None, *GOOD, dt, p, nb, None) == -1
        assert lib.tdrn_conv2d_strided_backward_parameters(None, p, p, None, *GOOD, 1.0, dt, p, nb, None) == -1
        assert lib.tdrn_conv2d_strided_backward_parameters(p, None, p, None, *GOOD, 1.0, dt, p, nb, None) == -1
        assert lib.tdrn_conv2d_strided_backward_parameters(p, p, None, None, *GOOD, 1.0, dt, p, nb, None) == -1
        # ... also in front of a bad geometry and of a short workspace
        assert lib.tdrn_conv2d_strided_forward(None, p, None, p, *_with(N=0), dt, None, 0, None) == -1
        assert lib.tdrn_conv2d_strided_backward_input(p, p, None, *_with(dH=1, dW=1), dt, None, 0, None) == -1
        # a shape error comes before an uncovered geometry, that before the workspace
        assert lib.tdrn_conv2d_strided_forward(p, p, None, p, *_with(N=0, dH=1, dW=1), dt, None, 0, None) == -2
        assert lib.tdrn_conv2d_strided_forward(p, p, None, p, *_with(dH=1, dW=1), dt, None, 0, None) == -4


def test_module_has_nn_conv2d_parameters():
    m, r = networks.Conv2d(5, 7, 3, padding=1, stride=2), torch.nn.Conv2d(5, 7, 3, 2, 1)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in r.state_dict().items()}
    assert m.stride == (2, 2) and networks.Conv2d(5, 7, 3).stride == (1, 1)
    assert networks.Conv2d(5, 7, 3, stride=2, bias=False).bias is None
    m.load_state_dict(r.state_dict())
    torch.manual_seed(3)
    r.reset_parameters()
    torch.manual_seed(3)
    m.reset_parameters()
    assert torch.equal(m.weight, r.weight) and torch.equal(m.bias, r.bias)
    # stride is the LAST parameter everywhere: the positional calls of before keep their meaning
    import inspect
    for f in (networks.Conv2dFunction.forward, networks.conv2d, networks.Conv2d.__init__):
        assert list(inspect.signature(f).parameters)[-1] == "stride"
        assert inspect.signature(f).parameters["stride"].default == 1


def test_uncovered_strides_raise_and_cpu_tensors_are_rejected():
    x, w, b = torch.zeros(1, 3, 8, 8), torch.zeros(4, 3, 3, 3), torch.zeros(4)
    for stride in (3, (2, 1), (1, 2), 0):
        with pytest.raises(RuntimeError, match="outside what libtdrn_hip covers"):
            networks._conv2d_family(stride)
    assert networks._conv2d_family(1) == networks._conv2d_family((1, 1)) == "tdrn_conv2d"
    assert networks._conv2d_family(2) == networks._conv2d_family((2, 2)) == "tdrn_conv2d_strided"
    for stride in (3, (2, 1)):
        with pytest.raises(RuntimeError, match="outside what libtdrn_hip covers"):
            networks.conv2d(x, w, b, 1, stride=stride)
    with pytest.raises(NotImplementedError):
        networks.conv2d(x, w, b, 1, stride=2)
    with pytest.raises(NotImplementedError):
        networks.Conv2dFunction.apply(x, w, None, 1, 1, "fp32", 2)
    with pytest.raises(NotImplementedError):
        networks.Conv2d(3, 4, 3, padding=1, stride=2)(x)


# ---- the plan, restated ---------------------------------------------------------------------------------------------------------
def _dense(case):
    """a case as the arguments of test_conv_grad_variants.py's dense_*: N, Cin, H, W, Cout, k = 3, stride 2, pad, dil = 1"""
    N, Cin, H, W, Cout, pad = G.CASES[case]
    return N, Cin, H, W, Cout, 3, 2, pad, 1


def geometry(case):
    N, Cin, H, W, Cout, pad = G.CASES[case]
    Ho, Wo, Hd, Wd = dense_geometry(H, W, 3, 2, pad, 1)
    assert (Ho, Wo) == G._out_hw(case) and (Hd, Wd) == (H + 2 * pad - 2, W + 2 * pad - 2)
    return N, Cin, H, W, Cout, pad, Ho, Wo, Hd, Wd


def problem(case, dgrad):
    """the implicit GEMM of the forward (stride 2) or of the input gradient (stride 1, pad' = 2 - pad, over the zero-inserted image)"""
    return dense_problem(*_dense(case), dgrad)


def wgrad_splits(case):
    """conv_wgrad_splits on the strided output -> (splits, per_split, M)"""
    return dense_wgrad_splits(*_dense(case))


def workspace_bytes(case, mode):
    return dense_workspace_bytes(*_dense(case), mode)


@pytest.mark.parametrize("mode", list(ES))
@pytest.mark.parametrize("case", list(G.CASES))
def test_restated_plan_reproduces_the_workspace_query(case, mode):
    assert _lib.lib().tdrn_conv2d_strided_workspace_bytes(*G._dims(case), _lib.DTYPES[mode]) == workspace_bytes(case, mode)


def test_the_zero_inserted_image_has_a_row_pair_per_output_row():
    for case in G.CASES:
        N, Cin, H, W, Cout, pad, Ho, Wo, Hd, Wd = geometry(case)
        assert Hd in (2 * Ho - 1, 2 * Ho) and Wd in (2 * Wo - 1, 2 * Wo), case
    # both parities of both axes, and Hd > H, are among the cases
    par = {(geometry(c)[8] - 2 * geometry(c)[6], geometry(c)[9] - 2 * geometry(c)[7]) for c in G.CASES}
    assert par == {(0, 0), (0, -1), (-1, 0), (-1, -1)}
    assert geometry("pad2_a")[8] > G.CASES["pad2_a"][2] and geometry("pad2_b")[8] > G.CASES["pad2_b"][2]


@pytest.mark.parametrize("mode", list(ES))
def test_each_case_reaches_its_variant(mode):
    es = ES[mode]
    # a 64-pixel wgrad chunk crosses images
    N, Cin, H, W, Cout, pad, Ho, Wo, Hd, Wd = geometry("odd_sizes")
    assert Ho * Wo == 20 and N * Ho * Wo < 64
    # two cin tiles; the bottom pad row is read by no output row
    N, Cin, H, W, Cout, pad, Ho, Wo, Hd, Wd = geometry("even_sizes")
    assert cpad(Cin) // 64 == 2 and 2 * (Ho - 1) - pad + 2 == H - 1
    # 1 x 1 outputs
    assert G._out_hw("one_pixel_a") == (1, 1) and G._out_hw("one_pixel_b") == (1, 1)
    # the extras layer: forward and input gradient run split-K
    assert splitk(problem("extras", False), es) > 1 and splitk(problem("extras", True), es) > 1
    # wgrad splits
    assert wgrad_splits("k_split") == (7, 256, 1600)
    S, per, M = wgrad_splits("k_ragged")
    assert (S, M, M - (S - 1) * per) == (4, 798, 30)
    assert wgrad_splits("one_pixel_a") == (1, 64, 3)
    # the scalar epilogue (o_cs no multiple of 4: Cout in the forward, Cin in the input gradient) and the 16-byte one
    assert G.CASES["odd_wo"][4] % 4 != 0 and G.CASES["odd_sizes"][1] % 4 != 0 and G.CASES["mobilenet_first"][1] % 4 != 0
    assert G.CASES["extras"][4] % 4 == 0 and G.CASES["extras"][1] % 4 == 0 and G.CASES["k_ragged"][4] % 4 == 0
    # the dilate kernel: 16-byte loads where Wo % 4 == 0, dwords elsewhere; a second 16-pixel tile of a row
    vec = {c for c in G.CASES if G._out_hw(c)[1] % 4 == 0}
    assert {"odd_sizes", "pad2_b", "mobilenet_first", "k_split"} <= vec
    assert {"odd_wo", "extras", "k_ragged", "even_sizes", "one_pixel_a"} & vec == set()
    assert G._out_hw("k_split")[1] == 20 and G._out_hw("k_ragged")[1] == 19           # two tiles: 16-byte loads | dwords
    # no case reaches the deep tile
    for case in G.CASES:
        for dgrad in (False, True):
            assert tile(problem(case, dgrad)) != "256x128", (case, dgrad)


def test_split_k_slices():
    assert [splitk(problem("extras", False), ES[m]) for m in ("fp32", "bf16", "fp16")] == [16, 9, 9]
    assert [splitk(problem("extras", True), ES[m]) for m in ("fp32", "bf16", "fp16")] == [16, 16, 16]
