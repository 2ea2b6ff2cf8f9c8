"""Which conv_igemm.hip variant each case of test_gpu_conv_grad.py reaches, without a GPU.

conv2d's forward and input gradient always run on conv_igemm.hip (conv_train_args: an fp32 result and KOFF_HEAD3X3, which every other
kernel's *_takes refuses).  Inside it four host-side rules pick the code that runs; they are restated here in plain Python:

  conv_n_pad            Npad = 32 | 64 | the next multiple of 128
  launch_dt             tile 256x128 (three LDS stages) when Npad % 128 == 0 and ceil(M / 256) * (Npad / 128) >= 512, otherwise
                        128x128, 128x64 or 128x32 by Npad
  igemm_splitk_choice   K slices of a layer that leaves the chip idle
  make_params           batch_minor: GEMM rows ordered pixel-major over the batch when pad > 0, B > 1 and Ho Wo <= 1600

The input gradient is the forward of the mirrored problem: grad_output (channels padded to 64) as the input, Cin output columns,
pad' = dil (k - 1) - pad.

The restatement is tied to the library in two ways: the rules that size the workspace (conv_n_pad, the channel padding, the split-K
choice) must reproduce tdrn_conv2d_workspace_bytes for every case and type, and the two rules that size nothing (the 256x128
threshold, batch_minor) must still stand in conv_igemm.hip word for word.  If either fails, a threshold moved: pick the shapes of
test_gpu_conv_grad.py's deep_* / two_big_images cases again so that each still reaches the variant this table names.
"""
import os

import pytest

import test_gpu_conv_grad as G
from tdrn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ES = {"fp32": 4, "bf16": 2, "fp16": 2}
ZERO_PAGE = 256


def cdiv(a, b):
    return -(-a // b)


def up(a, b):
    return cdiv(a, b) * b


def n_pad(cout):
    return 32 if cout <= 32 else (64 if cout <= 64 else up(cout, 128))


def cpad(c):
    return up(c, 64)


# ---- conv_dense_plan (api.hip), restated once for the three dense families: each test file passes its cases' k, stride, pad, dil ----
def dense_geometry(H, W, k, stride, pad, dil):
    """(Ho, Wo, Hd, Wd): the output, and the image the input gradient convolves -- grad_output itself at stride 1 (Hd = Ho), its
    zero-inserted image at stride 2"""
    Hd, Wd = H + 2 * pad - dil * (k - 1), W + 2 * pad - dil * (k - 1)
    return (Hd - 1) // stride + 1, (Wd - 1) // stride + 1, Hd, Wd


def dense_problem(N, Cin, H, W, Cout, k, stride, pad, dil, dgrad):
    """the implicit GEMM of the forward or of the input gradient: B, H, W, Cin (padded), Ho, Wo, Cout, Npad, k, pad.  The input
    gradient is the stride-1 conv with pad' = dil (k - 1) - pad over the Hd x Wd image"""
    Ho, Wo, Hd, Wd = dense_geometry(H, W, k, stride, pad, dil)
    if not dgrad:
        return dict(B=N, H=H, W=W, Cin=cpad(Cin), Ho=Ho, Wo=Wo, Cout=Cout, Npad=n_pad(Cout), k=k, pad=pad)
    return dict(B=N, H=Hd, W=Wd, Cin=cpad(Cout), Ho=H, Wo=W, Cout=Cin, Npad=n_pad(Cin), k=k, pad=dil * (k - 1) - pad)


def dense_wgrad_splits(N, Cin, H, W, Cout, k, stride, pad, dil):
    """conv_wgrad_splits on the output pixels -> (splits, per_split, M).  k = 5 runs five workgroups (the kernel rows) per split and
    tile and counts them; k = 1 | 3 count one"""
    Ho, Wo, Hd, Wd = dense_geometry(H, W, k, stride, pad, dil)
    M = N * Ho * Wo
    tiles = (cpad(Cin) // 64) * (cpad(Cout) // 64)
    S = max(1, min(cdiv(512, 5 * tiles if k == 5 else tiles), cdiv(M, 4 * 64)))
    per = up(cdiv(M, S), 64)
    return cdiv(M, per), per, M


def dense_workspace_bytes(N, Cin, H, W, Cout, k, stride, pad, dil, mode):
    """conv_train_layout on conv_dense_plan's two launches (api.hip), from the restated rules"""
    Ho, Wo, Hd, Wd = dense_geometry(H, W, k, stride, pad, dil)
    es = ES[mode]
    f, d = (dense_problem(N, Cin, H, W, Cout, k, stride, pad, dil, dgrad) for dgrad in (False, True))
    o = ZERO_PAGE + up(N * H * W * cpad(Cin) * es, 256) + up(N * Hd * Wd * cpad(Cout) * es, 256)
    S = dense_wgrad_splits(N, Cin, H, W, Cout, k, stride, pad, dil)[0]
    slab_end = o + up(S * k * k * cpad(Cout) * cpad(Cin) * 4, 256) + up(S * cpad(Cout) * 4, 256)
    o += up(max(f["Npad"] * k * k * cpad(Cin), d["Npad"] * k * k * cpad(Cout)) * es, 256)
    o += up(max(f["Npad"], d["Npad"]) * 4, 256)
    o += up(max(N * Ho * Wo * Cout, N * H * W * Cin) * 4, 256)
    partial = 0
    for p in (f, d):
        s = splitk(p, es)
        partial = max(partial, s * p["B"] * p["Ho"] * p["Wo"] * p["Npad"] * 4 if s > 1 else 0)
    return max(o + up(partial, 256), slab_end)


def _dense(case):
    """a stride-1 case as dense_*'s arguments: N, Cin, H, W, Cout, k, stride, pad, dil"""
    N, Cin, H, W, Cout, k, pad, dil = G.CASES[case]
    return N, Cin, H, W, Cout, k, 1, pad, dil


def problem(case, dgrad):
    p = dense_problem(*_dense(case), dgrad)
    assert ((p["H"], p["W"]) if dgrad else (p["Ho"], p["Wo"])) == G._out_hw(case)     # the GPU test's own output size
    return p


def splitk(p, es):
    nk = p["k"] * p["k"] * (p["Cin"] // (128 // es))
    bn = 128 if p["Npad"] % 128 == 0 else (64 if p["Npad"] % 64 == 0 else 32)
    blocks = cdiv(p["B"] * p["Ho"] * p["Wo"], 128) * (p["Npad"] // bn)
    if blocks >= 160 or nk < 8:
        return 1
    s = min(cdiv(384, blocks), nk // 4, 16)
    return 1 if s < 2 else s


def tile(p):
    M = p["B"] * p["Ho"] * p["Wo"]
    if p["Npad"] % 128 == 0 and cdiv(M, 256) * (p["Npad"] // 128) >= 512:
        return "256x128"
    return "128x128" if p["Npad"] % 128 == 0 else ("128x64" if p["Npad"] % 64 == 0 else "128x32")


def batch_minor(p):
    return int(p["pad"] > 0 and p["B"] > 1 and p["Ho"] * p["Wo"] <= 1600 and p["k"] * p["k"] <= 32)


def variant(case, mode, dgrad):
    """(tile, K slices, batch_minor, K steps of one slice-less pass)"""
    p = problem(case, dgrad)
    return tile(p), splitk(p, ES[mode]), batch_minor(p), p["k"] * p["k"] * (p["Cin"] // (128 // ES[mode]))


def workspace_bytes(case, mode):
    return dense_workspace_bytes(*_dense(case), mode)


# case: ((forward tile, dgrad tile), ...) -- what each case is in the suite for
TILES = {
    "deep_fwd": ("256x128", "128x32"),
    "deep_fwd_scalar": ("256x128", "128x32"),
    "deep_dgrad": ("128x32", "256x128"),
    "deep_1x1": ("256x128", "128x32"),
    "deep_dil6": ("256x128", "128x32"),
    "two_big_images": ("128x32", "128x32"),
}


@pytest.mark.parametrize("mode", list(ES))
@pytest.mark.parametrize("case", list(G.CASES))
def test_restated_rules_reproduce_the_workspace_query(case, mode):
    assert _lib.lib().tdrn_conv2d_workspace_bytes(*G._dims(case), _lib.DTYPES[mode]) == workspace_bytes(case, mode)


def test_the_rules_that_size_nothing_stand_in_the_source():
    src = " ".join(open(os.path.join(ROOT, "tdrn_amd", "csrc", "conv_igemm.hip")).read().split())
    for line in ("const long long big_tiles = (long long)cdiv(p.M, 256) * (p.Npad / 128) * phases;",
                 "if (p.Npad % 128 == 0 && big_tiles >= 512) return launch_cfg<DT, 256, 128, 4, 2, 3>(p, phases, s);",
                 "if (p.Npad % 128 == 0) return launch_cfg<DT, 128, 128, 2, 2, 2>(p, phases, s);",
                 "if (p.Npad % 64 == 0) return launch_cfg<DT, 128, 64, 2, 2, 2>(p, phases, s);",
                 "return launch_cfg<DT, 128, 32, 4, 1, 2>(p, phases, s);",
                 "p.batch_minor = (a.pad > 0 && a.phases == 1 && a.B > 1 && a.Ho * a.Wo <= 1600 && a.kh * a.kw <= 32) ? 1 : 0;"):
        assert line in src, "conv_igemm.hip changed this rule: restate it here and pick the deep_* shapes again: " + line


@pytest.mark.parametrize("mode", list(ES))
def test_each_new_case_reaches_its_variant(mode):
    for case, (fwd, dgr) in TILES.items():
        assert variant(case, mode, False)[0] == fwd, (case, "forward")
        assert variant(case, mode, True)[0] == dgr, (case, "dgrad")
    # the deep tile at the threshold exactly (512 workgroups), the last M-tile holding one row, columns past Cout
    for case, dgrad in (("deep_fwd", False), ("deep_fwd_scalar", False), ("deep_1x1", False), ("deep_dil6", False), ("deep_dgrad", True)):
        p = problem(case, dgrad)
        M = p["B"] * p["Ho"] * p["Wo"]
        assert M % 256 == 1 and cdiv(M, 256) * (p["Npad"] // 128) == 512 and p["Cout"] < p["Npad"] == 1024
        assert variant(case, mode, dgrad)[1:3] == (1, 0)              # whole K, batch-major rows
    assert problem("deep_fwd", False)["Cout"] % 4 == 0 and problem("deep_fwd_scalar", False)["Cout"] % 4 != 0       # o_cs: vector | scalar stores
    # fewer K steps than the ring has stages (3)
    assert variant("deep_1x1", mode, False)[3] == (2 if mode == "fp32" else 1)
    assert variant("deep_fwd", mode, False)[3] >= 9
    # conv6's geometry: the taps of a border pixel reach 6 pixels out
    assert G.CASES["deep_dil6"][5:] == (3, 6, 6)


@pytest.mark.parametrize("mode", list(ES))
def test_batch_minor_on_both_sides_of_its_edge(mode):
    for dgrad in (False, True):
        p = problem("two_big_images", dgrad)
        assert p["B"] == 2 and p["Ho"] * p["Wo"] == 1681 and variant("two_big_images", mode, dgrad)[2] == 0
        assert (p["Ho"] * p["Wo"]) % 128 != 0          # a 128-row tile holds the end of image 0 and the start of image 1
        p = problem("k6400_split", dgrad)
        assert p["B"] > 1 and p["Ho"] * p["Wo"] == 1600 and variant("k6400_split", mode, dgrad)[2] == 1
    # no earlier case has several images of more than 1600 pixels
    for case in list(G.CASES)[:12]:
        N, Ho, Wo = G.CASES[case][0], *G._out_hw(case)
        assert N == 1 or Ho * Wo <= 1600, case


def test_split_k_cases():
    # tiny_images: 75 pixels, 256 couts: two workgroups; the K slices are capped by a quarter of the K steps
    assert [variant("tiny_images", m, False)[1] for m in ("fp32", "bf16", "fp16")] == [4, 2, 2]
    assert [variant("tiny_images", m, True)[1] for m in ("fp32", "bf16", "fp16")] == [16, 9, 9]
    # two_big_images: the batch-major rows also go through the split-K reduction
    assert [variant("two_big_images", m, False)[1] for m in ("fp32", "bf16", "fp16")] == [4, 2, 2]
    # (the deep side of every deep_* case runs whole K: test_each_new_case_reaches_its_variant)


def test_the_old_cases_never_reach_the_deep_tile():
    for case in list(G.CASES)[:12]:
        for dgrad in (False, True):
            assert tile(problem(case, dgrad)) in ("128x32", "128x64", "128x128"), case
