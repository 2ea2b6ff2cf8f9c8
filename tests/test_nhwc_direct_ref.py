"""What test_gpu_nhwc_direct.py relies on, without a GPU: the plain-Python restatement of the launch rules gives the literal table of
tests/_nhwc_direct_cases.py, agrees with the library where a query exists (tdrn_conv2d_nhwc_route) and with the source text where
none does, the table keeps every variant the cases are in the suite for, and the comparison fails a result with a moved element, a
swapped image, an unmasked cout store or an unwritten tile.  If a rule moved, pick the cases again so that each still reaches the
variant its row of LAUNCHES names."""
import os

import pytest
import torch
import torch.nn.functional as F

import _nhwc_direct_cases as D
from _nhwc_harness import TYPES, bound16
from tdrn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = [(case, dgrad) for case in D.CASES for dgrad in (0, 1)]
ALL = [D.LAUNCHES[case][dgrad] for case, dgrad in BOTH]


@pytest.mark.parametrize("case", list(D.CASES))
def test_restatement_gives_the_table(case):
    assert (D.launch(case, 0), D.launch(case, 1)) == D.LAUNCHES[case]
    assert D.CASES[case][0] % D.PERIOD == 0
    for l in D.LAUNCHES[case]:
        # the table against itself: the per-XCD rounds hold every item
        assert sum(full * (l.grid // 8) + rem for full, rem, _ in l.xcd) == l.items


@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("case", list(D.CASES))
def test_library_routes_as_the_table_says(case, mode):
    lib, dt = _lib.lib(), _lib.DTYPES[mode]
    for dgrad in (0, 1):
        assert lib.tdrn_conv2d_nhwc_route(*D.dims_of(case), dt, 0, dgrad).decode() == D.LAUNCHES[case][dgrad].kernel, (case, dgrad)
        assert lib.tdrn_conv2d_nhwc_route(*D.dims_of(case), dt, _lib.CONV_NHWC_IGEMM_ONLY, dgrad).decode() == "igemm"
    assert lib.tdrn_conv2d_nhwc_workspace_bytes(*D.dims_of(case), dt, 0) > 0


def test_the_rules_no_query_exposes_stand_in_the_source():
    def src(name):
        return " ".join(open(os.path.join(ROOT, "tdrn_amd", "csrc", name)).read().split())
    for name, line, const in (
            ("conv_route.hip", "constexpr int kPatchMinPixels = 400;", D.PATCH_MIN_PIXELS),
            ("conv_route.hip", "} else if (!split && a.H * a.W >= kPatchMinPixels) {", None),
            ("conv3x3_pp.hip", "return p.items >= 192;", D.PP_MIN_ITEMS),
            ("conv3x3_pp.hip", "if (a.Cin < 256 || a.Cin % 64 || a.Npad % 256) return false;", None),
            ("conv3x3_pp.hip", "constexpr int kPPSlots = 44;", D.PP_SLOTS),
            ("conv3x3_patch.hip", "if (BN == 128 && p.m_tiles * (a.Npad / 128) < 160) BN = 64;", D.BN128_MIN_ITEMS),
            ("conv3x3_patch.hip", "if (full > 0 && rem > 0 && 2 * rem <= istride) {", None),
            ("conv3x3_patch.hip", "constexpr bool TAILOK = BN == 128 && sizeof(DT) == 2 && !FUSE;", None),
            ("conv3x3_patch.hip", "#define TDRN_PATCH_RING 3", None),
            ("conv3x3_patch.hip", "constexpr int kPatchSlots = kRing == 4 ? 43 : 44;", D.PATCH_SLOTS),
            ("kernels.h", "inline int persistent_grid(int items) { return items >= 256 ? 256 : ((items + 7) / 8) * 8; }", None),
            ("mfma_prims.h", "r.per_xcd = (items + 7) >> 3;", None)):
        assert line in src(name), "%s changed this rule: restate it in _nhwc_direct_cases.py and pick the cases again: %s" % (name, line)
        assert const is None or str(const) in line


def test_the_table_keeps_every_variant():
    by = lambda **kw: [l for l in ALL if all(getattr(l, k) == v for k, v in kw.items())]
    # all six (kernel, tile mode) pairs
    assert {(l.kernel, l.tiles) for l in ALL} == {(k, t) for k in ("pp", "patch") for t in ("flat", 32, 16)}
    # both patch item widths in every tile mode
    assert {(l.tiles, l.width) for l in by(kernel="patch")} == {(t, w) for t in ("flat", 32, 16) for w in (64, 128)}
    # a tail split in flat and in 2-D mode, and an XCD without one in a launch that has one
    tails = [l for l in by(kernel="patch", width=128) if any(t for _, _, t in l.xcd)]
    assert {l.tiles == "flat" for l in tails} == {True, False}
    assert any(not all(t for _, _, t in l.xcd) for l in tails)
    assert all(2 * rem <= l.grid // 8 for l in tails for _, rem, t in l.xcd if t)
    # no 64-cout launch has a tail, one of them runs two whole items in a workgroup
    assert not any(t for l in by(kernel="patch", width=64) for _, _, t in l.xcd) and any(2 in l.per_wg for l in by(kernel="patch", width=64))
    # pp: more items than workgroups (the item-to-item path), two cout tiles, an odd chunk count, a grid below 256
    pp = by(kernel="pp")
    assert any(l.items > 256 and 2 in l.per_wg for l in pp) and any(l.chunks % 2 for l in pp) and any(l.grid < 256 for l in pp)
    two_tiles = [(case, dgrad) for case, dgrad in BOTH if D.LAUNCHES[case][dgrad].kernel == "pp" and D.problem(case, dgrad)[5] // 256 > 1]
    assert two_tiles and any(D.LAUNCHES[c][d].tiles == "flat" for c, d in two_tiles)
    # a workgroup with no item at all
    assert any(0 in l.per_wg for l in pp) and any(0 in l.per_wg for l in by(kernel="patch"))
    # Cout < Npad on pp, on 128-cout patch items (the last item half masked) and on 64-cout patch items (wholly masked)
    assert any(l.masked for l in pp)
    masked = {l.width: D.problem(case, dgrad) for case, dgrad in BOTH for l in [D.LAUNCHES[case][dgrad]] if l.kernel == "patch" and l.masked}
    assert masked[128][5] - masked[128][4] == 64 and masked[64][5] - masked[64][4] == 64
    # flat tiles straddle an image boundary
    for case, dgrad in BOTH:
        if D.LAUNCHES[case][dgrad].tiles == "flat":
            N, _, H, W, _ = D.CASES[case]
            assert N > 1 and (H * W) % 256 != 0, case
    assert any((D.CASES[c][0] * D.CASES[c][2] * D.CASES[c][3]) % 256 for c, d in BOTH if D.LAUNCHES[c][d].tiles == "flat")     # a ragged last tile
    # more than one channel chunk and exactly one
    assert {l.chunks for l in by(kernel="patch")} >= {1, 2, 3}


FAULT_CASE = "patch_flat_chunks"


def _float32_result(mode):
    """the float32 conv of the batch, rounded once to the type: (N, Cout, H, W) in channels_last, as a kernel leaves it"""
    x, w, b, _ = D.base_inputs(FAULT_CASE, mode)
    y = F.conv2d(D.batch(x, FAULT_CASE), w, b, 1, 1, 1)
    return y.to(TYPES[mode]).contiguous(memory_format=torch.channels_last)


def _pixels(t):
    """the NHWC memory of a channels_last tensor as [pixel][channel]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("mode", D.MODES)
def test_the_comparison_passes_the_float32_conv(mode):
    ref, S = D.reference(FAULT_CASE, mode)
    share = D.assert_replicas_within("float32 conv, %s" % mode, mode, _float32_result(mode), ref[0], S[0])
    assert 0.0 < share <= 1.0
    assert D.replica_bits_differ(_float32_result(mode).repeat(2, 1, 1, 1)) == 0


@pytest.mark.parametrize("fault", ["moved_element", "swapped_images", "unmasked_store", "unwritten_tile"])
@pytest.mark.parametrize("mode", D.MODES)
def test_the_comparison_fails_a_fault(mode, fault):
    N, Cin, H, W, Cout = D.CASES[FAULT_CASE]
    ref, S = D.reference(FAULT_CASE, mode)
    got = _float32_result(mode)
    px = _pixels(got)
    assert px.data_ptr() == got.data_ptr()                      # a view of the same memory
    if fault == "moved_element":                                # one element of the last replica, by twice its bound
        n, c, h, w = N - 1, Cout - 1, H - 1, W - 1
        bound = bound16(mode, ref[0], S[0])[n % D.PERIOD, c, h, w]
        got[n, c, h, w] = float(ref[0][n % D.PERIOD, c, h, w] + 2 * bound)
        assert abs(float(got[n, c, h, w]) - float(ref[0][n % D.PERIOD, c, h, w])) > float(bound)       # (after its rounding to the type)
    elif fault == "swapped_images":
        got[[0, 1]] = got[[1, 0]]
    elif fault == "unmasked_store":
        # the fourth 64-cout item of a tile computes the padded couts [192, 256) (zero weight rows, zero bias: 0.0) and, without the
        # `< Cout` mask, stores them behind pixel p's 192 channels: onto the channels [0, 64) of pixel p + 1
        x, w, b, _ = D.base_inputs(FAULT_CASE, mode)
        wp, bp = torch.zeros(256, Cin, 3, 3), torch.zeros(256)
        wp[:Cout], bp[:Cout] = w, b
        padded = _pixels(F.conv2d(D.batch(x, FAULT_CASE), wp, bp, 1, 1, 1).to(TYPES[mode]).contiguous(memory_format=torch.channels_last))
        p = 300
        px[p + 1, 0:64] = padded[p, Cout:256]
    elif fault == "unwritten_tile":                             # flat tile 1 left at the prefill
        px[256:512] = float("nan")
    with pytest.raises(AssertionError):
        D.assert_replicas_within("%s, %s" % (fault, mode), mode, got, ref[0], S[0])
    if fault == "moved_element":
        assert D.replica_bits_differ(torch.cat([_float32_result(mode), got])) == 1
