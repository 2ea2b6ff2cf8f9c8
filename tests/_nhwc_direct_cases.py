"""Cases, launch table, inputs, float64 references and the comparison of test_gpu_nhwc_direct.py: the resident conv's direct-conv
kernels (conv3x3_patch / conv3x3_pp behind tdrn_conv2d_nhwc_*) at the variants a training step at batch 32 runs and
test_gpu_nhwc_conv.py does not reach.  No GPU is needed to import this; test_nhwc_direct_ref.py asserts what the construction
relies on.

Launches.  A case is N, Cin, H, W, Cout of a 3x3 / stride 1 / pad 1 / dilation 1 layer with a bias.  Its forward convolves Cin
channels into Cout columns, its input gradient Cout channels (grad_output) into Cin columns.  `launch` restates in plain Python the
host rules that decide what such a launch runs -- conv_n_pad, conv_route, conv3x3_tile_mode, conv_tiles, pp_takes,
launch_conv3x3_patch's item width, persistent_grid, xcd_items and conv3x3_patch's tail split -- and LAUNCHES holds what they give for
every case as literals, so that an edit of a case or of a rule shows.

Inputs.  The batch is N / 3 replicas of a base of three distinct images (x and grad_output alike; one weight, one bias).  The
neighbours of an image always differ from it, so a tile that reads or writes the wrong image shows.  Three images are no whole
number of flat tiles (1200 or 1260 pixels against 256), and in the pp cases the items of a replica (6 or 27) divide no XCD's
item range (50, 25, 38), so there the replicas fall at different places in tiles, XCD ranges and workgroups.  In the two 2-D patch
cases they do not: patch_bn128_32 has 24 (12) items a replica and 24 (12) an XCD, patch_tail_16 36 and 36, so every replica sits
alike in another XCD and its bit-equality compares XCDs, not placements; a tail-split half item is compared with whole items of
other placements by pp_flat's input gradient alone, and with float64 everywhere.  Outputs and input
gradients are the base's, replicated; grad_weight and grad_bias are N / 3 times the base's (the device of the > 2^30-element tests,
DESIGN.md section 14).

Bounds: the project's (tests/_nhwc_harness.py).  Output and grad_input bound16 = c S + u (|ref| + c S) + tiny, grad_weight and
grad_bias c S; u the type's unit roundoff, c = C_ACC, S the op on absolute values.  No element is exempted."""
import collections
import functools

import torch
import torch.nn.functional as F

from _conv_train_harness import C_ACC
from _nhwc_harness import bound16, exact

torch.set_num_threads(min(16, torch.get_num_threads()))      # (float64 references: the GPU hosts' threads oversubscribe)

PERIOD = 3
MODES = ("bf16", "fp16")
#        name                 N   Cin  H   W  Cout
CASES = {"pp_flat":           (90, 256, 20, 20, 512),
         "pp_32":             (99, 256, 16, 32, 448),
         "pp_16":             (33, 256, 48, 48, 256),
         "patch_flat_chunks": (3,  192, 21, 20, 192),
         "patch_bn128_32":    (24, 64,  16, 64, 192),
         "patch_tail_16":     (24, 128, 32, 48, 256)}

# the constants of the rules, where the source states them (test_nhwc_direct_ref.py ties them to the text or to the library)
PATCH_MIN_PIXELS = 400          # conv_route.hip kPatchMinPixels
PP_MIN_ITEMS = 192              # conv3x3_pp.hip pp_takes
BN128_MIN_ITEMS = 160           # conv3x3_patch.hip launch_conv3x3_patch
PATCH_SLOTS = PP_SLOTS = 44     # 8-row pieces of a patch buffer: flat tiles need 2 W + 2 + 256 rows

Launch = collections.namedtuple("Launch", "kernel tiles width items grid xcd per_wg chunks masked")
# kernel  "pp" | "patch" | "igemm"
# tiles   32 | 16 (2-D tiles of 8 x 32 | 16 x 16 pixels) | "flat" (256 consecutive NHW pixels)
# width   couts of an item: 256 (pp), 128 | 64 (patch)
# items, grid
# xcd     per XCD label 0..7: (full, rem, tail): full rounds of the XCD's grid / 8 workgroups, items of its last round, and whether
#         conv3x3_patch cuts those into 2 rem half items (128-cout items only, when the last round is at most half full)
# per_wg  the sorted set of item counts a workgroup of the grid runs (a half item counts as one)
# chunks  64-channel chunks of the launch's input
# masked  Cout < Npad: the last cout item of every tile masks columns


def cdiv(a, b):
    return -(-a // b)


def n_pad(cout):
    return 32 if cout <= 32 else (64 if cout <= 64 else cdiv(cout, 128) * 128)


def problem(case, dgrad):
    """(B, H, W, Cin, Cout, Npad) of the launch: the input gradient is the forward of the mirrored layer over grad_output"""
    N, Cin, H, W, Cout = CASES[case]
    ci, co = (Cout, Cin) if dgrad else (Cin, Cout)
    return N, H, W, ci, co, n_pad(co)


def tile_mode(H, W, slots):
    if W % 32 == 0 and H % 8 == 0:
        return 32
    if W % 16 == 0 and H % 16 == 0:
        return 16
    return "flat" if 2 * W + 2 + 256 <= slots * 8 else None


def m_tiles(B, H, W, tiles):
    return cdiv(B * H * W, 256) if tiles == "flat" else B * (W // tiles) * (H // (256 // tiles))


def launch(case, dgrad):
    B, H, W, Cin, Cout, Npad = problem(case, dgrad)
    kernel, tiles, width = "igemm", None, None
    if H * W >= PATCH_MIN_PIXELS:
        tiles = tile_mode(H, W, PP_SLOTS)
        if Cin >= 256 and Npad % 256 == 0 and tiles and m_tiles(B, H, W, tiles) * (Npad // 256) >= PP_MIN_ITEMS:
            kernel, width = "pp", 256
        else:
            tiles = tile_mode(H, W, PATCH_SLOTS)
            if tiles and Npad % 64 == 0:
                kernel = "patch"
                width = 128 if Npad % 128 == 0 and m_tiles(B, H, W, tiles) * (Npad // 128) >= BN128_MIN_ITEMS else 64
    if kernel == "igemm":
        return Launch("igemm", None, None, None, None, None, None, Cin // 64, Cout < Npad)
    items = m_tiles(B, H, W, tiles) * (Npad // width)
    grid = 256 if items >= 256 else cdiv(items, 8) * 8
    per_xcd, istride = cdiv(items, 8), grid // 8
    xcd, per_wg = [], set()
    for x in range(8):
        avail = max(0, min(per_xcd, items - x * per_xcd))
        full, rem = divmod(avail, istride)
        tail = kernel == "patch" and width == 128 and full > 0 and rem > 0 and 2 * rem <= istride
        xcd.append((full, rem, tail))
        per_wg |= {full + (slot < (2 * rem if tail else rem)) for slot in range(istride)}
    return Launch(kernel, tiles, width, items, grid, tuple(xcd), tuple(sorted(per_wg)), Cin // 64, Cout < Npad)


def _x(*runs):
    """per-XCD triples from (count, triple) runs"""
    return tuple(t for n, t in runs for _ in range(n))


# case: (forward launch, input-gradient launch) -- what each case is in the suite for
LAUNCHES = {
    # tiles straddle images (400 px an image); two cout tiles: n_major
    "pp_flat": (Launch("pp", "flat", 256, 282, 256, _x((7, (1, 4, False)), (1, (0, 30, False))), (0, 1, 2), 4, False),
                # tail split on seven XCDs; the last has 30 items: no full round, no tail
                Launch("patch", "flat", 128, 282, 256, _x((7, (1, 4, True)), (1, (0, 30, False))), (0, 1, 2), 8, False)),
    # Cout 448 < Npad 512 on two cout tiles; the input gradient has an odd chunk count on a grid of 200
    "pp_32": (Launch("pp", 32, 256, 396, 256, _x((7, (1, 18, False)), (1, (1, 14, False))), (1, 2), 4, True),
              Launch("pp", 32, 256, 198, 200, _x((7, (1, 0, False)), (1, (0, 23, False))), (0, 1), 7, False)),
    "pp_16": (Launch("pp", 16, 256, 297, 256, _x((7, (1, 6, False)), (1, (0, 31, False))), (0, 1, 2), 4, False),
              Launch("pp", 16, 256, 297, 256, _x((7, (1, 6, False)), (1, (0, 31, False))), (0, 1, 2), 4, False)),
    # Npad 256: the fourth 64-cout item of every tile is wholly masked; ragged last tile (1260 = 4 x 256 + 236 pixels)
    "patch_flat_chunks": (Launch("patch", "flat", 64, 20, 24, _x((6, (1, 0, False)), (1, (0, 2, False)), (1, (0, 0, False))), (0, 1), 3, True),
                          Launch("patch", "flat", 64, 20, 24, _x((6, (1, 0, False)), (1, (0, 2, False)), (1, (0, 0, False))), (0, 1), 3, True)),
    # 128-cout items with the second item of every tile half masked, one chunk
    "patch_bn128_32": (Launch("patch", 32, 128, 192, 192, _x((8, (1, 0, False))), (1,), 1, True),
                       Launch("patch", 32, 64, 96, 96, _x((8, (1, 0, False))), (1,), 3, False)),
    # tail split on every XCD (8 half items each); the input gradient's 64-cout kernel has none: two whole items in a workgroup
    "patch_tail_16": (Launch("patch", 16, 128, 288, 256, _x((8, (1, 4, True))), (1, 2), 2, False),
                      Launch("patch", 16, 64, 288, 256, _x((8, (1, 4, False))), (1, 2), 4, False)),
}


def dims_of(case):
    N, Cin, H, W, Cout = CASES[case]
    return (N, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 1, 1)


def replicas(case):
    assert CASES[case][0] % PERIOD == 0
    return CASES[case][0] // PERIOD


@functools.lru_cache(maxsize=None)
def base_inputs(case, mode):
    """x (3, Cin, H, W), weight, bias, grad_output (3, Cout, H, W): exact values of the type, scaled as test_gpu_nhwc_conv.py's"""
    N, Cin, H, W, Cout = CASES[case]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(case) * 7 + MODES.index(mode))
    x = exact(torch.randn(PERIOD, Cin, H, W, generator=g), mode)
    w = exact(torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5, mode)
    b = exact(torch.randn(Cout, generator=g), mode)
    go = exact(torch.randn(PERIOD, Cout, H, W, generator=g), mode)
    return x, w, b, go


def batch(base, case):
    """the base repeated N / 3 times along N"""
    return base.repeat(replicas(case), 1, 1, 1)


@functools.lru_cache(maxsize=None)
def reference(case, mode):
    """float64 autograd on the base, on the values and on their absolute values, computed once and never changed:
    ((y, gx, gw, gb), (Sy, Sgx, Sgw, Sgb)); y and gx are the base's (3 images), gw and gb those of the whole batch (N / 3 times the
    base's)"""
    R = replicas(case)
    out = []
    for absolute in (False, True):
        x, w, b, go = (t.double().abs() if absolute else t.double() for t in base_inputs(case, mode))
        x.requires_grad_(True); w.requires_grad_(True); b.requires_grad_(True)
        y = F.conv2d(x, w, b, 1, 1, 1)
        y.backward(go)
        out.append((y.detach(), x.grad, R * w.grad, R * b.grad))
    return tuple(out)


def assert_replicas_within(what, mode, got, ref, S):
    """every element of every replica of got (N, C, H, W), on any device, against the base's float64 reference (3, C, H, W) and
    its absolute-value sum, compared in float64 where got lives -> the worst share of bound16, printed before it is asserted"""
    assert got.shape[0] % PERIOD == 0 and tuple(got.shape[1:]) == tuple(ref.shape[1:]) and ref.shape[0] == PERIOD, what
    fmt = torch.channels_last if got.is_contiguous(memory_format=torch.channels_last) else torch.contiguous_format
    ref, bound = (t.to(got.device).contiguous(memory_format=fmt) for t in (ref, bound16(mode, ref, S)))
    g = got.detach().unflatten(0, (got.shape[0] // PERIOD, PERIOD))
    finite = bool(torch.isfinite(g).all())
    d = (g.double() - ref).abs()
    over = int((~(d <= bound)).sum())
    ratio = float(torch.nan_to_num(d / bound, nan=float("inf")).max())
    print("%s: max|d| %.3e  worst share of the bound %.3e" % (what, float(torch.nan_to_num(d, nan=float("inf")).max()), ratio))
    assert finite, "%s: non-finite values" % what
    assert over == 0, (what, ratio, "%d elements over the bound" % over)
    return ratio


def assert_sum_within(what, mode, got, ref, S):
    """a sum over the whole batch (grad_weight, grad_bias) against c S"""
    g = got.detach().cpu().double()
    assert g.shape == ref.shape, what
    assert torch.isfinite(g).all(), "%s: non-finite values" % what
    d, bound = (g - ref).abs(), C_ACC[mode] * S
    ratio = float((d / bound.clamp_min(1e-300)).max())
    print("%s: max|d| %.3e  worst share of the bound %.3e" % (what, float(d.max()), ratio))
    assert bool((d <= bound).all()), (what, ratio)
    return ratio


def replica_bits_differ(t):
    """a 16-bit tensor (N, C, H, W): how many elements of the replicas 1.. differ from the first period's, bit for bit"""
    bits = t.detach().permute(0, 2, 3, 1).contiguous().view(torch.int16).unflatten(0, (t.shape[0] // PERIOD, PERIOD))
    return int((bits != bits[:1]).sum())
