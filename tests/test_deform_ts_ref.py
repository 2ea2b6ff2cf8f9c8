"""tests/_deform_ts_harness.py checked on the CPU (no GPU, no launch): the general offset_S equals the one it generalises and
dominates the oracle's grad_offset, every shape of tests/test_gpu_deform_ts_scope.py is inside the op's scope, the fuzz reaches what
it is meant to reach, and the oracle evaluated under the mistakes a kernel could make (a swapped axis pair, a wrong tap split, a lost
column per lane) leaves the bound in enough seeds: a kernel with that mistake could not pass the GPU file."""
import pytest
import torch

from tdrn_amd import _lib

import test_gpu_deform_ts as old
from _deform_grad_ref import grads
from _deform_ts_harness import (MODES, TS_FUZZ_SEEDS, bound, fixed_problems, fuzz_problem, offset_S, offset_S_square, square,
                                ts_fuzz_shape)


def test_general_offset_S_equals_the_square_one():
    """the seven cases x three regimes of test_gpu_deform_ts.py (bf16 inputs; the function does not depend on the type)"""
    for case in old.CASES:
        N, Cin, H, W, Cout, k = case
        for regime in old.REGIMES:
            p = old.problem(case, "bf16", regime)
            a = offset_S_square(p["x"], p["off"], p["w"], p["go"], k, k // 2)
            b = offset_S(square(*case), p["x"], p["off"], p["w"], p["go"])
            assert a.dtype == b.dtype == torch.float64 and torch.equal(a, b), (case, regime)
            assert torch.equal(p["S"]["grad_offset"], a)
            assert float(a.max()) > 0 or H * W == 1         # (one pixel: every accepted sample is inside both clamp bands)


def all_problems(mode):
    for seed in TS_FUZZ_SEEDS:
        g, p = fuzz_problem(seed, mode)
        yield "fuzz %d %s" % (seed, g.name), g, p
    for what, g, p in fixed_problems(mode):
        yield what, g, p


@pytest.mark.parametrize("mode", MODES)
def test_offset_S_dominates_the_oracle(mode):
    """the triangle inequality, elementwise, for every fuzz seed and every fixed case of the GPU file"""
    n = 0
    for what, g, p in all_problems(mode):
        S, ref = p["S"]["grad_offset"], p["ref"]["grad_offset"]
        assert S.shape == ref.shape == (g.N, 2 * g.taps, g.Ho, g.Wo), what
        assert torch.isfinite(S).all() and all(torch.isfinite(r).all() for r in p["ref"].values()), what
        assert bool((S >= ref.abs() * (1 - 1e-12)).all()), what
        # a rejected sample has no offset gradient, on both axes, in the oracle and in S
        rej = (~p["kinds"]["accepted"]).repeat_interleave(2, dim=1)
        assert bool((ref[rej] == 0).all()) and bool((S[rej] == 0).all()), what
        if "far" in p:
            assert bool(rej[p["far"]].all()) and bool((ref[p["far"]] == 0).all()), what
        n += 1
    assert n > len(TS_FUZZ_SEEDS) + 10


def test_every_shape_is_inside_the_scope():
    lib = _lib.lib()
    seen = set()
    for what, g, _ in all_problems("bf16"):
        assert g.Cin % 64 == 0 and 1 <= g.Cout <= 256 and g.Ho >= 1 and g.Wo >= 1, what
        for dt in (_lib.BF16, _lib.F16):
            assert lib.tdrn_deform_conv_ts_workspace_bytes(*g.dims, dt) > 0, what
            assert lib.tdrn_deform_conv_ts_y_bytes(*g.dims, dt) == g.N * g.H * g.W * g.YC * 2, what
        seen.add(g)
    # the row paddings the fixed cases are there for: none (1 x 1, 256 couts) and 56 of 64 columns (1 x 1, one cout)
    assert any(g.taps == 1 and g.Cout == 256 and g.YC == 256 for g in seen) and any(g.taps == 1 and g.Cout == 1 and g.YC == 64 for g in seen)
    assert any(g.YC == 6400 for g in seen)


def test_fuzz_coverage():
    shapes = [ts_fuzz_shape(s) for s in TS_FUZZ_SEEDS]
    gs = [g for g, _ in shapes]
    count = lambda f: sum(1 for g in gs if f(g))
    for nj in (1, 2, 3, 4):
        assert count(lambda g: g.NJ == nj) >= 4, nj
    assert count(lambda g: g.kh != g.kw) >= 8 and count(lambda g: g.sh != g.sw) >= 8 and count(lambda g: g.dh != g.dw) >= 8
    assert count(lambda g: g.M % 4 != 0) >= 8
    assert count(lambda g: g.smaller_than_kernel) >= 2
    assert count(lambda g: (g.Ho, g.Wo) != (g.H, g.W)) >= 12
    for mode in MODES:
        share, generic = [], 0
        for s in TS_FUZZ_SEEDS:
            g, p = fuzz_problem(s, mode)
            k = p["kinds"]
            share.append(float(k["accepted"].double().mean()))
            assert share[-1] >= 0.05, (s, mode, share[-1])
            assert int(k["band"].sum()) >= 1, (s, mode)
            generic += int((k["accepted"] & ~k["band"] & ~k["integer"]).sum()) > 0
        assert sum(1 for v in share if v >= 0.25) >= 12, (mode, share)
        assert generic >= 12, (mode, generic)


def _detected(mode, p, mut):
    """a mutated result leaves the bound at some element of output or grad_offset"""
    for i, name in ((0, "output"), (2, "grad_offset")):
        if mut[i].shape != p["ref"][name].shape:
            return True
        if bool(((mut[i] - p["ref"][name]).abs() > bound(mode, p["S"][name])).any()):
            return True
    return False


def _zero_couts(first):
    def run(g, p):
        w = p["w"].clone()
        w[first:] = 0
        return grads(p["x"], p["off"], w, p["go"], g.stride, g.padding, g.dilation)
    return run


def _geometry(**swap):
    def run(g, p):
        m = g._replace(**{a: getattr(g, b) for a, b in swap.items()})
        if (m.Ho, m.Wo) != (g.Ho, g.Wo):
            return None                                             # another output shape: detected
        return grads(p["x"], p["off"], p["w"], p["go"], m.stride, m.padding, m.dilation)
    return run


def _tap_split(g, p):
    return grads(p["x"], p["off"], p["w"], p["go"], g.stride, g.padding, g.dilation, tap_cols=g.kh)


MUTATIONS = {"sh <-> sw": _geometry(sh="sw", sw="sh"), "dh <-> dw": _geometry(dh="dw", dw="dh"), "ph <-> pw": _geometry(ph="pw", pw="ph"),
             "taps split by kh": _tap_split, "couts >= 192 lost": _zero_couts(192), "couts >= 128 lost": _zero_couts(128)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_the_fuzz_detects(mutation, mode):
    hits = []
    for s in TS_FUZZ_SEEDS:
        g, p = fuzz_problem(s, mode)
        mut = MUTATIONS[mutation](g, p)
        if mut is None or _detected(mode, p, mut):
            hits.append(s)
    print("%s, %s: detected in seeds %r" % (mutation, mode, hits))
    assert len(hits) >= 6, (mutation, mode, hits)


def test_the_unmutated_oracle_is_not_detected():
    """the detector itself: the oracle against itself, and an identity 'mutation', stay inside the bound"""
    for s in TS_FUZZ_SEEDS[:6]:
        g, p = fuzz_problem(s, "fp16")
        assert not _detected("fp16", p, grads(p["x"], p["off"], p["w"], p["go"], g.stride, g.padding, g.dilation, tap_cols=g.kw))
