"""tests/_train_model_ref.py tied to the oracle on the CPU (no GPU): in eval mode every model's restatement gives
oracle.net_ref.*_forward(phase='train') under the project's rule for these outputs against the oracle (test_gpu_net.py's): atol 1e-3;
behind deformable heads on every prior row but those net_ref.border_rows finds on a sampling discontinuity from the oracle's own
offsets, at most 30 of them.  Two 192 px frames of seed 5, in float32 and float64.

Measured with the five modules this one replaced: worst |d| 1.1e-4 (MobileNet conf, float64); exactly 0 in float32 for every output
with no deformable op in front of it; rows on a discontinuity 0, 24 (temporal ssd4scale_vgg) and 9 (temporal ssd4scale_mobile).
"""
import functools

import numpy as np
import pytest
import torch

import _train_model_harness as H
import _train_model_ref as M
from oracle import net_ref

torch.set_num_threads(min(16, torch.get_num_threads()))
SIZE, MAPS, SEED, B, ATOL = 192, (24, 12, 6, 3), 5, 2, 1e-3
DTYPE = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])


def _check(label, dtype, pairs):
    """pairs: [(name, ours, the oracle's, the rows on a discontinuity or None where no deformable op is in front)]"""
    for name, got, want, allowed in pairs:
        want = torch.as_tensor(want)
        assert tuple(got.shape) == tuple(want.shape) and got.dtype == dtype, name
        on = np.zeros(got.numel() // got.shape[-1], bool) if allowed is None else allowed
        bad, d = H.rows_off(got, want, on, ATOL)
        print("%s %s %s: max|d| %.3e (atol 1e-3), rows on a discontinuity %d, rows over atol elsewhere %d"
              % (label, str(dtype).split(".")[1], name, d, int(on.sum()), bad))
        assert bad == 0, (name, bad)


@DTYPE
@pytest.mark.parametrize("arch", ["vgg", "mobile"])
def test_dual_refinement_nets(arch, dtype):
    model = H.drn_vgg(True, False) if arch == "vgg" else H.drn_mobilenet(False)
    sd, x, taps = H.state(model, 0), H.frames(B, SIZE, SEED), {}
    if arch == "vgg":
        want = net_ref.drn_vggbn_forward(sd, x, 21, True, False, phase="train", taps=taps)
    else:
        want = net_ref.drn_mobilenet_forward(sd, x, 21, False, phase="train", taps=taps)
    allowed = net_ref.border_rows(taps, False)
    got = M.run(model.restatement(), sd, x, dtype, False)
    assert len(got) == 3 and len(want) == 4          # the oracle's second entry is not compared: forward_train hands back None there
    _check("dualrefinedet " + arch, dtype, [("arm_loc", got[0], want[0], None), ("odm_loc", got[1], want[2], allowed),
                                            ("conf", got[2], want[3], allowed)])


@DTYPE
def test_refinedet_with_refine_and_multihead(dtype):
    model = H.refinedet(True, True)
    sd, x = H.state(model, 0), H.frames(B, SIZE, SEED)
    want = net_ref.refinedet_vgg_forward(sd, x, 21, True, True, True, phase="train")
    got = M.run(model.restatement(), sd, x, dtype, False)
    assert len(got) == 3 and want[1] is None
    _check("refinedet", dtype, [("arm_loc", got[0], want[0], None), ("odm_loc", got[1], want[2], None), ("conf", got[2], want[3], None)])


@DTYPE
@pytest.mark.parametrize("arch,deform", [("vgg", False), ("vgg", True), ("mobile", False), ("mobile", True)],
                         ids=["vgg-static", "vgg-temporal", "mobile-static", "mobile-temporal"])
def test_ssd4scale_nets(arch, deform, dtype):
    model = H.ssd4scale(arch, deform)
    sd, x = H.state(model, 0), H.frames(B, SIZE, SEED)
    ref_loc = H.ref_loc(arch, B, SEED, SIZE, MAPS, 1) if deform else None
    want = H.ORACLE[arch](sd, x, 21, "train", deform_on=deform, ref_loc=ref_loc, ret_loc=True, ret_off=True)
    allowed = None
    if deform:
        allowed = net_ref.border_rows({"offset.%d" % s: torch.as_tensor(np.asarray(o)) for s, o in enumerate(want[3])}, False, def_groups=M.G)
    extra = ([torch.as_tensor(r).to(dtype) for r in ref_loc],) if deform else ()
    got = M.run(functools.partial(model.restatement(), ret_loc=True), sd, x, dtype, False, *extra)
    pairs = [("loc", got[0], want[0], allowed), ("conf", got[1], want[1], allowed)]
    if deform:
        assert got[2] == []                              # as the model: the temporal net hands back no loc maps
    else:
        assert len(got[2]) == len(want[2]) == 4
        pairs += [("loc map %d" % s, m, r, None) for s, (m, r) in enumerate(zip(got[2], want[2]))]
    _check("ssd4scale %s deform=%s" % (arch, deform), dtype, pairs)
