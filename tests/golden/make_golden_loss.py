"""Generate tests/golden/loss_*.npz by running the REFERENCE's own match / refine_match / MultiBoxLoss /
RefineMultiBoxLoss on CPU (build container only).

    python tests/golden/make_golden_loss.py            # writes the fixtures next to this file

The reference is imported through ref_shim, as make_golden.py does; nothing of it is copied.  Inputs are regenerated from
seeds (tests/_loss_ref.case_inputs), priors are the committed priorbox_*.npz (the reference's PriorBox output).  Stored:
conf_t, loc_t, sel, the losses and the nonzero rows of the gradients (row index + values).

sel comes from the reference's outputs alone: positives are conf_t > 0, and a row is in pos u neg exactly when its conf
gradient row is nonzero (softmax - onehot never vanishes for finite logits).

Generation asserts that the fixtures do not hinge on rounding: no IoU lies within 1e-6 of the threshold, and the mining
scores (the reference's own log_sum_exp) leave a gap of at least 1e-5 at every image's num_neg boundary, so the selected
set does not depend on summation order.  arm_loc does not require grad: with device='cpu' the reference's `.to(device)`
(refine_multibox_loss.py:55-57) would not detach the targets and a gradient would flow into arm_loc through encode.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import ref_shim  # noqa: E402
import _loss_ref as R  # noqa: E402

THRESH, VAR, NEGPOS = 0.5, (0.1, 0.2), 3


def run_case(name, bu, MultiBoxLoss, RefineMultiBoxLoss):
    import torch
    cfg, B, C, refine, only_loc, counts, seed = R.CASES[name]
    priors_np = R.priors_of(cfg, HERE)
    P = priors_np.shape[0]
    loc_np, conf_np, arm_np, targets_np = R.case_inputs(name, P)
    priors = torch.from_numpy(priors_np)
    targets = [torch.from_numpy(t) for t in targets_np]
    arm = None if arm_np is None else torch.from_numpy(arm_np)        # requires_grad False (see the module docstring)

    # the reference's own matching, per image, for conf_t / loc_t and for the margin checks
    loc_t = torch.Tensor(B, P, 4)
    conf_t = torch.LongTensor(B, P)
    for b in range(B):
        truths, labels = targets[b][:, :-1], targets[b][:, -1]
        if refine:
            bu.refine_match(THRESH, truths, priors, list(VAR), labels, loc_t, conf_t, b, arm[b])
            boxes = bu.decode(arm[b], priors, list(VAR))
        else:
            bu.match(THRESH, truths, priors, list(VAR), labels, loc_t, conf_t, b)
            boxes = bu.point_form(priors)
        ov = bu.jaccard(truths, boxes)
        assert float((ov - THRESH).abs().min()) > 1e-6, (name, b, "an IoU sits on the threshold")
        if b == B - 1:
            assert float(ov[-1].max()) == 0.0, (name, "the tiny truth overlaps a prior")
        if b == 0:
            best_prior = ov.max(1)[1]
            assert best_prior[0] == best_prior[-1], (name, "the duplicated truth has another best prior")

    loc = torch.from_numpy(loc_np).requires_grad_(True)
    if only_loc:
        crit = RefineMultiBoxLoss(C, THRESH, True, 0, True, NEGPOS, 0.5, False, device=torch.device("cpu"), only_loc=True)
        loss_l = crit(loc, priors, targets)
        loss_c = None
        loss_l.backward()
    else:
        conf = torch.from_numpy(conf_np).requires_grad_(True)
        if refine:
            crit = RefineMultiBoxLoss(C, THRESH, True, 0, True, NEGPOS, 0.5, False, device=torch.device("cpu"))
            loss_l, loss_c = crit((loc, conf), priors, targets, arm_data=(arm, None))
        else:
            crit = MultiBoxLoss(C, THRESH, True, 0, True, NEGPOS, 0.5, False, device="cpu")
            loss_l, loss_c = crit((loc, conf), priors, targets)
        (loss_l + loss_c).backward()

    ct = conf_t.numpy()
    pos = ct > 0
    sel = pos.astype(np.uint8)
    out = dict(conf_t=ct.astype(np.uint8), loc_t=loc_t.numpy().astype(np.float32),
               loss_l=np.float32(loss_l.item()))
    gl = loc.grad.numpy().reshape(B * P, 4)
    rl = np.nonzero(np.abs(gl).sum(1))[0]
    assert set(rl) <= set(np.nonzero(pos.reshape(-1))[0])
    out.update(gloc_rows=rl.astype(np.int32), gloc=gl[rl])
    if not only_loc:
        gc = conf.grad.numpy().reshape(B * P, C)
        rc = np.nonzero(np.abs(gc).sum(1))[0]
        used = np.zeros(B * P, bool)
        used[rc] = True
        used = used.reshape(B, P)
        assert (used | ~pos).all(), "a positive row without a conf gradient"
        sel[used & ~pos] = 2
        out.update(loss_c=np.float32(loss_c.item()), gconf_rows=rc.astype(np.int32), gconf=gc[rc])
        # the selected set must not depend on rounding: a gap at every num_neg boundary (the reference's log_sum_exp)
        x = torch.from_numpy(conf_np).reshape(-1, C)
        s = (bu.log_sum_exp(x) - x.gather(1, conf_t.reshape(-1, 1))).reshape(B, P).numpy()
        s[pos] = 0
        for b in range(B):
            k = min(NEGPOS * int(pos[b].sum()), P - 1)
            if k:
                v = np.sort(s[b])[::-1]
                assert v[k - 1] - v[k] > 1e-5, (name, b, "a score tie straddles num_neg", v[k - 1] - v[k])
    out["sel"] = sel
    np.savez_compressed(os.path.join(HERE, "loss_%s.npz" % name), **out)
    print("loss_%s: P=%d B=%d C=%d num_pos=%s loss_l=%.6f loss_c=%s" % (
        name, P, B, C, pos.sum(1).tolist(), out["loss_l"], out.get("loss_c")))


def main():
    import torch
    ref_shim.install()
    torch.set_num_threads(8)
    import layers.box_utils as bu
    from layers.modules.multibox_loss import MultiBoxLoss
    from layers.modules.refine_multibox_loss import RefineMultiBoxLoss
    for name in R.CASES:
        run_case(name, bu, MultiBoxLoss, RefineMultiBoxLoss)


if __name__ == "__main__":
    main()
