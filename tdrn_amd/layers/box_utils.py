"""decode / center_size / encode and the loss targets (match, refine_match) on the device (layers/box_utils.py of the reference)."""
from collections import namedtuple

import torch

from .. import _lib


def decode(loc, priors, variances):
    _lib.require_cuda(loc, "loc")
    loc = _lib.aligned16(loc.contiguous().float())
    pri = _lib.aligned16(priors.to(loc.device).contiguous().float())
    out = torch.empty_like(loc)
    _lib.check(_lib.lib().tdrn_decode(_lib.ptr(loc), _lib.ptr(pri), loc.size(0), float(variances[0]),
                                      float(variances[1]), _lib.ptr(out), _lib.current_stream(loc.device)))
    return out


def center_size(boxes):
    _lib.require_cuda(boxes, "boxes")
    boxes = _lib.aligned16(boxes.contiguous().float())
    out = torch.empty_like(boxes)
    _lib.check(_lib.lib().tdrn_center_size(_lib.ptr(boxes), boxes.size(0), _lib.ptr(out),
                                           _lib.current_stream(boxes.device)))
    return out


def encode(matched, priors, variances):
    """layers/box_utils.py:151-172 of the reference: matched (P,4) point form against priors (P,4) center-size."""
    _lib.require_cuda(matched, "matched")
    m = _lib.aligned16(matched.contiguous().float())
    pri = _lib.aligned16(priors.to(m.device).contiguous().float())
    out = torch.empty_like(m)
    _lib.check(_lib.lib().tdrn_encode(_lib.ptr(m), _lib.ptr(pri), m.size(0), float(variances[0]), float(variances[1]),
                                      _lib.ptr(out), _lib.current_stream(m.device)))
    return out


def _to_device(t, device):
    """A host tensor goes up through pinned memory, asynchronously: a blocking host-to-device copy would synchronise."""
    if t.device == device:
        return t
    if t.device.type == "cpu":
        return t.pin_memory().to(device, non_blocking=True)
    return t.to(device)


PackedTargets = namedtuple("PackedTargets", "truths offsets T_total max_truths")
PackedTargets.__doc__ = """A batch's truths already on the device, in tdrn_match's layout (SSDAugmentation.batch makes them): truths
(>= T_total, 5) fp32 rows [x1, y1, x2, y2, label], offsets (B+1) int32 (image b = rows [offsets[b], offsets[b+1])), and two
HOST bounds: T_total >= offsets[B] and max_truths >= every image's count."""


def match_targets(targets, priors, threshold, variances, arm_loc=None):
    """Batched match / refine_match (box_utils.py:81-149) on the device: one call for the whole batch.

    targets: list of B tensors [n_i, 5] (x1, y1, x2, y2, label), as detection_collate gives them, on any device; or a
    PackedTargets, whose truths and offsets are used as they are (no copy, nothing read back).
    priors (P, 4) on the GPU; arm_loc (B, P, 4) or None (None: match against the priors; else refine_match against the
    ARM decode).  Returns (loc_t (B, P, 4) fp32, conf_t (B, P) int32) on the priors' device.  No host synchronisation:
    the per-image counts are tensor sizes, and the packed truths and offsets go up through pinned memory."""
    _lib.require_cuda(priors, "priors")
    dev = priors.device
    if isinstance(targets, PackedTargets):
        B, P = targets.offsets.numel() - 1, priors.size(0)
        truths, off = targets.truths.to(dev).float().contiguous(), targets.offsets.to(dev).int().contiguous()
        total, max_truths = int(targets.T_total), int(targets.max_truths)
        truths = truths if total else None
        return _match(truths, off, total, max_truths, B, priors, threshold, variances, arm_loc)
    B, P = len(targets), priors.size(0)
    counts = [int(t.size(0)) for t in targets]
    offs = [0]
    for n in counts:
        offs.append(offs[-1] + n)
    rows = [t.reshape(-1, 5).float() for t in targets if t.numel()]
    truths = _to_device(torch.cat([r.to(rows[0].device) for r in rows]).contiguous(), dev) if rows else None
    off = _to_device(torch.tensor(offs, dtype=torch.int32), dev)
    max_truths = max(counts) if counts else 0
    return _match(truths, off, offs[-1], max_truths, B, priors, threshold, variances, arm_loc)


def _match(truths, off, total, max_truths, B, priors, threshold, variances, arm_loc):
    dev, P = priors.device, priors.size(0)
    pri = _lib.aligned16(priors.detach().contiguous().float())
    arm = None
    if arm_loc is not None:
        arm = _lib.aligned16(arm_loc.detach().to(dev).reshape(B, P, 4).contiguous().float())
    loc_t = torch.empty(B, P, 4, dtype=torch.float32, device=dev)
    conf_t = torch.empty(B, P, dtype=torch.int32, device=dev)
    L = _lib.lib()
    nb = L.tdrn_match_workspace_bytes(B, P, max_truths)
    if nb == 0:
        raise _lib.TdrnError(-4 if max_truths > 512 else -1, "match: B=%d P=%d, %d truths in one image (at most 512)"
                             % (B, P, max_truths))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.check(L.tdrn_match(_lib.ptr(truths), _lib.ptr(off), total, max_truths, B, _lib.ptr(pri), P, _lib.ptr(arm),
                            float(threshold), float(variances[0]), float(variances[1]), _lib.ptr(loc_t), _lib.ptr(conf_t),
                            _lib.ptr(ws), nb, _lib.current_stream(dev)), "match")
    return loc_t, conf_t


def _match_one(threshold, truths, priors, variances, labels, loc_t, conf_t, idx, arm_loc):
    t = torch.cat([truths.reshape(-1, 4).float(), labels.reshape(-1, 1).float().to(truths.device)], 1)
    lt, ct = match_targets([t], priors, threshold, variances,
                           None if arm_loc is None else arm_loc.reshape(1, -1, 4))
    loc_t[idx] = lt[0]
    conf_t[idx] = ct[0]


def match(threshold, truths, priors, variances, labels, loc_t, conf_t, idx):
    """The reference's per-image match (box_utils.py:81-121): fills loc_t[idx] and conf_t[idx] through the kernel."""
    _match_one(threshold, truths, priors, variances, labels, loc_t, conf_t, idx, None)


def refine_match(threshold, truths, priors, variances, labels, loc_t, conf_t, idx, arm_loc):
    """The reference's per-image refine_match (box_utils.py:123-149); arm_loc (P, 4) of image idx."""
    _match_one(threshold, truths, priors, variances, labels, loc_t, conf_t, idx, arm_loc)
