"""MultiBoxLoss / RefineMultiBoxLoss on the device (layers/modules/multibox_loss.py, refine_multibox_loss.py of the
reference), forward and backward through libtdrn_hip.so (tdrn_hip.h section ii-b).

The targets (match / refine_match), the hard-negative mining and both losses run as HIP kernels with no host
synchronisation; the semantics, the reference's quirks included, are listed in the header.  fp32 throughout: 16-bit
predictions are upcast, and their gradients come back in the input dtype.  Targets and arm_loc get no gradient (the
reference detaches them, refine_multibox_loss.py:55-57)."""
import torch
import torch.nn as nn

from ... import _lib
from ..box_utils import match_targets


class MultiBoxLossFunction(torch.autograd.Function):
    """(loc, conf) -> [loss_l, loss_c] (one fp32 tensor of 2).  conf None = only_loc (loss_c is not computed).
    loc_t, conf_t (the targets) and sel (0 unused, 1 positive, 2 mined negative) are constants of the graph."""

    @staticmethod
    def forward(ctx, loc, conf, loc_t, conf_t, num_classes, negpos_ratio):
        _lib.require_cuda(loc, "loc_data")
        dev = loc.device
        B, P = loc_t.shape[:2]
        loc32 = _lib.aligned16(loc.detach().reshape(B, P, 4).contiguous().float())
        conf32 = None
        C = 0
        if conf is not None:
            C = int(num_classes)
            conf32 = conf.detach().reshape(B, P, C).contiguous().float()
        L = _lib.lib()
        nb = L.tdrn_multibox_loss_workspace_bytes(B, P, C)
        if nb == 0:
            raise _lib.TdrnError(-4 if C > 1024 else -1, "multibox loss: B=%d P=%d C=%d" % (B, P, C))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        if conf is None:
            loss[1:].zero_()
        sel = torch.empty(B, P, dtype=torch.uint8, device=dev)
        num_pos = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(L.tdrn_multibox_loss_forward(_lib.ptr(loc32), _lib.ptr(conf32), _lib.ptr(loc_t), _lib.ptr(conf_t), B, P, C,
                                                int(negpos_ratio), _lib.ptr(loss), _lib.ptr(sel), _lib.ptr(num_pos),
                                                _lib.ptr(ws), nb, _lib.current_stream(dev)), "multibox loss forward")
        ctx.save_for_backward(loc32, conf32, loc_t, conf_t, sel, num_pos)
        ctx.shapes = (loc.shape, loc.dtype, None if conf is None else (conf.shape, conf.dtype), C)
        ctx.mark_non_differentiable(sel)
        return loss, sel

    @staticmethod
    def backward(ctx, g_loss, g_sel):
        loc32, conf32, loc_t, conf_t, sel, num_pos = ctx.saved_tensors
        (loc_shape, loc_dtype, conf_meta, C) = ctx.shapes
        dev = loc32.device
        B, P = loc_t.shape[:2]
        if g_loss is None:
            g_loss = torch.zeros(2, dtype=torch.float32, device=dev)
        g = g_loss.detach().float().contiguous()
        grad_loc = torch.empty_like(loc32)
        grad_conf = None if conf32 is None else torch.empty_like(conf32)
        _lib.check(_lib.lib().tdrn_multibox_loss_backward(_lib.ptr(loc32), _lib.ptr(conf32), _lib.ptr(loc_t), _lib.ptr(conf_t),
                                                          _lib.ptr(sel), _lib.ptr(num_pos), _lib.ptr(g), B, P, C,
                                                          _lib.ptr(grad_loc), _lib.ptr(grad_conf),
                                                          _lib.current_stream(dev)), "multibox loss backward")
        gl = grad_loc.reshape(loc_shape).to(loc_dtype) if ctx.needs_input_grad[0] else None
        gc = None
        if grad_conf is not None and ctx.needs_input_grad[1]:
            gc = grad_conf.reshape(conf_meta[0]).to(conf_meta[1])
        return gl, gc, None, None, None, None


def multibox_loss(loc, conf, loc_t, conf_t, num_classes, negpos_ratio=3):
    """(loss [2], sel (B, P) uint8) from predictions and targets (match_targets).  conf None: only_loc."""
    return MultiBoxLossFunction.apply(loc, conf, loc_t, conf_t, num_classes, negpos_ratio)


def _check_ratio(neg_pos):
    if int(neg_pos) != neg_pos or neg_pos < 0:
        raise NotImplementedError("neg_pos must be a non-negative integer (the reference drivers use 3)")
    return int(neg_pos)


class RefineMultiBoxLoss(nn.Module):
    """layers/modules/refine_multibox_loss.py: same constructor and forward.  prior_for_matching, bkg_label, neg_mining,
    neg_overlap and encode_target are stored and unused, as in the reference.  N = 0 (no truth in the batch) returns the
    reference's arithmetic, 0/0 = NaN.  An image with no truths is all background and adds nothing (the reference fails
    there)."""

    def __init__(self, num_classes, overlap_thresh, prior_for_matching, bkg_label, neg_mining, neg_pos, neg_overlap,
                 encode_target, device=torch.device('cpu'), only_loc=False, filter_object=0.):
        super().__init__()
        self.device = device
        self.num_classes = num_classes
        self.threshold = overlap_thresh
        self.background_label = bkg_label
        self.encode_target = encode_target
        self.use_prior_for_matching = prior_for_matching
        self.do_neg_mining = neg_mining
        self.negpos_ratio = _check_ratio(neg_pos)
        self.neg_overlap = neg_overlap
        self.variance = [0.1, 0.2]
        self.only_loc = only_loc
        self.filter_object = filter_object
        if filter_object:
            raise NotImplementedError("filter_object != 0 is not supported (no reference driver sets it)")

    def forward(self, odm_data, priors, targets, arm_data=None):
        if self.only_loc:
            loc_data, conf_data = odm_data, None
        else:
            loc_data, conf_data = odm_data
        arm_loc = arm_data[0] if arm_data else None       # arm_data[1] is unused when filter_object == 0; may be None
        loc_t, conf_t = match_targets(targets, priors.to(loc_data.device), self.threshold, self.variance, arm_loc)
        loss, _ = multibox_loss(loc_data, conf_data, loc_t, conf_t, self.num_classes, self.negpos_ratio)
        if self.only_loc:
            return loss[0]
        return loss[0], loss[1]


class MultiBoxLoss(nn.Module):
    """layers/modules/multibox_loss.py: same constructor and forward (match against the priors, loss_l and loss_c / N)."""

    def __init__(self, num_classes, overlap_thresh, prior_for_matching, bkg_label, neg_mining, neg_pos, neg_overlap,
                 encode_target, device='cuda'):
        super().__init__()
        self.device = device
        self.num_classes = num_classes
        self.threshold = overlap_thresh
        self.background_label = bkg_label
        self.encode_target = encode_target
        self.use_prior_for_matching = prior_for_matching
        self.do_neg_mining = neg_mining
        self.negpos_ratio = _check_ratio(neg_pos)
        self.neg_overlap = neg_overlap
        self.variance = [0.1, 0.2]

    def forward(self, predictions, priors, targets):
        loc_data, conf_data = predictions
        loc_t, conf_t = match_targets(targets, priors.to(loc_data.device), self.threshold, self.variance)
        loss, _ = multibox_loss(loc_data, conf_data, loc_t, conf_t, self.num_classes, self.negpos_ratio)
        return loss[0], loss[1]
