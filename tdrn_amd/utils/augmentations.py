"""SSDAugmentation and pairSSDAugmentation on the device (utils/augmentations.py:618-689 of the reference) through
libtdrn_hip.so (tdrn_hip.h sections ii-c and ii-d).

Raw uint8 BGR frames go in; out come the network input (B, 3, S, S) fp32 and the packed truths that MultiBoxLoss /
RefineMultiBoxLoss consume (PackedTargets), with no host synchronisation in between.  The semantics are the reference's,
quirks included; the deviations (bounded crop rounds, no crop for an image without truths, the Philox draw source) are
listed in the header.  A pair is the single chain with a second frame under the same decisions: PairSSDAugmentation adds
that frame's tensors to what SSDAugmentation packs and decodes."""
import ctypes as C
import itertools

import numpy as np
import torch

from .. import _lib
from ..layers.box_utils import PackedTargets, _to_device

PARAMS_BYTES = C.sizeof(_lib.AugmentParams)
PAIR_PARAMS_BYTES = C.sizeof(_lib.AugmentPairParams)
PAIR_FIELDS = ("shift_x", "shift_y", "trans_x", "trans_y", "attempts")


def _host_bytes(struct_array):
    return torch.frombuffer(bytearray(struct_array), dtype=torch.uint8)


def _records(params, struct):
    raw = params.detach().cpu().contiguous().numpy().tobytes()
    n = C.sizeof(struct)
    return [struct.from_buffer_copy(raw[b * n:(b + 1) * n]) for b in range(len(raw) // n)]


def _base_dict(p):
    d = {k: getattr(p, k) for k, _ in p._fields_}
    d["perm"] = tuple(p.perm)
    d["crop"] = (p.crop_x0, p.crop_y0, p.crop_x1, p.crop_y1)
    return d


def params_to_dicts(params):
    """Decode a (B, PARAMS_BYTES) uint8 tensor of tdrn_augment_params records (synchronises when it is on the device)."""
    return [_base_dict(p) for p in _records(params, _lib.AugmentParams)]


def pair_params_to_dicts(params):
    """Decode a (B, PAIR_PARAMS_BYTES) uint8 tensor of tdrn_augment_pair_params records (synchronises when it is on the
    device): the embedded record's fields as params_to_dicts gives them, plus shift_x, shift_y, trans_x, trans_y, attempts."""
    return [dict(_base_dict(q.base), **{k: getattr(q, k) for k in PAIR_FIELDS}) for q in _records(params, _lib.AugmentPairParams)]


def _image_table(images, dev, what):
    tab = (_lib.AugmentImage * len(images))()
    for b, im in enumerate(images):
        _lib.require_cuda(im, "%s[%d]" % (what, b))
        if im.dtype != torch.uint8 or im.dim() != 3 or im.size(2) != 3 or not im.is_contiguous():
            raise ValueError("augment: %s[%d] must be a contiguous uint8 (H, W, 3) tensor" % (what, b))
        tab[b].data, tab[b].h, tab[b].w = im.data_ptr(), im.size(0), im.size(1)
    return _to_device(_host_bytes(tab), dev)


def _frame(img):
    img = torch.as_tensor(img)
    return (img if img.is_cuda else img.to("cuda")).to(torch.uint8).contiguous()


def _truth_rows(boxes, labels):
    b = torch.as_tensor(boxes, dtype=torch.float64).reshape(-1, 4)
    return torch.cat([b, torch.as_tensor(labels, dtype=torch.float64).reshape(-1, 1).to(b.device)], 1)


def _truth_counts(hw, targets):
    if len(hw) == 0 or len(targets) != len(hw):
        raise ValueError("augment: %d images and %d targets" % (len(hw), len(targets)))
    return [int(t.reshape(-1, 5).size(0)) for t in targets]


def _pack_rows(targets, device):
    rows = [t.reshape(-1, 5).to(torch.float64) for t in targets if t.numel()]
    return _to_device(torch.cat([r.to(rows[0].device) for r in rows]).contiguous(), device) if rows else None


def _pack_batch(hw, counts, device):
    """-> (hw (B, 2) int32 and the truth offsets (B+1) int32 on the device, T_total, max_truths)"""
    offs = np.zeros(len(counts) + 1, np.int32)
    offs[1:] = np.cumsum(counts)
    T, Tmax = int(offs[-1]), max(counts)
    if Tmax > _lib.AUGMENT_MAX_TRUTHS:
        raise _lib.TdrnError(-4, "augment: %d truths in one image (at most %d)" % (Tmax, _lib.AUGMENT_MAX_TRUTHS))
    off = _to_device(torch.from_numpy(offs), device)
    hw_t = _to_device(torch.tensor([[int(h), int(w)] for h, w in hw], dtype=torch.int32), device)
    return hw_t, off, T, Tmax


def _draw_source(B, sample_ids, tape, device):
    """-> (ids, tape, tape_off) on the device: Philox sample ids, or the recorded draws and their offsets; the others None"""
    if tape is not None:
        lens = np.zeros(B + 1, np.int32)
        lens[1:] = np.cumsum([len(t) for t in tape])
        draws = np.concatenate([np.asarray(t, np.float64) for t in tape] + [np.zeros(1)])
        return None, _to_device(torch.from_numpy(draws), device), _to_device(torch.from_numpy(lens), device)
    if sample_ids is None:
        raise ValueError("augment: sample_ids (with seed) or a tape is needed")
    ids = torch.as_tensor(sample_ids, dtype=torch.int64).reshape(-1)
    if ids.numel() != B:
        raise ValueError("augment: %d sample ids for %d images" % (ids.numel(), B))
    return _to_device(ids.contiguous(), device), None, None


def _sample_outputs(B, T, Tmax, nbytes, frames, device):
    """-> (records (B, nbytes) uint8, one PackedTargets per frame behind one offset tensor)"""
    params = torch.empty(B, nbytes, dtype=torch.uint8, device=device)
    rows = [torch.empty(max(T, 1), 5, dtype=torch.float32, device=device) for _ in range(frames)]
    out_off = torch.empty(B + 1, dtype=torch.int32, device=device)
    return params, [PackedTargets(r, out_off, T, Tmax) for r in rows]


class _DeviceAugmentation(object):
    """The settings that the single chain and the pair chain share."""

    def __init__(self, size=300, mean=(104, 117, 123), seed=0):
        self.size = int(size)
        self.mean = mean
        self.seed = int(seed)
        self._mean = (C.c_float * 3)(*[float(m) for m in mean])
        self._calls = itertools.count()

    def _seed(self, seed):
        return (self.seed if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF

    def _out(self, out, B, dev):
        return torch.empty(B, 3, self.size, self.size, dtype=torch.float32, device=dev) if out is None else out


class SSDAugmentation(_DeviceAugmentation):
    """The reference's SSDAugmentation(size, mean), batched on the GPU.

    batch(images, targets, sample_ids, seed) is the fast path: images is a list of B uint8 (H, W, 3) BGR tensors on the
    device, targets a list of B (n, 5) tensors of fractions [x1, y1, x2, y2, label] (as detection_collate yields them, on any
    device).  A sample's result depends on (seed, sample id) alone.  It returns (x (B, 3, S, S) fp32, PackedTargets); x is in
    RGB order (VOCDetection.pull_item swaps after the transform) unless to_rgb=False.

    __call__(img, boxes, labels) is the one-image convenience with the reference's signature: it returns device tensors
    (image (S, S, 3) fp32 BGR, boxes (k, 4), labels (k,)) and, unlike batch, synchronises to learn k."""

    def sample(self, hw, targets, device, sample_ids=None, seed=None, tape=None):
        """The decisions and the moved boxes: (params (B, PARAMS_BYTES) uint8, PackedTargets).  hw: B (h, w) pairs (host).
        Exactly one source: sample_ids (+ seed) for Philox, or tape (B host arrays of the reference's draws)."""
        counts = _truth_counts(hw, targets)
        truths = _pack_rows(targets, device)
        hw_t, off, T, Tmax = _pack_batch(hw, counts, device)
        ids, tp, tp_off = _draw_source(len(hw), sample_ids, tape, device)
        params, (packed,) = _sample_outputs(len(hw), T, Tmax, PARAMS_BYTES, 1, device)
        _lib.check(_lib.lib().tdrn_augment_sample(_lib.ptr(hw_t), _lib.ptr(truths), _lib.ptr(off), T, Tmax, len(hw),
                                                  self._seed(seed), _lib.ptr(ids), _lib.ptr(tp), _lib.ptr(tp_off),
                                                  _lib.ptr(params), _lib.ptr(packed.truths), _lib.ptr(packed.offsets),
                                                  _lib.current_stream(device)), "augment sample")
        return params, packed

    def apply(self, images, params, to_rgb=True, out=None):
        """The pixels: (B, 3, S, S) fp32 from the frames and their parameter records."""
        B = len(images)
        dev = images[0].device
        tab = _image_table(images, dev, "images")
        out = self._out(out, B, dev)
        _lib.check(_lib.lib().tdrn_augment_apply(_lib.ptr(tab), _lib.ptr(params), B, self._mean, self.size, 1 if to_rgb else 0,
                                                 _lib.ptr(out), _lib.current_stream(dev)), "augment apply")
        return out

    def batch(self, images, targets, sample_ids=None, seed=None, tape=None, to_rgb=True, return_params=False):
        dev = images[0].device
        _lib.require_cuda(images[0], "images")
        params, packed = self.sample([tuple(im.shape[:2]) for im in images], targets, dev, sample_ids, seed, tape)
        x = self.apply(images, params, to_rgb)
        return (x, packed, params) if return_params else (x, packed)

    def __call__(self, img, boxes, labels):
        x, packed = self.batch([_frame(img)], [_truth_rows(boxes, labels)], [next(self._calls)], to_rgb=False)
        k = int(packed.offsets[1])
        rows = packed.truths[:k]
        return x[0].permute(1, 2, 0), rows[:, :4], rows[:, 4]


class PairSSDAugmentation(_DeviceAugmentation):
    """The reference's pairSSDAugmentation(size, mean) together with VOCDetection.pull_translational_item's translated second
    frame (tdrn_hip.h section ii-d), batched on the GPU: what train_trn.py's VIDDETtrans loader and pair_collate hand to
    static_net(images_ori) and net(images_trans).

    batch(images, targets, sample_ids, seed) takes what SSDAugmentation.batch takes and returns (x_ori, x_trans, packed_ori,
    packed_trans) in pair_collate's order: two (B, 3, S, S) fp32 inputs and two PackedTargets that share one offset tensor.
    With images_t / targets_t the caller supplies the second frames and their truths (the same sizes and counts) and no
    translation is drawn; without them the second frame is the first, translated by at most max_trans_ratio of its size.
    A sample's result depends on (seed, sample id) alone.

    __call__(img_pair, boxes_pair, labels_pair) is the one-pair convenience with the reference's signature: two frames in
    (a None second frame is translated here), device tensors out ([img, img_t] (S, S, 3) fp32 BGR, [boxes, boxes_t],
    [labels, labels_t]); unlike batch it synchronises to learn the kept count."""

    def __init__(self, size=300, mean=(104, 117, 123), seed=0, max_trans_ratio=0.1):
        super(PairSSDAugmentation, self).__init__(size, mean, seed)
        self.max_trans_ratio = float(max_trans_ratio)
        if not 0.0 <= self.max_trans_ratio < 1.0:
            raise ValueError("augment: max_trans_ratio %r is outside [0, 1)" % (max_trans_ratio,))

    def sample(self, hw, targets, device, sample_ids=None, seed=None, tape=None, targets_t=None):
        """The decisions and both frames' moved boxes: (params (B, PAIR_PARAMS_BYTES) uint8, PackedTargets of frame 0,
        PackedTargets of frame 1).  Arguments as SSDAugmentation.sample; targets_t: frame 1's truths, or None to translate."""
        counts = _truth_counts(hw, targets)
        if targets_t is not None:
            counts_t = [int(t.reshape(-1, 5).size(0)) for t in targets_t]
            if counts_t != counts:
                raise ValueError("augment: the second frames' truth counts %r differ from the first's %r" % (counts_t, counts))
        truths = _pack_rows(targets, device)
        truths_t = _pack_rows(targets_t, device) if targets_t is not None else None
        hw_t, off, T, Tmax = _pack_batch(hw, counts, device)
        ids, tp, tp_off = _draw_source(len(hw), sample_ids, tape, device)
        params, (packed, packed_t) = _sample_outputs(len(hw), T, Tmax, PAIR_PARAMS_BYTES, 2, device)
        _lib.check(_lib.lib().tdrn_augment_pair_sample(_lib.ptr(hw_t), _lib.ptr(truths), _lib.ptr(truths_t), _lib.ptr(off), T, Tmax,
                                                       len(hw), self.max_trans_ratio, self._seed(seed), _lib.ptr(ids),
                                                       _lib.ptr(tp), _lib.ptr(tp_off), _lib.ptr(params), _lib.ptr(packed.truths),
                                                       _lib.ptr(packed_t.truths), _lib.ptr(packed.offsets),
                                                       _lib.current_stream(device)), "augment pair sample")
        return params, packed, packed_t

    def apply(self, images, params, images_t=None, to_rgb=True, out=None, out_t=None):
        """The pixels of both frames: two (B, 3, S, S) fp32 tensors from the frames and their pair records."""
        B = len(images)
        dev = images[0].device
        tab = _image_table(images, dev, "images")
        tab_t = None
        if images_t is not None:
            if len(images_t) != B or any(tuple(a.shape) != tuple(b.shape) for a, b in zip(images, images_t)):
                raise ValueError("augment: the second frames must match the first in number and size")
            tab_t = _image_table(images_t, dev, "images_t")
        out, out_t = self._out(out, B, dev), self._out(out_t, B, dev)
        _lib.check(_lib.lib().tdrn_augment_pair_apply(_lib.ptr(tab), _lib.ptr(tab_t), _lib.ptr(params), B, self._mean, self.size,
                                                      1 if to_rgb else 0, _lib.ptr(out), _lib.ptr(out_t),
                                                      _lib.current_stream(dev)), "augment pair apply")
        return out, out_t

    def batch(self, images, targets, sample_ids=None, seed=None, tape=None, images_t=None, targets_t=None, to_rgb=True,
              return_params=False):
        dev = images[0].device
        _lib.require_cuda(images[0], "images")
        if (images_t is None) != (targets_t is None):
            raise ValueError("augment: second frames and their truths come together")
        params, packed, packed_t = self.sample([tuple(im.shape[:2]) for im in images], targets, dev, sample_ids, seed, tape,
                                               targets_t)
        x, x_t = self.apply(images, params, images_t, to_rgb)
        return (x, x_t, packed, packed_t, params) if return_params else (x, x_t, packed, packed_t)

    def __call__(self, img_pair, boxes_pair, labels_pair):
        second = len(img_pair) > 1 and img_pair[1] is not None
        x, x_t, packed, packed_t = self.batch([_frame(img_pair[0])], [_truth_rows(boxes_pair[0], labels_pair[0])],
                                              [next(self._calls)],
                                              images_t=[_frame(img_pair[1])] if second else None,
                                              targets_t=[_truth_rows(boxes_pair[1], labels_pair[1])] if second else None,
                                              to_rgb=False)
        k = int(packed.offsets[1])
        r, r_t = packed.truths[:k], packed_t.truths[:k]
        return [x[0].permute(1, 2, 0), x_t[0].permute(1, 2, 0)], [r[:, :4], r_t[:, :4]], [r[:, 4], r_t[:, 4]]


pairSSDAugmentation = PairSSDAugmentation
