"""SSDAugmentation on the device (utils/augmentations.py:618-635 of the reference) through libtdrn_hip.so (tdrn_hip.h section
ii-c).

Raw uint8 BGR frames go in; out come the network input (B, 3, S, S) fp32 and the packed truths that MultiBoxLoss /
RefineMultiBoxLoss consume (PackedTargets), with no host synchronisation in between.  The semantics are the reference's,
quirks included; the deviations (bounded crop rounds, no crop for an image without truths, the Philox draw source) are
listed in the header."""
import ctypes as C
import itertools

import numpy as np
import torch

from .. import _lib
from ..layers.box_utils import PackedTargets, _to_device

PARAMS_BYTES = C.sizeof(_lib.AugmentParams)


def _host_bytes(struct_array):
    return torch.frombuffer(bytearray(struct_array), dtype=torch.uint8)


def params_to_dicts(params):
    """Decode a (B, PARAMS_BYTES) uint8 tensor of tdrn_augment_params records (synchronises when it is on the device)."""
    raw = params.detach().cpu().contiguous().numpy().tobytes()
    out = []
    for b in range(len(raw) // PARAMS_BYTES):
        p = _lib.AugmentParams.from_buffer_copy(raw[b * PARAMS_BYTES:(b + 1) * PARAMS_BYTES])
        d = {k: getattr(p, k) for k, _ in p._fields_}
        d["perm"] = tuple(p.perm)
        d["crop"] = (p.crop_x0, p.crop_y0, p.crop_x1, p.crop_y1)
        out.append(d)
    return out


class SSDAugmentation(object):
    """The reference's SSDAugmentation(size, mean), batched on the GPU.

    batch(images, targets, sample_ids, seed) is the fast path: images is a list of B uint8 (H, W, 3) BGR tensors on the
    device, targets a list of B (n, 5) tensors of fractions [x1, y1, x2, y2, label] (as detection_collate yields them, on any
    device).  A sample's result depends on (seed, sample id) alone.  It returns (x (B, 3, S, S) fp32, PackedTargets); x is in
    RGB order (VOCDetection.pull_item swaps after the transform) unless to_rgb=False.

    __call__(img, boxes, labels) is the one-image convenience with the reference's signature: it returns device tensors
    (image (S, S, 3) fp32 BGR, boxes (k, 4), labels (k,)) and, unlike batch, synchronises to learn k."""

    def __init__(self, size=300, mean=(104, 117, 123), seed=0):
        self.size = int(size)
        self.mean = mean
        self.seed = int(seed)
        self._mean = (C.c_float * 3)(*[float(m) for m in mean])
        self._calls = itertools.count()

    def sample(self, hw, targets, device, sample_ids=None, seed=None, tape=None):
        """The decisions and the moved boxes: (params (B, PARAMS_BYTES) uint8, PackedTargets).  hw: B (h, w) pairs (host).
        Exactly one source: sample_ids (+ seed) for Philox, or tape (B host arrays of the reference's draws)."""
        B = len(hw)
        if B == 0 or len(targets) != B:
            raise ValueError("augment: %d images and %d targets" % (B, len(targets)))
        counts = [int(t.reshape(-1, 5).size(0)) for t in targets]
        offs = np.zeros(B + 1, np.int32)
        offs[1:] = np.cumsum(counts)
        T, Tmax = int(offs[-1]), max(counts)
        if Tmax > _lib.AUGMENT_MAX_TRUTHS:
            raise _lib.TdrnError(-4, "augment: %d truths in one image (at most %d)" % (Tmax, _lib.AUGMENT_MAX_TRUTHS))
        rows = [t.reshape(-1, 5).to(torch.float64) for t in targets if t.numel()]
        truths = None
        if rows:
            truths = _to_device(torch.cat([r.to(rows[0].device) for r in rows]).contiguous(), device)
        off = _to_device(torch.from_numpy(offs), device)
        hw_t = _to_device(torch.tensor([[int(h), int(w)] for h, w in hw], dtype=torch.int32), device)
        ids = tp = tp_off = None
        if tape is not None:
            lens = np.zeros(B + 1, np.int32)
            lens[1:] = np.cumsum([len(t) for t in tape])
            tp = _to_device(torch.from_numpy(np.concatenate([np.asarray(t, np.float64) for t in tape] + [np.zeros(1)])), device)
            tp_off = _to_device(torch.from_numpy(lens), device)
        else:
            if sample_ids is None:
                raise ValueError("augment: sample_ids (with seed) or a tape is needed")
            ids = torch.as_tensor(sample_ids, dtype=torch.int64).reshape(-1)
            if ids.numel() != B:
                raise ValueError("augment: %d sample ids for %d images" % (ids.numel(), B))
            ids = _to_device(ids.contiguous(), device)
        params = torch.empty(B, PARAMS_BYTES, dtype=torch.uint8, device=device)
        out_truths = torch.empty(max(T, 1), 5, dtype=torch.float32, device=device)
        out_off = torch.empty(B + 1, dtype=torch.int32, device=device)
        s = self.seed if seed is None else int(seed)
        _lib.check(_lib.lib().tdrn_augment_sample(_lib.ptr(hw_t), _lib.ptr(truths), _lib.ptr(off), T, Tmax, B,
                                                  s & 0xFFFFFFFFFFFFFFFF, _lib.ptr(ids), _lib.ptr(tp), _lib.ptr(tp_off),
                                                  _lib.ptr(params), _lib.ptr(out_truths), _lib.ptr(out_off),
                                                  _lib.current_stream(device)), "augment sample")
        return params, PackedTargets(out_truths, out_off, T, Tmax)

    def apply(self, images, params, to_rgb=True, out=None):
        """The pixels: (B, 3, S, S) fp32 from the frames and their parameter records."""
        B = len(images)
        dev = images[0].device
        tab = (_lib.AugmentImage * B)()
        for b, im in enumerate(images):
            _lib.require_cuda(im, "images[%d]" % b)
            if im.dtype != torch.uint8 or im.dim() != 3 or im.size(2) != 3 or not im.is_contiguous():
                raise ValueError("augment: images[%d] must be a contiguous uint8 (H, W, 3) tensor" % b)
            tab[b].data, tab[b].h, tab[b].w = im.data_ptr(), im.size(0), im.size(1)
        tab_d = _to_device(_host_bytes(tab), dev)
        S = self.size
        if out is None:
            out = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().tdrn_augment_apply(_lib.ptr(tab_d), _lib.ptr(params), B, self._mean, S, 1 if to_rgb else 0,
                                                 _lib.ptr(out), _lib.current_stream(dev)), "augment apply")
        return out

    def batch(self, images, targets, sample_ids=None, seed=None, tape=None, to_rgb=True, return_params=False):
        dev = images[0].device
        _lib.require_cuda(images[0], "images")
        params, packed = self.sample([tuple(im.shape[:2]) for im in images], targets, dev, sample_ids, seed, tape)
        x = self.apply(images, params, to_rgb)
        return (x, packed, params) if return_params else (x, packed)

    def __call__(self, img, boxes, labels):
        img = torch.as_tensor(img)
        if not img.is_cuda:
            img = img.to("cuda")
        img = img.to(torch.uint8).contiguous()
        b = torch.as_tensor(boxes, dtype=torch.float64).reshape(-1, 4)
        lab = torch.as_tensor(labels, dtype=torch.float64).reshape(-1, 1).to(b.device)
        x, packed = self.batch([img], [torch.cat([b, lab], 1)], [next(self._calls)], to_rgb=False)
        k = int(packed.offsets[1])
        rows = packed.truths[:k]
        return x[0].permute(1, 2, 0), rows[:, :4], rows[:, 4]
