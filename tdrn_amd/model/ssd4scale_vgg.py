"""4-scale SSD on VGG16: drop-in for model/ssd4scale_vgg.py (SSD4Scale :8-68, forward :71-135,
build_net :146-151) -- the static (deform=False) and temporal (deform=True, 8 deformable groups)
nets the TRN drivers build (train_trn.py:122-124, evaluate_trn.py:541-543, test_video_trn.py:54-56).  `net(x, ...)` is the inference
engine; `net.forward_train(x, ref_loc)` is the differentiable walk train_trn.py's loop needs."""
import torch.nn as nn

from .. import _lib
from ..layers.modules.l2norm import L2Norm
from ._base import EngineModule, TrainWalk
from .networks import ConvOffset2d, vgg, vgg_base
from .ssd4scale_mobile import _OffsetList


class SSD4Scale(EngineModule, TrainWalk):
    def __init__(self, size, num_classes=21, phase='train', c7_channel=1024, bn=True, deform=False):
        super(SSD4Scale, self).__init__()
        self.num_classes, self.size, self.phase, self.bn, self.deform = num_classes, size, phase, bn, deform
        nb = 3
        self.backbone = nn.ModuleList(vgg(vgg_base['320'], 3, batch_norm=bn, pool5_ds=True, c7_channel=c7_channel))
        self.L2Norm_4_3 = L2Norm(512, 10)
        self.L2Norm_5_3 = L2Norm(512, 8)
        if bn:
            self.extras = nn.Sequential(nn.Conv2d(c7_channel, 256, 1), nn.BatchNorm2d(256), nn.ReLU(inplace=True),
                                        nn.Conv2d(256, 512, 3, 2, 1), nn.BatchNorm2d(512), nn.ReLU(inplace=True))
        else:
            self.extras = nn.Sequential(nn.Conv2d(c7_channel, 256, 1), nn.ReLU(inplace=True),
                                        nn.Conv2d(256, 512, 3, 2, 1), nn.ReLU(inplace=True))
        chans = [512, 512, c7_channel, 512]
        if deform:
            g = 8
            self.offset = nn.ModuleList([nn.Conv2d(nb * 4, g * 18, 1) for _ in range(4)])
            mk = lambda cout: nn.ModuleList([ConvOffset2d(c, cout, 3, 1, 1, num_deformable_groups=g) for c in chans])
        else:
            mk = lambda cout: nn.ModuleList([nn.Conv2d(c, cout, 3, 1, 1) for c in chans])
        self.arm_loc, self.arm_conf = mk(nb * 4), mk(nb * num_classes)
        if phase == 'test':
            self.softmax = nn.Softmax(dim=1)
        self._engine_init(model=_lib.SSD4SCALE_VGG, size=size, num_classes=num_classes, c7_channel=c7_channel, bn=bn,
                          deform=deform, test_phase=(phase == 'test'))

    def forward(self, x, ref_loc=list(), offset_list=list(), ret_loc=False, ret_off=False, ref_event=None):
        if self.deform and offset_list:
            # the reference's precedence (ssd4scale_vgg.py:73-78): a non-empty offset_list wins over ref_loc.  Its offsets are a pure
            # function of the loc maps it was computed from, which it carries along: THOSE are the source of truth, whether or
            # not the engine's reuse token is still current (the token only decides whether they are recomputed or still there)
            cached = getattr(offset_list, "ref_loc", None)
            if cached is None:
                raise ValueError("offset_list was not returned by this net (it carries no ref_loc to recompute the offsets from)")
            ref_loc = cached
        elif self.deform and not ref_loc:
            raise ValueError("deform=True needs ref_loc (or an offset_list returned by this net)")
        # (the frames between two key frames hand back the offset_list of the key frame: its offsets are still in the engine's
        # workspace -- the token says so -- and are not recomputed, as in evaluate_trn.py:459-462)
        r = self.engine_for(x).forward(x, want_offsets=bool(ret_off and self.deform),
                                          ref_loc=ref_loc if self.deform else None,
                                          want_loc_maps=bool(ret_loc and not self.deform),
                                          reuse_offsets_token=getattr(offset_list, "token", None) if (self.deform and not ret_off) else None,
                                          ref_event=ref_event)
        conf = r["conf"] if self.phase == 'test' else r["conf"].view(x.size(0), -1, self.num_classes)
        out = [r["arm_loc"], conf]
        if ret_loc:
            out.append(r["loc_maps"])
        if ret_off:
            offs = _OffsetList(r["offsets"] or [])
            offs.ref_loc = list(ref_loc)
            offs.token = r["offsets_token"]
            out.append(offs)
        return tuple(out)

    def forward_train(self, x, ref_loc=(), compute="fp32", ret_loc=False, resident=False):
        """-> (arm_loc (B, P, 4), arm_conf (B, P, num_classes) raw logits): the phase-'train' outputs of forward whatever self.phase
        is, computed from this module's fp32 parameters through the library's differentiable ops (_base.TrainWalk), so that
        `loss.backward()` fills their .grad.  deform=True needs ref_loc, four CUDA tensors (B, 12, Hs, Ws): the static net's loc
        maps (its forward with ret_loc=True); one that requires grad gets a gradient.  ret_loc=True appends the four loc maps (NCHW,
        with their graph) when deform=False and [] when deform=True, as the reference does.  BatchNorm runs in the module's mode;
        `compute` ("fp32" | "bf16" | "fp16") is the MFMA input type of the conv-type ops.  offset_list, ret_off and ref_event belong
        to inference.  The engine's packed weights are marked stale, so net(x) after an optimizer step re-packs by itself.  resident=True (compute "bf16" | "fp16"; ValueError otherwise) keeps the VGG trunk's
        activations and their gradients from conv1_2 to fc7 as 16-bit NHWC tensors between layers; the default,
        resident=False, is unchanged."""
        return self._ssd_forward_train(self._vgg_sources, x, ref_loc, compute, ret_loc, resident)


def build_net(phase, size=320, num_classes=21, c7_channel=1024, bn=False, deform=False):
    if size not in [320, 512]:
        print("Error: Sorry only SSD320 and SSD512 is supported currently!")
        return
    return SSD4Scale(size, num_classes=num_classes, phase=phase, c7_channel=c7_channel, bn=bn, deform=deform)
