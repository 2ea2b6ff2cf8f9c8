"""Shared host-side shell of the model mirrors: an nn.Module that owns the reference's parameter
layout (so `load_state_dict(torch.load(...))`, `.eval()`, `.cuda()` keep working) while `forward`
hands the batch to libtdrn_hip.so through NetEngine (inference), and TrainWalk: what the forward_train of the five models is made
of, on the library's differentiable ops."""
import os

import torch
import torch.nn as nn

from .. import _lib
from ..engine import NetEngine
from . import networks


class EngineModule(nn.Module):
    """Sub-classes set self._engine_args (kwargs of NetEngine) at the end of __init__."""

    def _engine_init(self, **kwargs):
        object.__setattr__(self, "_engine", None)
        object.__setattr__(self, "_size_engines", {})
        object.__setattr__(self, "_engine_args", kwargs)
        object.__setattr__(self, "_dirty", True)
        object.__setattr__(self, "_packs", 0)             # how often this module has (re)packed: what a pipeline_twin watches
        object.__setattr__(self, "_twin_of", None)
        object.__setattr__(self, "compute_dtype", os.environ.get("TDRN_DTYPE", "fp32"))

    # precision switches select the MFMA input type instead of casting the fp32 master params
    def set_plan_flags(self, flags):
        """tdrn_hip.h TDRN_PLAN_* bits of the next engine this module builds (0 = the default plan)."""
        args = dict(self._engine_args)
        args["plan_flags"] = int(flags)
        object.__setattr__(self, "_engine_args", args)
        object.__setattr__(self, "_engine", None)
        object.__setattr__(self, "_size_engines", {})
        object.__setattr__(self, "_dirty", True)
        return self

    def set_compute_dtype(self, name):
        object.__setattr__(self, "compute_dtype", name)
        object.__setattr__(self, "_engine", None)
        object.__setattr__(self, "_size_engines", {})
        object.__setattr__(self, "_dirty", True)
        return self

    def half(self):
        return self.set_compute_dtype("fp16")

    def bfloat16(self):
        return self.set_compute_dtype("bf16")

    def float(self):
        return self.set_compute_dtype("fp32")

    def load_state_dict(self, state_dict, strict=True):
        # PyTorch-0.4 checkpoints have no num_batches_tracked buffers
        own = super().state_dict()
        sd = dict(state_dict)
        for k, v in own.items():
            if k.endswith("num_batches_tracked") and k not in sd:
                sd[k] = v
        r = super().load_state_dict(sd, strict=strict)
        object.__setattr__(self, "_dirty", True)
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        object.__setattr__(self, "_dirty", True)
        return r

    def repack(self):
        """Call after mutating parameters in place (the engine keeps its own packed copy)."""
        object.__setattr__(self, "_dirty", True)

    def engine(self, device):
        if self._twin_of is not None:
            return self._twin_engine(device)
        if self._engine is None:
            args = dict(self._engine_args)
            args["dtype"] = self.compute_dtype
            object.__setattr__(self, "_engine", NetEngine(**args))
            object.__setattr__(self, "_dirty", True)
        if self._dirty or self._engine.device != torch.device(device):
            self._engine.load(super().state_dict(), device)
            object.__setattr__(self, "_dirty", False)
            object.__setattr__(self, "_packs", self._packs + 1)
            object.__setattr__(self, "_size_engines", {})        # they share the blob that was just replaced
        return self._engine

    def _twin_engine(self, device):
        """A twin never packs: it follows its source.  When the source has re-packed since the twin's engine was cloned
        (load_state_dict, set_compute_dtype, set_plan_flags, .to(), repack() -- each leaves the source dirty or with a new
        blob), the twin re-clones from the source's CURRENT engine, so both pipelines always run the same weights and plan."""
        src = self._twin_of
        main = src.engine(device)                        # (re-packs the source first if it is dirty)
        if self._engine is None or self._twin_packs != src._packs or self._engine.weights is not main.weights:
            object.__setattr__(self, "_engine", main.clone())
            object.__setattr__(self, "_twin_packs", src._packs)
            object.__setattr__(self, "_size_engines", {})
            object.__setattr__(self, "compute_dtype", src.compute_dtype)
            object.__setattr__(self, "_engine_args", src._engine_args)
        return self._engine

    def pipeline_twin(self, device):
        """A second handle on this model for a second step in flight (tdrn_amd.engine.InFlight): the same parameters and the same
        packed weight blob, its own engine (workspace, lanes, offset-reuse state): `NetEngine.clone()` behind the module interface."""
        import copy
        src = self._twin_of or self
        twin = copy.copy(src)
        object.__setattr__(twin, "_twin_of", src)             # linked: see _twin_engine (round-5 advisor finding: a twin that only
        object.__setattr__(twin, "_engine", None)             # held the old blob ran stale weights after a reload of the source)
        object.__setattr__(twin, "_twin_packs", -1)
        object.__setattr__(twin, "_size_engines", {})
        object.__setattr__(twin, "_dirty", False)
        twin.engine(device)
        return twin

    def engine_for(self, x):
        """The engine that runs input x.  The reference nets are fully convolutional: multi_eval.py:526-547
        feeds one net frames of 192..704 (1216) pixels.  The plan of a tdrn_net is static per input size, so
        every other size gets its own plan -- built on first use -- over the SAME packed weight blob."""
        main = self.engine(x.device)
        size = int(x.size(-1))
        if size == self._engine_args["size"]:
            return main                                 # (its forward checks the full shape)
        if x.dim() != 4 or x.size(1) != 3 or x.size(2) != size or size % 64 or not 128 <= size <= 1280:
            raise ValueError("expected input (B,3,S,S) with S = %d or another multiple of 64 in [128, 1280], got %r"
                             % (self._engine_args["size"], tuple(x.shape)))
        eng = self._size_engines.get(size)
        if eng is None:
            args = dict(self._engine_args)
            args["dtype"] = self.compute_dtype
            args["size"] = size
            eng = NetEngine(**args)
            eng.share_weights(main)
            self._size_engines[size] = eng
        return eng

    def adopt_broadcast_weights(self, src=0, device=None):
        """Multi-GPU start-up: rank `src` packs, everyone receives the blob by one RCCL broadcast."""
        import torch.distributed as dist
        device = device or torch.device("cuda", torch.cuda.current_device())
        if dist.get_rank() == src:
            eng = self.engine(device)
        else:
            if self._engine is None:
                args = dict(self._engine_args)
                args["dtype"] = self.compute_dtype
                object.__setattr__(self, "_engine", NetEngine(**args))
            eng = self._engine
            eng._alloc_weights(device)
        eng.broadcast_weights(src)
        object.__setattr__(self, "_dirty", False)
        object.__setattr__(self, "_packs", self._packs + 1)
        return eng

    def load_weights(self, base_file):
        ext = os.path.splitext(base_file)[1]
        if ext in (".pkl", ".pth"):
            print("Loading weights into state dict...")
            self.load_state_dict(torch.load(base_file, map_location=lambda storage, loc: storage))
            print("Finished!")
        else:
            print("Sorry only .pth and .pkl files supported.")


def _flatten(layers):
    """the holders of a list, with every nn.Sequential among them replaced by its own (flattened) holders"""
    out = []
    for m in layers:
        out.extend(_flatten(m) if isinstance(m, nn.Sequential) else [m])
    return out


def _is_depthwise3x3(m):
    return (m.groups == m.in_channels == m.out_channels and tuple(m.kernel_size) == (3, 3) and tuple(m.padding) == (1, 1)
            and tuple(m.dilation) == (1, 1))


class TrainWalk(object):
    """What the forward_train of the models is made of: the walk over a list of parameter holders, the VGG and MobileNet source walks,
    the TCB pyramid, the dual-refinement head and the SSD4Scale heads, on the library's differentiable ops.  The ops are looked up on
    `networks` at call time."""

    # the loc and conf heads of an SSD4Scale level with deform=True run as ONE conv_offset2d over their concatenated weights (the
    # input is transposed and gathered, and its gradient scattered, once instead of twice); False: two calls.  Measured: DESIGN 20.
    _paired_heads = True

    def _bn_relu(self, bn, x, resident=False):
        if bn.momentum is None:
            raise NotImplementedError("forward_train: BatchNorm2d(momentum=None) needs a host-side batch count; use networks.BatchNorm2d")
        if self.training and bn.track_running_stats:
            bn.num_batches_tracked.add_(1)            # on the device: no host read, no synchronisation
        op = networks.batch_norm_nhwc if resident else networks.batch_norm
        return op(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, self.training, bn.momentum, bn.eps, relu=True)

    @staticmethod
    def _check_resident(resident, compute, vgg_trunk=True):
        """forward_train's `resident` switch, checked before anything else happens (a refused call does not mark the engine's weights
        stale): the VGG trunks only, and a 16-bit compute type, which is the resident tensors' dtype"""
        if resident and not vgg_trunk:
            raise NotImplementedError("forward_train: resident=True covers the VGG trunks; the MobileNet trunk's depthwise conv is fp32 NCHW")
        if resident and compute not in ("bf16", "fp16"):
            raise ValueError("forward_train: resident=True needs compute 'bf16' or 'fp16', got %r" % (compute,))

    def _check_deform_algo(self, deform_algo, compute):
        """forward_train's `deform_algo` switch of the dual-refinement models, checked like `resident` before anything else happens:
        "gather" (conv_offset2d, the default) or "transform" (conv_offset2d_ts: 16-bit compute types, one deformable group)"""
        if deform_algo not in ("gather", "transform"):
            raise ValueError("forward_train: deform_algo must be 'gather' or 'transform', got %r" % (deform_algo,))
        if deform_algo == "transform":
            if compute not in ("bf16", "fp16"):
                raise ValueError("forward_train: deform_algo='transform' needs compute 'bf16' or 'fp16', got %r" % (compute,))
            if self.def_groups != 1:
                raise NotImplementedError("forward_train: deform_algo='transform' covers def_groups=1, this model has %d" % self.def_groups)

    @staticmethod
    def _resident_conv(m):
        """a conv the resident path takes: the stride-1 family of conv2d_nhwc with whole 64-channel blocks on both sides"""
        return (m.groups == 1 and tuple(m.stride) == (1, 1) and tuple(m.kernel_size) in ((1, 1), (3, 3))
                and m.in_channels % networks.RESIDENT_CHANNELS == 0 and m.out_channels % networks.RESIDENT_CHANNELS == 0)

    def _walk(self, layers, x, compute, taps=(), resident=False):
        """A list of nn.Conv2d [+ nn.BatchNorm2d] [+ nn.ReLU] and nn.MaxPool2d holders, in order, nested nn.Sequentials flattened ->
        (output, [the output behind conv number n (1-based, activation included) for n in taps]).  A dense conv goes to conv2d with
        `compute`; a depthwise 3x3 conv with pad 1 (conv_dw's first layer) goes to depthwise_conv2d, which is fp32.
        resident=True (compute "bf16" | "fp16"): from the first conv of the stride-1 family whose input and output both hold whole
        64-channel blocks on, the activation is a resident tensor (networks.to_nhwc) and stays one through conv2d_nhwc,
        batch_norm_nhwc (or torch.relu) and max_pool2d_nhwc; a conv outside that family takes it back to fp32 NCHW first, and so do
        a tap and the result (networks.from_nhwc)."""
        layers, kept, n_conv, i, nhwc = _flatten(layers), [], 0, 0, False
        while i < len(layers):
            m = layers[i]
            i += 1
            if isinstance(m, nn.MaxPool2d):
                pool = networks.max_pool2d_nhwc if nhwc else networks.max_pool2d
                x = pool(x, m.kernel_size, m.stride, m.padding, m.ceil_mode)
                continue
            if not isinstance(m, nn.Conv2d) or not (m.groups == 1 or _is_depthwise3x3(m)):
                raise NotImplementedError("forward_train: no differentiable op for %r" % (m,))
            if resident and self._resident_conv(m):
                if not nhwc:
                    x, nhwc = networks.to_nhwc(x, compute), True
                x = networks.conv2d_nhwc(x, m.weight, m.bias, m.padding, m.dilation)
            else:
                if nhwc:
                    x, nhwc = networks.from_nhwc(x), False
                if m.groups == 1:
                    x = networks.conv2d(x, m.weight, m.bias, m.padding, m.dilation, compute, m.stride)
                else:
                    x = networks.depthwise_conv2d(x, m.weight, m.bias, m.stride, m.padding)
            if i < len(layers) and isinstance(layers[i], nn.BatchNorm2d):
                x = self._bn_relu(layers[i], x, nhwc)  # the nn.ReLU behind it is fused
                i += 2 if i + 1 < len(layers) and isinstance(layers[i + 1], nn.ReLU) else 1
            elif i < len(layers) and isinstance(layers[i], nn.ReLU):
                x = torch.relu(x)
                i += 1
            n_conv += 1
            if n_conv in taps:
                kept.append(networks.from_nhwc(x) if nhwc else x)
        return (networks.from_nhwc(x) if nhwc else x), kept

    def _train_input(self, x):
        """the checks and the engine mark every forward_train starts with -> the input as fp32"""
        if x.dim() != 4:
            raise ValueError("Expected 4D tensor as input, got {}D tensor instead.".format(x.dim()))
        _lib.require_cuda(x, "input")
        object.__setattr__(self, "_dirty", True)
        return x.float()

    def _vgg_sources(self, x, compute, resident=False):
        """the VGG trunk of the three VGG models -> ([conv4_3 and conv5_3 behind their ReLU and L2Norm, fc7, extras], extras).
        resident: the trunk behind conv1_1, up to and including fc7, on resident tensors (_walk); the taps, fc7 and everything behind
        them are fp32 NCHW either way."""
        self._check_resident(resident, compute)
        x, (c43, c53) = self._walk(self.backbone, x, compute, taps=(10, 13), resident=resident)     # x: fc7
        arm_sources = [networks.l2norm(c43, self.L2Norm_4_3.weight, self.L2Norm_4_3.eps),
                       networks.l2norm(c53, self.L2Norm_5_3.weight, self.L2Norm_5_3.eps), x]
        x, _ = self._walk(self.extras, x, compute)
        arm_sources.append(x)
        return arm_sources, x

    def _mobilenet_sources(self, x, compute, resident=False):
        """the MobileNet trunk of the two MobileNet models -> ([block 11 and block 13 behind their L2Norm, the two extras], extras).
        Its depthwise op is fp32 NCHW: there is no resident path."""
        if resident:
            raise NotImplementedError("forward_train: resident=True covers the VGG trunks; the MobileNet trunk's depthwise conv is fp32 NCHW")
        x, _ = self._walk(self.backbone[:12], x, compute)
        arm_sources = [networks.l2norm(x, self.L2Norm_4_3.weight, self.L2Norm_4_3.eps)]
        x, _ = self._walk(self.backbone[12:], x, compute)
        arm_sources.append(networks.l2norm(x, self.L2Norm_5_3.weight, self.L2Norm_5_3.eps))
        for block in self.extras:
            x, _ = self._walk(block, x, compute)
            arm_sources.append(x)
        return arm_sources, x

    def _ssd_heads_train(self, arm_sources, ref_loc, compute, ret_loc):
        """the heads of the two SSD4Scale models from their four sources -> forward_train's tuple.  deform=False: two conv2d per
        level.  deform=True: offsets from ref_loc[s] by the 1x1 conv offset[s], then both deformable heads over them."""
        B = arm_sources[0].size(0)
        locs, confs, loc_maps = [], [], []
        if self.deform:
            if not ref_loc:
                raise ValueError("deform=True needs ref_loc")
            if len(ref_loc) != 4:
                raise ValueError("ref_loc must hold four loc maps, got %d" % len(ref_loc))
            for s, (a, r) in enumerate(zip(arm_sources, ref_loc)):
                want = (B, self.offset[s].in_channels) + tuple(a.shape[2:])
                if not torch.is_tensor(r) or tuple(r.shape) != want:
                    raise ValueError("ref_loc[%d] must be a tensor of shape %r, got %r" % (s, want, tuple(getattr(r, "shape", ()))))
                _lib.require_cuda(r, "ref_loc[%d]" % s)
        for s, a in enumerate(arm_sources):
            hl, hc = self.arm_loc[s], self.arm_conf[s]
            if not self.deform:
                loc = networks.conv2d(a, hl.weight, hl.bias, 1, 1, compute)
                conf = networks.conv2d(a, hc.weight, hc.bias, 1, 1, compute)
                loc_maps.append(loc)
            else:
                off = networks.conv2d(ref_loc[s].float(), self.offset[s].weight, self.offset[s].bias, 0, 1, compute)
                if self._paired_heads:
                    both = networks.conv_offset2d(a, off, torch.cat([hl.weight, hc.weight]), 1, 1, 1, hl.num_deformable_groups, compute)
                    loc, conf = both.split([hl.out_channels, hc.out_channels], 1)
                else:
                    loc, conf = (networks.conv_offset2d(a, off, h.weight, 1, 1, 1, h.num_deformable_groups, compute) for h in (hl, hc))
            locs.append(loc.permute(0, 2, 3, 1).contiguous().view(B, -1))
            confs.append(conf.permute(0, 2, 3, 1).contiguous().view(B, -1))
        out = (torch.cat(locs, 1).view(B, -1, 4), torch.cat(confs, 1).view(B, -1, self.num_classes))
        return out + (loc_maps,) if ret_loc else out

    def _ssd_forward_train(self, sources, x, ref_loc, compute, ret_loc, resident=False):
        """forward_train of the two SSD4Scale models; `sources`: _vgg_sources or _mobilenet_sources"""
        self._check_resident(resident, compute, sources == self._vgg_sources)
        x = self._train_input(x)
        arm_sources, _ = sources(x, compute, resident)
        return self._ssd_heads_train(arm_sources, ref_loc, compute, ret_loc)

    def _tcb_train(self, arm_sources, x, compute):
        """last_layer_trans and the TCB pyramid (trans_layers, up_layers, latent_layers) from the four ARM sources and the last
        feature map x -> the four ODM sources, largest map first"""
        conv = lambda m, t, pad: networks.conv2d(t, m.weight, m.bias, pad, 1, compute)
        x, _ = self._walk(self.last_layer_trans, x, compute)
        odm_sources = [x]
        trans = [self._walk(self.trans_layers[s], arm_sources[s], compute)[0] for s in range(3)]
        trans.reverse()
        for i, t in enumerate(trans):
            up = self.up_layers[i]
            u = torch.relu(networks.conv_transpose2d(x, up.weight, up.bias, 2, compute) + t)
            x = torch.relu(conv(self.latent_layers[i], u, 1))
            odm_sources.append(x)
        odm_sources.reverse()
        return odm_sources

    def _head_train(self, arm_sources, x, compute, deform_algo="gather"):
        """ARM loc / offsets, last_layer_trans, the TCB pyramid and the deformable heads (add_refine_head's modules, with or without
        biases) from the four ARM sources and the last feature map x -> forward_train's 4-tuple.
        deform_algo="transform": the loc and conf heads of one (level, branch) run as ONE conv_offset2d_ts over their concatenated
        weights (one Y, one scatter, one grad_offset: what _paired_heads does for SSD4Scale); the multihead branch is a second call."""
        B = x.size(0)
        conv = lambda m, t, pad: networks.conv2d(t, m.weight, m.bias, pad, 1, compute)
        arm_loc, off1, off2 = [], [], []
        for s, a in enumerate(arm_sources):
            loc_a = conv(self.arm_loc[s], a, 1)
            arm_loc.append(loc_a.permute(0, 2, 3, 1).contiguous().view(B, -1))
            off1.append(conv(self.offset[s], loc_a, 0))
            if self.multihead:
                off2.append(conv(self.offset2[s], loc_a, 0))
        odm_sources = self._tcb_train(arm_sources, x, compute)
        odm_loc, odm_conf = [], []
        for s, ob in enumerate(odm_sources):
            heads = [(self.odm_loc[s], self.odm_conf[s], off1[s])]
            if self.multihead:
                heads.append((self.odm_loc_2[s], self.odm_conf_2[s], off2[s]))
            l = c = None
            for hl, hc, off in heads:
                if deform_algo == "transform":
                    both = networks.conv_offset2d_ts(ob, off, torch.cat([hl.weight, hc.weight]), hl.stride, hl.padding, hl.dilation, compute)
                    dl, dc = both.split([hl.out_channels, hc.out_channels], 1)
                else:
                    dl, dc = (networks.conv_offset2d(ob, off, h.weight, h.stride, h.padding, h.dilation, h.num_deformable_groups, compute)
                              for h in (hl, hc))
                l, c = (dl, dc) if l is None else (l + dl, c + dc)
            odm_loc.append(l.permute(0, 2, 3, 1).contiguous().view(B, -1))
            odm_conf.append(c.permute(0, 2, 3, 1).contiguous().view(B, -1))
        return (torch.cat(arm_loc, 1).view(B, -1, 4), None, torch.cat(odm_loc, 1).view(B, -1, 4),
                torch.cat(odm_conf, 1).view(B, -1, self.num_classes))

    def _refinedet_head_train(self, arm_sources, x, compute):
        """refinedet_vgg's heads: ARM loc (use_refine), the TCB pyramid and the dense ODM heads, 3x3 through conv2d and, with
        multihead, 5x5 through conv5x5, summed -> forward_train's tuple"""
        B = x.size(0)
        conv = lambda m, t: networks.conv2d(t, m.weight, m.bias, 1, 1, compute)
        if self.use_refine:
            arm_loc = [conv(self.arm_loc[s], a).permute(0, 2, 3, 1).contiguous().view(B, -1) for s, a in enumerate(arm_sources)]
        odm_loc, odm_conf = [], []
        for s, ob in enumerate(self._tcb_train(arm_sources, x, compute)):
            l, c = conv(self.odm_loc[s], ob), conv(self.odm_conf[s], ob)
            if self.multihead:
                l = l + networks.conv5x5(ob, self.odm_loc_2[s].weight, self.odm_loc_2[s].bias, compute)
                c = c + networks.conv5x5(ob, self.odm_conf_2[s].weight, self.odm_conf_2[s].bias, compute)
            odm_loc.append(l.permute(0, 2, 3, 1).contiguous().view(B, -1))
            odm_conf.append(c.permute(0, 2, 3, 1).contiguous().view(B, -1))
        out = (torch.cat(odm_loc, 1).view(B, -1, 4), torch.cat(odm_conf, 1).view(B, -1, self.num_classes))
        return (torch.cat(arm_loc, 1).view(B, -1, 4), None) + out if self.use_refine else out
