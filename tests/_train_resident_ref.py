"""CPU restatement of the part of RefineSSD.forward_train (dualrefinedet_vggbn) in front of the deformable heads, with or without
BatchNorm (test helper; product code never imports it): the VGG trunk, L2Norm, extras and the four ARM loc heads -> arm_loc.

With bn=True it is tests/_train_net_ref.py's walk (the same ops in the same order; test_gpu_train_resident.py checks that the two
agree exactly in float64); with bn=False every `bn_relu(conv(...))` is `F.relu(conv(...))` and the state-dict indices are those of
vgg(batch_norm=False): a conv every 2 holders instead of every 3, extras.0 and extras.2.  Computed in the dtype it is given:
float64 is the reference, float32 the check that no ReLU or max-pool decision flip dominates a distance to it."""
import numpy as np
import torch
import torch.nn.functional as F

VGG_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "C", 512, 512, 512, "M", 512, 512, 512]
MOMENTUM, EPS = 0.1, 1e-5


def arm_loc(sd, x, bn, dtype):
    """training-mode forward -> arm_loc (B, P, 4) in `dtype`; `sd`: the module's state dict (numpy or torch), never changed"""
    P = {k: torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v.detach().cpu()).clone() for k, v in sd.items()}
    P = {k: (v if k.endswith("num_batches_tracked") else v.to(dtype)) for k, v in P.items()}
    x = torch.as_tensor(x).to(dtype)
    step = 3 if bn else 2

    def conv(name, t, stride=1, padding=0, dilation=1):
        return F.conv2d(t, P[name + ".weight"], P.get(name + ".bias"), stride, padding, dilation)

    def act(prefix, idx, t):
        """the activation behind conv number idx of `prefix`: BatchNorm (batch statistics) + ReLU, or ReLU"""
        if not bn:
            return F.relu(t)
        name = "%s.%d" % (prefix, idx + 1)
        return F.relu(F.batch_norm(t, P[name + ".running_mean"], P[name + ".running_var"], P[name + ".weight"], P[name + ".bias"], True,
                                   MOMENTUM, EPS))

    with torch.no_grad():
        idx, n_conv, feats = 0, 0, []
        for v in VGG_CFG:
            if v in ("M", "C"):
                x = F.max_pool2d(x, 2, 2, ceil_mode=(v == "C"))
                idx += 1
                continue
            x = act("backbone", idx, conv("backbone.%d" % idx, x, padding=1))
            idx += step
            n_conv += 1
            if n_conv in (10, 13):
                feats.append(x)
        x = F.max_pool2d(x, 2, 2)
        idx += 1
        x = act("backbone", idx, conv("backbone.%d" % idx, x, padding=6, dilation=6))
        idx += step
        x = act("backbone", idx, conv("backbone.%d" % idx, x))
        l2 = lambda name, t: P[name + ".weight"].view(1, -1, 1, 1) * (t / (t.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10))
        srcs = [l2("L2Norm_4_3", feats[0]), l2("L2Norm_5_3", feats[1]), x]
        e = act("extras", 0, conv("extras.0", x))
        srcs.append(act("extras", step, conv("extras.%d" % step, e, stride=2, padding=1)))
        B = x.size(0)
        arm = [conv("arm_loc.%d" % s, a, padding=1).permute(0, 2, 3, 1).contiguous().view(B, -1) for s, a in enumerate(srcs)]
        return torch.cat(arm, 1).view(B, -1, 4)
