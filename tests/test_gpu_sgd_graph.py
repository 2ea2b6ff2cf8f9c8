"""A whole training step with tdrn_amd.optim.SGD inside it -- forward, multibox_loss, backward, opt.step() in one closure -- run
eagerly, on a side stream and replayed from a captured graph, with the learning rate changed between the first and the second
step through param_group['lr'], as the reference's adjust_learning_rate does (train.py:321-328).

The net and its inputs are test_gpu_train_graph.py's Dense step, copied here.  Three steps on the inputs A, B, A from one initial
state; after each, the losses, every parameter, every BatchNorm buffer and every momentum buffer are compared bit for bit with the
eager run.  The learning rate lives on the device (tdrn_hip.h section i-j): the graph is captured once, sync_hyper() before the
second replay rewrites the device copy, and that replay must take the new value; a replay without the change must differ from it.
"""
import functools

import pytest
import torch

from tdrn_amd.layers.box_utils import PackedTargets, match_targets
from tdrn_amd.layers.modules.multibox_loss import multibox_loss
from tdrn_amd.model import networks
from tdrn_amd.optim import SGD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, CLASSES, ANCHORS, MAP = 2, 5, 2, 20          # 20 x 20 prediction maps, 800 priors
T_TOTAL, MAX_TRUTHS = 5, 4
LRS = (0.05, 0.02, 0.02)                        # the learning rate of steps 0, 1, 2
HYPER = dict(momentum=0.9, weight_decay=5e-4)
VAR = (0.1, 0.2)


class Dense(torch.nn.Module):
    """39 x 39 -> conv -> BN+ReLU -> pool 2/2 ceil (odd map) -> 20 x 20 -> dilated conv -> BN+ReLU -> pool 3/1/1 -> L2Norm -> heads"""

    def __init__(self):
        super(Dense, self).__init__()
        self.c1, self.bn1, self.p1 = networks.Conv2d(3, 16, 3, padding=1), networks.BatchNorm2d(16, relu=True), networks.MaxPool2d(2, 2, ceil_mode=True)
        self.c2, self.bn2, self.p2 = networks.Conv2d(16, 32, 3, padding=2, dilation=2), networks.BatchNorm2d(32, relu=True), networks.MaxPool2d(3, 1, 1)
        self.l2 = networks.L2Norm(32, 10)
        self.loc, self.conf = networks.Conv2d(32, ANCHORS * 4, 3, padding=1), networks.Conv2d(32, ANCHORS * CLASSES, 3, padding=1)

    def forward(self, x):
        f = self.l2(self.p2(self.bn2(self.c2(self.p1(self.bn1(self.c1(x)))))))
        return self.loc(f), self.conf(f)


def _priors():
    c = (torch.arange(MAP, dtype=torch.float32) + 0.5) / MAP
    cy, cx = torch.meshgrid(c, c, indexing="ij")
    per = [torch.stack([cx, cy, torch.full_like(cx, s), torch.full_like(cx, s)], -1) for s in (0.2, 0.35)]
    return torch.stack(per, 2).reshape(-1, 4)                 # prior (i W + j) A + a, the order of the heads' NHWC view


@functools.lru_cache(maxsize=None)
def _inputs():
    """{"A": (x, truths (T_TOTAL, 5), offsets (B + 1)), "B": ...} on the host: other images, other boxes, other counts per image"""
    gen = torch.Generator().manual_seed(41)
    out = {}
    for tag, counts in (("A", (3, 2)), ("B", (1, 4))):
        assert sum(counts) == T_TOTAL and max(counts) <= MAX_TRUTHS
        x = torch.randn((B, 3, 39, 39), generator=gen)
        centre = 0.2 + 0.6 * torch.rand(T_TOTAL, 2, generator=gen)
        half = 0.08 + 0.1 * torch.rand(T_TOTAL, 2, generator=gen)
        label = torch.randint(0, CLASSES - 1, (T_TOTAL, 1), generator=gen).float()
        truths = torch.cat([centre - half, centre + half, label], 1)
        offsets = torch.tensor([0, counts[0], T_TOTAL], dtype=torch.int32)
        out[tag] = (x, truths, offsets)
    return out


class Run(object):
    """one net from the fixed initial state, its optimizer, its static buffers and its step"""

    def __init__(self, zero_grads):
        with torch.random.fork_rng(devices=[]):                  # the modules' default init, the same every time
            torch.manual_seed(7)
            self.net = Dense().to(DEV).train()
        self.start = {k: v.clone() for k, v in self.net.state_dict().items()}
        self.params = list(self.net.parameters())
        self.opt = SGD(self.params, lr=LRS[0], zero_grads=zero_grads, **HYPER)
        for p in self.params:                                    # static gradient and momentum buffers: a graph keeps their addresses
            p.grad = torch.zeros_like(p)
            self.opt.state[p]["momentum_buffer"] = torch.zeros_like(p)
        x, truths, offsets = _inputs()["A"]
        self.x = torch.zeros_like(x, device=DEV)
        self.truths, self.offsets = torch.zeros_like(truths, device=DEV), torch.zeros_like(offsets, device=DEV)
        self.pri = _priors().to(DEV)
        self.loss = torch.zeros(2, device=DEV)

    def restart(self):
        with torch.no_grad():
            for k, v in self.net.state_dict().items():
                v.copy_(self.start[k])                           # in place: a captured graph keeps these addresses
            for p in self.params:
                self.opt.state[p]["momentum_buffer"].zero_()
                p.grad.zero_()
            self.loss.zero_()
        self.set_lr(LRS[0])

    def set_lr(self, lr):
        for group in self.opt.param_groups:                      # what adjust_learning_rate does
            group["lr"] = lr

    def fill(self, tag):
        x, truths, offsets = _inputs()[tag]
        with torch.no_grad():
            self.x.copy_(x.to(DEV))
            self.truths.copy_(truths.to(DEV))
            self.offsets.copy_(offsets.to(DEV))

    def step(self):
        def closure():
            loc, conf = self.net(self.x)
            loc = loc.permute(0, 2, 3, 1).reshape(B, -1, 4)
            conf = conf.permute(0, 2, 3, 1).reshape(B, -1, CLASSES)
            loc_t, conf_t = match_targets(PackedTargets(self.truths, self.offsets, T_TOTAL, MAX_TRUTHS), self.pri, 0.5, VAR)
            loss, _ = multibox_loss(loc, conf, loc_t, conf_t, CLASSES, 3)
            grads = torch.autograd.grad(loss.sum(), self.params)
            with torch.no_grad():
                for p, g in zip(self.params, grads):
                    p.grad.copy_(g)                              # (with zero_grads the step has left +0 here; without, overwritten)
                self.loss.copy_(loss)
            return loss
        self.opt.step(closure)

    def snapshot(self):
        torch.cuda.synchronize()
        s = {"loss": self.loss.clone()}
        s.update({"state." + k: v.clone() for k, v in self.net.state_dict().items()})
        s.update({"momentum.%d" % i: self.opt.state[p]["momentum_buffer"].clone() for i, p in enumerate(self.params)})
        s.update({"grad.%d" % i: p.grad.clone() for i, p in enumerate(self.params)})
        return s


@functools.lru_cache(maxsize=None)
def _eager(zero_grads, lrs=LRS):
    """the three steps on the default stream: computed once, never changed"""
    r = Run(zero_grads)
    out = []
    for tag, lr in zip("ABA", lrs):
        r.set_lr(lr)
        r.fill(tag)
        r.step()
        out.append(r.snapshot())
    for s in out:
        assert bool(torch.isfinite(s["loss"]).all())
    assert not torch.equal(out[0]["loss"], out[2]["loss"])
    for k, v in r.start.items():
        if k.endswith("weight") or k.endswith("running_mean"):       # (a bias in front of a BatchNorm has a zero gradient)
            assert not torch.equal(v, out[0]["state." + k]), k + " did not move in the first step"
    assert any(bool(v.any()) for k, v in out[0].items() if k.startswith("momentum."))
    for k, v in out[2].items():
        if k.startswith("grad.") and zero_grads:
            assert not bool(v.view(torch.int32).any()), k + " is not +0 after a step with zero_grads=True"
    return out


def _compare(how, ref, k, got):
    assert sorted(got) == sorted(ref[k])
    for key, r in ref[k].items():
        g = got[key]
        assert g.dtype == r.dtype and g.shape == r.shape
        assert torch.equal(g.reshape(-1).view(torch.uint8), r.reshape(-1).view(torch.uint8)), \
            "%s: %s differs from the eager run after step %d" % (how, key, k)


def _busy():
    """unrelated work on the default stream, some milliseconds of it, that nothing waits for"""
    a = torch.ones(2048, 2048, device=DEV)
    for _ in range(8):
        a = (a @ a) * 2.0 ** -11
    return a


@pytest.mark.parametrize("zero_grads", [False, True], ids=["keep_grads", "zero_grads"])
def test_step_with_the_optimizer_on_a_side_stream_equals_the_default_stream(zero_grads):
    ref = _eager(zero_grads)
    r = Run(zero_grads)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    for k, tag in enumerate("ABA"):
        keep = _busy()
        r.set_lr(LRS[k])
        with torch.cuda.stream(side):
            r.fill(tag)
            r.step()                               # an eager step syncs the hyper-parameters itself, on this stream
        _compare("side stream", ref, k, r.snapshot())
        assert bool(torch.isfinite(keep).all())


def _captured(zero_grads):
    r = Run(zero_grads)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        r.fill("A")
        r.step()                                   # warm-up: every lazy initialisation happens outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    r.restart()
    r.fill("B")                                    # captured on B's inputs, first replayed on A's
    r.opt.sync_hyper()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r.step()
    r.restart()                                    # (a capture runs nothing; the BatchNorm modules' device counters restart too)
    return r, graph


@pytest.mark.parametrize("zero_grads", [False, True], ids=["keep_grads", "zero_grads"])
def test_step_with_the_optimizer_replayed_from_a_graph_reads_lr_on_the_device(zero_grads):
    ref = _eager(zero_grads)
    r, graph = _captured(zero_grads)
    r.opt.sync_hyper()
    for k, tag in enumerate("ABA"):
        r.fill(tag)
        if LRS[k] != r.opt.param_groups[0]["lr"]:
            r.set_lr(LRS[k])
            r.opt.sync_hyper()                     # the one thing graph mode asks of the user
        graph.replay()
        _compare("graph replay", ref, k, r.snapshot())
    # the same graph without the change of lr: the second step must differ, or lr was baked in at capture
    same_lr = _eager(zero_grads, (LRS[0],) * 3)
    r.restart()
    r.opt.sync_hyper()
    for k, tag in enumerate("ABA"):
        r.fill(tag)
        graph.replay()
        got = r.snapshot()
        _compare("graph replay, lr unchanged", same_lr, k, got)
        if k == 0:
            _compare("graph replay, lr unchanged", ref, 0, got)
        else:
            assert not torch.equal(got["state.c1.weight"], ref[k]["state.c1.weight"]), "step %d ignored the new lr" % k
    del graph


def test_a_stale_mirror_during_capture_raises():
    r, graph = _captured(False)
    r.set_lr(0.5 * LRS[0])                         # param_groups changed, sync_hyper() not called
    before = r.snapshot()
    other = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="sync_hyper"):
        with torch.cuda.graph(other):
            r.step()                               # forward and backward are captured, then the optimizer refuses
    torch.cuda.synchronize()
    _compare("after the refused capture", [before], 0, r.snapshot())
    r.set_lr(LRS[0])                               # back in agreement with the device copy: the first graph still replays
    r.fill("A")
    graph.replay()
    _compare("graph replay after the refused capture", _eager(False), 0, r.snapshot())
    del other, graph
