"""The training ops on a side stream and under hipGraph capture (tdrn_hip.h: every training entry promises "no allocation and no
host synchronisation: everything is enqueued on `stream`").

Two small training steps, each a closure over static input buffers: forward, multibox loss, backward, in-place SGD.  Step k reads
the parameters and BatchNorm buffers step k - 1 wrote.  Each step runs three times, on the inputs A, B, A, from one initial state:

  eager on the default stream                                       the values everything else is compared with
  eager inside torch.cuda.stream(side), unrelated work queued on the default stream meanwhile
  captured once with torch.cuda.graph (after a warm-up on the side stream, the state put back), replayed three times with the
  static inputs refilled

After every step the losses, sel, num_pos, every parameter and every buffer are compared.  A launch that went to another stream
than the one it was given either fails the capture or is not part of the graph, and then the replay on B (captured on A)
disagrees; a host read fails the capture.

dense_step uses only entries whose outputs the header calls bitwise reproducible: everything is compared bit for bit.
deform_step: ConvOffset2d's grad_input is accumulated with float atomics (the header says so); here it reaches nothing but the
gradient of the static feature map, which is compared within test_gpu_deform_grad.py's bound, 1e-4 * max(1, max|eager|), of the
eager values.  Everything else is bit for bit again.

What these tests found when they were written: conv2d and conv_offset2d zeroed parts of their workspace with hipMemsetAsync, and a
captured memset node took effect in the first launch of the graph only.  From the second replay on dense_step's losses, sel and
every parameter differed from the eager run, and deform_step's feature gradient was off by 5.5e-2.  The entries zero with a kernel
now (launch_fill_zero); test_conv2d_replayed_over_a_dirty_workspace_zeroes_it_again holds that alone.

The truths are packed once, outside the step, into static PackedTargets buffers: match_targets' packing of a list of host tensors
goes through pinned host memory, which a graph cannot re-read.  The counts per image differ between A and B inside fixed host
bounds (T_total, max_truths), as PackedTargets allows.
"""
import functools

import pytest
import torch

from tdrn_amd import _lib
from tdrn_amd.layers.box_utils import PackedTargets, match_targets
from tdrn_amd.layers.modules.multibox_loss import multibox_loss
from tdrn_amd.model import networks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, CLASSES, ANCHORS, MAP = 2, 5, 2, 20          # 20 x 20 prediction maps, 800 priors
T_TOTAL, MAX_TRUTHS = 5, 4
LR = 0.05
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


class Deform(torch.nn.Module):
    """a fixed 20 x 20 feature map -> 1x1 offset conv -> deformable loc and conf heads"""

    def __init__(self):
        super(Deform, self).__init__()
        self.off = networks.Conv2d(16, 2 * 9, 1)
        self.loc, self.conf = networks.ConvOffset2d(16, ANCHORS * 4, 3, padding=1), networks.ConvOffset2d(16, ANCHORS * CLASSES, 3, padding=1)

    def forward(self, x):
        o = self.off(x)
        return self.loc(x, o), self.conf(x, o)


STEPS = {"dense_step": (Dense, (B, 3, 39, 39)), "deform_step": (Deform, (B, 16, MAP, MAP))}


def _priors():
    c = (torch.arange(MAP, dtype=torch.float32) + 0.5) / MAP
    cy, cx = torch.meshgrid(c, c, indexing="ij")
    per = [torch.stack([cx, cy, torch.full_like(cx, s), torch.full_like(cx, s)], -1) for s in (0.2, 0.35)]
    return torch.stack(per, 2).reshape(-1, 4)                 # prior (i W + j) A + a, the order of the heads' NHWC view


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """{"A": (x, truths (T_TOTAL, 5), offsets (B + 1)), "B": ...} on the host: other images, other boxes, other counts per image"""
    gen = torch.Generator().manual_seed(41 + sorted(STEPS).index(name))
    out = {}
    for tag, counts in (("A", (3, 2)), ("B", (1, 4))):
        assert sum(counts) == T_TOTAL and max(counts) <= MAX_TRUTHS
        x = torch.randn(STEPS[name][1], generator=gen)
        centre = 0.2 + 0.6 * torch.rand(T_TOTAL, 2, generator=gen)
        half = 0.08 + 0.1 * torch.rand(T_TOTAL, 2, generator=gen)
        label = torch.randint(0, CLASSES - 1, (T_TOTAL, 1), generator=gen).float()
        truths = torch.cat([centre - half, centre + half, label], 1)
        offsets = torch.tensor([0, counts[0], T_TOTAL], dtype=torch.int32)
        out[tag] = (x, truths, offsets)
    return out


class Run(object):
    """one net from the fixed initial state, its static buffers and its step"""

    def __init__(self, name):
        self.name = name
        with torch.random.fork_rng(devices=[]):                  # the modules' default init, the same every time
            torch.manual_seed(7)
            self.net = STEPS[name][0]().to(DEV).train()
        self.start = {k: v.clone() for k, v in self.net.state_dict().items()}
        self.params = list(self.net.parameters())
        x, truths, offsets = _inputs(name)["A"]
        self.x = torch.zeros_like(x, device=DEV).requires_grad_(name == "deform_step")
        self.truths, self.offsets = torch.zeros_like(truths, device=DEV), torch.zeros_like(offsets, device=DEV)
        self.pri = _priors().to(DEV)
        self.loss = torch.zeros(2, device=DEV)
        self.sel = torch.zeros(B, MAP * MAP * ANCHORS, dtype=torch.uint8, device=DEV)
        self.gx = torch.zeros_like(self.x) if name == "deform_step" else None

    def restart(self):
        with torch.no_grad():
            for k, v in self.net.state_dict().items():
                v.copy_(self.start[k])                           # in place: a captured graph keeps these addresses
            self.loss.zero_()
            self.sel.zero_()

    def fill(self, tag):
        x, truths, offsets = _inputs(self.name)[tag]
        with torch.no_grad():
            self.x.copy_(x.to(DEV))
            self.truths.copy_(truths.to(DEV))
            self.offsets.copy_(offsets.to(DEV))

    def step(self):
        loc, conf = self.net(self.x)
        loc = loc.permute(0, 2, 3, 1).reshape(B, -1, 4)
        conf = conf.permute(0, 2, 3, 1).reshape(B, -1, CLASSES)
        loc_t, conf_t = match_targets(PackedTargets(self.truths, self.offsets, T_TOTAL, MAX_TRUTHS), self.pri, 0.5, VAR)
        loss, sel = multibox_loss(loc, conf, loc_t, conf_t, CLASSES, 3)
        wanted = self.params + ([self.x] if self.gx is not None else [])
        grads = torch.autograd.grad(loss.sum(), wanted)
        with torch.no_grad():
            for p, g in zip(self.params, grads):
                p.add_(g, alpha=-LR)
            self.loss.copy_(loss)
            self.sel.copy_(sel)
            if self.gx is not None:
                self.gx.copy_(grads[-1])

    def snapshot(self):
        torch.cuda.synchronize()
        s = {"loss": self.loss.clone(), "sel": self.sel.clone(), "num_pos": (self.sel == 1).sum(1)}
        s.update({"state." + k: v.clone() for k, v in self.net.state_dict().items()})
        if self.gx is not None:
            s["grad_feature"] = self.gx.clone()
        return s


@functools.lru_cache(maxsize=None)
def _eager(name):
    """the three steps on the default stream: computed once, never changed"""
    r = Run(name)
    out = []
    for tag in "ABA":
        r.fill(tag)
        r.step()
        out.append(r.snapshot())
    # the steps are real ones: finite losses, positives and mined negatives, parameters that move, B unlike A
    for s in out:
        assert bool(torch.isfinite(s["loss"]).all()) and int(s["num_pos"].min()) >= 1 and int((s["sel"] == 2).sum()) > 0
    assert not torch.equal(out[0]["sel"], out[1]["sel"]) and not torch.equal(out[0]["loss"], out[2]["loss"])
    for k, v in r.start.items():
        if k.endswith("weight") or k.endswith("running_mean"):       # (a bias in front of a BatchNorm has a zero gradient)
            assert not torch.equal(v, out[0]["state." + k]), k + " did not move in the first step"
    return out


def _compare(name, how, k, got):
    ref = _eager(name)[k]
    assert sorted(got) == sorted(ref)
    for key, r in ref.items():
        g = got[key]
        if key == "grad_feature":
            d, bound = float((g.double() - r.double()).abs().max()), 1e-4 * max(1.0, float(r.abs().max()))
            print("%s %s step %d grad_feature max|d| %.3e  bound %.3e" % (name, how, k, d, bound))
            assert bool(torch.isfinite(g).all()) and d <= bound, (name, how, k, d, bound)
        else:
            assert g.dtype == r.dtype and g.shape == r.shape
            assert torch.equal(g.reshape(-1).view(torch.uint8), r.reshape(-1).view(torch.uint8)), \
                "%s %s: %s differs from the eager run after step %d" % (name, how, key, k)


def _busy():
    """unrelated work on the default stream, some milliseconds of it, that nothing waits for"""
    a = torch.ones(2048, 2048, device=DEV)
    for _ in range(8):
        a = (a @ a) * 2.0 ** -11
    return a


@pytest.mark.parametrize("name", list(STEPS))
def test_training_step_on_a_side_stream_equals_the_default_stream(name):
    _eager(name)
    r = Run(name)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    for k, tag in enumerate("ABA"):
        keep = _busy()
        with torch.cuda.stream(side):
            r.fill(tag)
            r.step()
        _compare(name, "side stream", k, r.snapshot())
        assert bool(torch.isfinite(keep).all())


@pytest.mark.parametrize("name", list(STEPS))
def test_training_step_replayed_from_a_graph_equals_eager(name):
    _eager(name)
    r = Run(name)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        r.fill("A")
        r.step()                                   # warm-up: every lazy initialisation happens outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    r.restart()
    r.fill("B")                                    # captured on B's inputs, first replayed on A's
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r.step()
    r.restart()                                    # (a capture runs nothing; the BatchNorm modules' device counters restart too)
    for k, tag in enumerate("ABA"):
        r.fill(tag)
        graph.replay()
        _compare(name, "graph replay", k, r.snapshot())
    del graph


def test_conv2d_replayed_over_a_dirty_workspace_zeroes_it_again():
    """What the graph test found, alone: the entries zero parts of their workspace (the zero page the padding taps read, the padded
    bias) on every call.  Done with hipMemsetAsync, that took effect in the first launch of a captured graph only; from the second
    replay on the border pixels read what other kernels had left there.  Here a kernel dirties the workspace inside the graph."""
    lib, dt = _lib.lib(), _lib.DTYPES["fp32"]
    dims = (2, 6, 9, 7, 4, 3, 3, 1, 1, 1, 1, 1, 1)
    gen = torch.Generator().manual_seed(3)
    x, w, b = (torch.randn(s, generator=gen).to(DEV) for s in ((2, 6, 9, 7), (4, 6, 3, 3), (4,)))
    nb = lib.tdrn_conv2d_workspace_bytes(*dims, dt)
    ws = torch.zeros((nb + 3) // 4, dtype=torch.int32, device=DEV)
    out = torch.full((2, 4, 9, 7), float("nan"), device=DEV)

    def work():
        ws.fill_(0x4B000000)                       # 8388608.0 in every word
        _lib.check(lib.tdrn_conv2d_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(out), *dims, dt, _lib.ptr(ws), nb,
                                           _lib.current_stream(DEV)))
    work()
    torch.cuda.synchronize()
    want = out.clone()
    ref = torch.nn.functional.conv2d(x.cpu().double(), w.cpu().double(), b.cpu().double(), 1, 1)
    assert float((want.cpu().double() - ref).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max()))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        work()
    for k in range(3):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), "replay %d: %d of %d outputs differ" % (
            k, int((out != want).sum()), out.numel())


@pytest.mark.parametrize("name", list(STEPS))
def test_training_step_does_not_synchronise_with_the_host(name):
    r = Run(name)
    r.fill("A")
    r.step()                                       # (lazy initialisation may synchronise once)
    r.fill("B")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r.step()
        honoured = True
        try:
            _ = torch.ones(2, device=DEV).nonzero()
            honoured = False
        except RuntimeError:
            pass
    finally:
        torch.cuda.set_sync_debug_mode(0)
    print("sync debug mode honoured by this build: %s" % honoured)
    assert bool(torch.isfinite(r.snapshot()["loss"]).all())
