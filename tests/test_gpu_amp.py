"""Dynamic loss scaling on the card (tdrn_hip.h section i-m) against its numpy restatement (tests/_amp_ref.py), bit for bit:
tdrn_amp_check_finite, tdrn_sgd_step_scaled and tdrn_amp_update through the C entries, then tdrn_amd.amp.GradScaler on top.

A list of tensors lives in three flat buffers (p, g, b), each tensor at a 16-byte aligned offset or one float past it (the scalar
path), with gaps in between; the whole buffers are compared, so a write outside a tensor shows as well.  Sizes sit around the
kernel's paths: below one vector, a vector and its numel % 4 tail, a chunk (_lib.SGD_CHUNK) minus / plus one, several chunks.
"""
import ctypes

import numpy as np
import pytest
import torch

import _amp_ref as A
import _sgd_ref as R
from tdrn_amd import _lib
from tdrn_amd.amp import GradScaler
from tdrn_amd.optim import SGD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK, K = _lib.SGD_CHUNK, _lib.SGD_TENSORS_PER_LAUNCH
SIZES = [1, 3, 4, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
MODES = {"no_momentum": dict(momentum=0.0), "momentum": dict(momentum=0.9), "momentum_wd": dict(momentum=0.9, weight_decay=5e-4),
         "nesterov_wd": dict(momentum=0.9, weight_decay=5e-4, nesterov=True)}
FLT_MAX = float(np.finfo(np.float32).max)


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(a).reshape(-1).view(np.int32)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, what
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d" % (what, bad.size, g.size, bad[0])


def _hyper(hps):
    return torch.tensor([[h["lr"], h.get("momentum", 0.0), h.get("weight_decay", 0.0), float(h.get("nesterov", False))] for h in hps],
                        dtype=torch.float32, device=DEV)


def _state(scale=65536.0, good=0.0, found=0.0, skipped=0.0):
    t = torch.tensor([scale, good, found, skipped], dtype=torch.float32, device=DEV)
    assert t.data_ptr() % 16 == 0
    return t


class Pack(object):
    """tensors i = 0.. of sizes[i] elements in three flat buffers; tensor i starts one float off the 16-byte grid where off[i];
    skip: {i: "null grad" | "numel 0"}; group i % n_groups"""

    def __init__(self, sizes, off, seed, n_groups=1, skip=None):
        self.sizes, self.skip, self.n_groups = list(sizes), dict(skip or {}), n_groups
        self.at, end = [], 8
        for n, o in zip(sizes, off):
            start = (end + 3) // 4 * 4 + 4 + (1 if o else 0)          # at least four floats of gap
            self.at.append(start)
            end = start + n
        self.total = end + 8
        gen = torch.Generator().manual_seed(seed)
        self.host = [torch.randn(self.total, generator=gen).numpy().copy() for _ in range(3)]       # p, g, b
        self.dev = None

    def view(self, which, i):
        return self.host[which][self.at[i]:self.at[i] + self.sizes[i]]

    def upload(self):
        self.dev = [torch.from_numpy(h).to(DEV) for h in self.host]
        assert all(d.data_ptr() % 16 == 0 for d in self.dev)
        self.recs = (_lib.SgdTensor * len(self.sizes))()
        for i, r in enumerate(self.recs):
            addr = [d.data_ptr() + 4 * self.at[i] for d in self.dev]
            r.param, r.grad, r.momentum_buf, r.numel, r.group = addr[0], addr[1], addr[2], self.sizes[i], i % self.n_groups
            if self.skip.get(i) == "null grad":
                r.grad = None
            elif self.skip.get(i) == "numel 0":
                r.numel = 0
        return self

    def live(self):
        return [i for i in range(len(self.sizes)) if i not in self.skip]

    def args(self):
        return ctypes.cast(self.recs, ctypes.c_void_p), len(self.sizes)

    def check(self, state):
        _lib.check(_lib.lib().tdrn_amp_check_finite(*self.args(), _lib.ptr(state), _lib.current_stream(DEV)), "tdrn_amp_check_finite")

    def step_scaled(self, hyper, state, zero_grads):
        _lib.check(_lib.lib().tdrn_sgd_step_scaled(*self.args(), _lib.ptr(hyper), self.n_groups, _lib.ptr(state),
                                                   _lib.SGD_ZERO_GRADS if zero_grads else 0, _lib.current_stream(DEV)),
                   "tdrn_sgd_step_scaled")

    def step_plain(self, hyper, zero_grads):
        _lib.check(_lib.lib().tdrn_sgd_step(*self.args(), _lib.ptr(hyper), self.n_groups, _lib.SGD_ZERO_GRADS if zero_grads else 0,
                                            _lib.current_stream(DEV)), "tdrn_sgd_step")

    def want(self, hps, state, zero_grads):
        """the restatement on the host copies -> (p, g, b) flat, and the state after the check"""
        state = A.check_finite([self.view(1, i) for i in self.live()], state)
        out = [h.copy() for h in self.host]
        for i in self.live():
            s = slice(self.at[i], self.at[i] + self.sizes[i])
            out[0][s], out[2][s] = A.sgd_step_scaled(self.view(0, i), self.view(1, i), self.view(2, i), state, **hps[i % self.n_groups])
            if zero_grads:
                out[1][s] = 0.0
        return out, state

    def compare(self, want, what):
        torch.cuda.synchronize()
        for name, d, w in zip("pgb", self.dev, want):
            _same(d, w, "%s: %s" % (what, name))


def _run(pack, hps, state_host, zero_grads, what):
    """check + scaled step on the card and in the restatement; compares the buffers and the state; returns the device state"""
    want, want_state = pack.want(hps, state_host, zero_grads)
    pack.upload()
    state = torch.from_numpy(state_host.copy()).to(DEV)
    pack.check(state)
    pack.step_scaled(_hyper(hps), state, zero_grads)
    pack.compare(want, what)
    _same(state, want_state, what + ": state")
    return state, want


@pytest.mark.parametrize("zero_grads", [False, True], ids=["keep_grads", "zero_grads"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "one_float_off"])
@pytest.mark.parametrize("mode", list(MODES))
def test_scaled_step_at_every_size(mode, off, zero_grads):
    hps = [dict(lr=4e-3, **MODES[mode])]
    pack = Pack(SIZES, [off] * len(SIZES), seed=11)
    pack.host[1] *= 1000.0                                      # gradients of a scaled loss
    assert [(4 * a) % 16 for a in pack.at] == [4 * off] * len(SIZES)
    state, want = _run(pack, hps, A.new_state(1000.0), zero_grads, "%s off %d" % (mode, off))       # a scale that is no power of two
    assert float(state[A.FOUND_INF]) == 0.0
    assert not np.array_equal(_bits(want[0]), _bits(pack.host[0]))                                   # the step moved p


def _two_hundred(seed, skip=True):
    """200 tensors = three launches: tensor 0 spans chunks and has a numel % 4 tail, tensor 1 is off the 16-byte grid, the rest are
    small, every seventh of them off the grid; one record with a null grad and one with numel 0 in each launch's range"""
    sizes = [2 * CHUNK + 7, CHUNK + 1] + [(1, 2, 3, 4, 5, 7, 8, 13, 64, 67, 130, 257)[(5 * i) % 12] for i in range(198)]
    off = [0, 1] + [1 if i % 7 == 3 else 0 for i in range(198)]
    skips = {5: "null grad", 40: "numel 0", 100: "null grad", 120: "numel 0", 195: "numel 0", 199: "null grad"} if skip else {}
    return Pack(sizes, off, seed, n_groups=2, skip=skips)


HPS2 = [dict(lr=4e-3, momentum=0.9, weight_decay=5e-4, nesterov=False), dict(lr=0.05, momentum=0.5, weight_decay=1e-2, nesterov=True)]


@pytest.mark.parametrize("zero_grads", [False, True], ids=["keep_grads", "zero_grads"])
def test_two_hundred_tensors_in_three_launches_with_skipped_records(zero_grads):
    pack = _two_hundred(21)
    assert -(-len(pack.live()) // K) == 3
    pack.host[1] *= 65536.0
    state, want = _run(pack, HPS2, A.new_state(65536.0), zero_grads, "200 tensors")
    assert float(state[A.FOUND_INF]) == 0.0
    for i in pack.skip:                                          # a skipped record keeps p, g and b
        for which in range(3):
            s = slice(pack.at[i], pack.at[i] + pack.sizes[i])
            _same(want[which][s], pack.host[which][s], "skipped record %d" % i)


# (which tensor of the 200, which element): each sits on another path of the check, and tensor 150 in another launch than tensor 0
PLACES = {"first_of_first": (0, 0), "last_of_a_tail": (0, 2 * CHUNK + 6), "last_of_a_whole_chunk": (0, CHUNK - 1),
          "inside_a_misaligned": (1, 2000), "tensor_150": (150, 1)}


@pytest.mark.parametrize("zero_grads", [False, True], ids=["keep_grads", "zero_grads"])
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")], ids=["inf", "-inf", "nan"])
@pytest.mark.parametrize("place", list(PLACES))
def test_one_non_finite_element_stops_every_launch_of_the_step(place, bad, zero_grads):
    pack = _two_hundred(22)
    t, e = PLACES[place]
    assert t not in pack.skip and e < pack.sizes[t]
    pack.view(1, t)[e] = bad
    before = [h.copy() for h in pack.host]
    state, want = _run(pack, HPS2, A.new_state(65536.0), zero_grads, place)
    assert float(state[A.FOUND_INF]) == 1.0
    # spelled out, whatever the restatement says: p and b keep every byte; g is +0 in the live tensors with zero_grads, else kept
    _same(pack.dev[0], before[0], "p after a skipped step")
    _same(pack.dev[2], before[2], "b after a skipped step")
    g = pack.dev[1].cpu().numpy()
    if zero_grads:
        for i in pack.live():
            assert not _bits(g[pack.at[i]:pack.at[i] + pack.sizes[i]]).any(), "gradient %d is not +0" % i
        keep = np.ones(pack.total, bool)
        for i in pack.live():
            keep[pack.at[i]:pack.at[i] + pack.sizes[i]] = False
        _same(g[keep], before[1][keep], "g outside the live tensors")
    else:
        assert np.array_equal(_bits(g), _bits(before[1]))


def test_the_largest_finite_value_and_subnormals_are_finite():
    pack = Pack([CHUNK + 3, 7], [0, 1], seed=31)
    tiny = np.float32(2.0 ** -149)
    for i in range(2):
        g = pack.view(1, i)
        g[0], g[1], g[2], g[3], g[-1] = FLT_MAX, -FLT_MAX, tiny, -3 * tiny, np.float32(2.0 ** -127)
    hps = [dict(lr=4e-3, momentum=0.9, weight_decay=5e-4)]
    state, want = _run(pack, hps, A.new_state(65536.0), False, "FLT_MAX and subnormal gradients")
    assert float(state[A.FOUND_INF]) == 0.0
    assert np.isfinite(want[0]).all() and not np.array_equal(_bits(want[0]), _bits(pack.host[0]))


@pytest.mark.parametrize("zero_grads", [False, True], ids=["keep_grads", "zero_grads"])
def test_scale_one_gives_the_plain_steps_bits(zero_grads):
    packs = [_two_hundred(41).upload() for _ in range(2)]
    hyper = _hyper(HPS2)
    state = _state(1.0)
    packs[0].check(state)
    packs[0].step_scaled(hyper, state, zero_grads)
    packs[1].step_plain(hyper, zero_grads)
    torch.cuda.synchronize()
    for name, a, b in zip("pgb", packs[0].dev, packs[1].dev):
        _same(a, b, "%s: scaled step at scale 1 against tdrn_sgd_step" % name)
    assert not np.array_equal(_bits(packs[1].dev[0]), _bits(packs[1].host[0]))
    _same(state, A.new_state(1.0), "the step writes nothing to the state")


def test_found_inf_is_sticky_until_update():
    bad, good = Pack([CHUNK + 3, 5], [0, 1], seed=51), Pack([CHUNK + 3, 5], [1, 0], seed=52)
    bad.view(1, 1)[4] = np.nan
    bad.upload(), good.upload()
    state = _state(1024.0, good=2.0)
    good.check(state)
    assert state.tolist() == [1024.0, 2.0, 0.0, 0.0]
    bad.check(state)
    assert state.tolist() == [1024.0, 2.0, 1.0, 0.0]
    good.check(state)                                           # a second, finite list (another optimizer's) leaves the flag up
    assert state.tolist() == [1024.0, 2.0, 1.0, 0.0]
    hyper = _hyper([dict(lr=0.1, momentum=0.9)])
    good.step_scaled(hyper, state, False)                       # and that optimizer's step is skipped as well
    good.compare(good.host, "the finite list's step under a raised flag")
    _lib.check(_lib.lib().tdrn_amp_update(_lib.ptr(state), 2.0, 0.5, 2000, _lib.current_stream(DEV)), "tdrn_amp_update")
    assert state.tolist() == [512.0, 0.0, 0.0, 1.0]
    good.check(state)
    assert state.tolist() == [512.0, 0.0, 0.0, 1.0]


@pytest.mark.parametrize("what,scale,found,growth,backoff,interval", A.UPDATE_SEQUENCES, ids=[s[0] for s in A.UPDATE_SEQUENCES])
def test_update_sequences_on_the_device(what, scale, found, growth, backoff, interval):
    state, ref, want = _state(scale), A.new_state(scale), []
    for f in found:
        if f:
            state[A.FOUND_INF].fill_(1.0)                       # what a check would have stored
            ref = A.check_finite([np.array([np.inf], np.float32)], ref)      # (a new array: the ones in `want` stay as they are)
        _lib.check(_lib.lib().tdrn_amp_update(_lib.ptr(state), growth, backoff, interval, _lib.current_stream(DEV)), "tdrn_amp_update")
        ref = A.update(ref, growth, backoff, interval)
        want.append((ref, state.clone()))
    torch.cuda.synchronize()
    for k, (r, got) in enumerate(want):
        _same(got, r, "%s: state after update %d" % (what, k))


# ---- tdrn_amd.amp.GradScaler ----------------------------------------------------------------------------------------------------------

def _params(sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=gen).to(DEV)) for n in sizes]


def test_grad_scaler_drives_the_optimizer_and_follows_the_reference():
    """three iterations through scale / step / update with growth_interval 2: a good step, an overflowing one, a good one"""
    sizes = [5, CHUNK + 1] + [3] * 120                          # two launches; the bad element sits in the second
    hp = dict(lr=4e-3, momentum=0.9, weight_decay=5e-4)
    params = _params(sizes, 61)
    ref_p = [p.detach().cpu().numpy().copy() for p in params]
    ref_b = [np.zeros_like(a) for a in ref_p]
    opt = SGD(params, **hp)
    scaler = GradScaler(init_scale=1024.0, growth_interval=2)
    ref = A.new_state(1024.0)
    gen = torch.Generator().manual_seed(62)
    for it in range(3):
        scale = scaler.get_scale()
        assert scale == float(ref[A.SCALE])
        grads = [(torch.randn(n, generator=gen) * scale).numpy() for n in sizes]
        if it == 1:
            grads[-1][2] = np.inf
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g).to(DEV)
        assert scaler.step(opt) is None
        ref = A.check_finite(grads, ref)
        for i in range(len(sizes)):
            ref_p[i], ref_b[i] = A.sgd_step_scaled(ref_p[i], grads[i], ref_b[i], ref, **hp)
        scaler.update()
        ref = A.update(ref, 2.0, 0.5, 2)
        for i, p in enumerate(params):
            _same(p, ref_p[i], "p %d after iteration %d" % (i, it))
            _same(opt.state[p]["momentum_buffer"], ref_b[i], "b %d after iteration %d" % (i, it))
        _same(scaler._state, ref, "state after iteration %d" % it)
    assert scaler.skipped_steps() == 1 and scaler.get_scale() == 512.0
    loss = torch.full((), 0.5, device=DEV, requires_grad=True)
    scaled = scaler.scale(loss)
    assert scaled.shape == loss.shape and float(scaled.detach()) == 256.0
    scaled.backward()
    assert float(loss.grad) == 512.0                            # autograd differentiates the multiply
    assert torch.equal(scaler.scale(torch.ones(3, device=DEV)), torch.full((3,), 512.0, device=DEV))


def test_state_dict_round_trip_with_torchs_grad_scaler():
    ours = GradScaler(init_scale=4096.0, growth_factor=1.5, backoff_factor=0.25, growth_interval=7).init(DEV)
    ours._state[A.GOOD_STEPS].fill_(3.0)
    d = ours.state_dict()
    assert d == {"scale": 4096.0, "growth_factor": 1.5, "backoff_factor": 0.25, "growth_interval": 7, "_growth_tracker": 3}
    theirs = torch.amp.GradScaler("cuda")
    assert sorted(theirs.state_dict()) == sorted(d)             # the same keys
    theirs.load_state_dict(d)
    back = theirs.state_dict()
    assert back == d
    back.update(scale=128.0, _growth_tracker=5)
    fresh, live = GradScaler(), GradScaler().init(DEV)          # before and after the state exists
    for s in (fresh, live):
        s.load_state_dict(back)
        assert s.get_scale() == 128.0 and s.state_dict() == back
    fresh.init(DEV)
    assert fresh._state.tolist() == [128.0, 5.0, 0.0, 0.0] and live._state.tolist() == [128.0, 5.0, 0.0, 0.0]
    assert GradScaler(enabled=False).state_dict() == {}
    with pytest.raises(RuntimeError):
        live.load_state_dict({})


def test_a_disabled_scaler_passes_everything_through():
    (p,) = _params([CHUNK + 1], 71)
    g = torch.randn(CHUNK + 1, generator=torch.Generator().manual_seed(72))
    p.grad = g.to(DEV)
    want, _ = R.sgd_step(p.detach().cpu().numpy(), g.numpy(), np.zeros(CHUNK + 1, np.float32), lr=0.1)
    opt = SGD([p], lr=0.1)
    scaler = GradScaler(enabled=False)
    loss = torch.ones((), device=DEV)
    assert scaler.scale(loss) is loss
    assert scaler.step(opt) is None
    scaler.update()
    _same(p, want, "p after a step through a disabled scaler")
    assert scaler._state is None and scaler.get_scale() == 1.0 and scaler.skipped_steps() == 0 and not scaler.is_enabled()
    assert scaler.step(torch.optim.SGD([p], lr=0.1), lambda: 2.5) == 2.5      # any optimizer, as torch's disabled scaler


def test_what_the_scaler_refuses():
    (p,) = _params([8], 81)
    p.grad = torch.ones_like(p)
    keep = p.detach().clone()
    scaler = GradScaler()
    with pytest.raises(TypeError, match="tdrn_amd.optim.SGD"):
        scaler.step(torch.optim.SGD([p], lr=0.1))
    with pytest.raises(RuntimeError, match="closure"):
        scaler.step(SGD([p], lr=0.1), lambda: 1.0)
    with pytest.raises(NotImplementedError, match="fused into the SGD step"):
        scaler.unscale_(SGD([p], lr=0.1))
    with pytest.raises(RuntimeError, match="before the first"):
        scaler.update()
    with pytest.raises(NotImplementedError):
        scaler.scale(torch.ones(()))                            # a CPU loss: no CPU path
    _same(p, keep, "p after the refusals")
    for kw in (dict(growth_factor=1.0), dict(backoff_factor=1.0), dict(backoff_factor=0.0), dict(growth_interval=0),
               dict(growth_interval=1 << 24), dict(init_scale=0.0), dict(init_scale=float("inf"))):
        with pytest.raises(ValueError):
            GradScaler(**kw)


def test_step_without_a_scaler_is_the_plain_step():
    sizes = [3, CHUNK + 1, 2 * CHUNK + 5]
    hp = dict(lr=4e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)
    params = _params(sizes, 91)
    gen = torch.Generator().manual_seed(92)
    opt = SGD(params, **hp)
    for i, p in enumerate(params):
        g = torch.randn(sizes[i], generator=gen)
        g[0] = float("inf")                                     # no check, no skip: the plain step lets it through to its element
        want_p, want_b = R.sgd_step(p.detach().cpu().numpy(), g.numpy(), np.zeros(sizes[i], np.float32), **hp)
        p.grad = g.to(DEV)
        opt.step(grad_scaler=None)
        _same(p, want_p, "p %d" % i)
        _same(opt.state[p]["momentum_buffer"], want_b, "b %d" % i)
        p.grad = None
