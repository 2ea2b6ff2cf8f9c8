"""Caller-owned memory: every C entry that writes a caller's buffer, run on buffers that sit between guard bands.

torch's caching allocator hands out 512-byte-aligned blocks rounded up in size, so the rest of the suite never sees (a) a
kernel's path for an output pointer that is not 16-byte aligned and (b) a store behind the end of an output, a workspace
or the weight blob (it lands in allocator slack).  Here every such buffer is a view into a larger one whose bytes before
and behind it hold a NaN bit pattern no kernel produces (SENTINEL); after the call both bands must still hold it, bit for
bit, outputs the contract says are fully overwritten must hold no sentinel, and every result must have the same bits as
the same call on plain buffers (the geometry alone chooses the arithmetic: no tolerance).

What the guards show is that nothing is WRITTEN outside a buffer; they say nothing about reads.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tdrn_amd import _lib
from tdrn_amd.engine import NetEngine
from tdrn_amd.utils import synth

DEV = "cuda:0"
SENTINEL = 0x7FBADBAD          # a quiet NaN with a payload no kernel computes
GUARD = 4096                   # bytes on either side of a buffer (1 Ki floats)
gpu = pytest.mark.gpu


def _pattern():
    return torch.full((2 * GUARD // 4 + 16,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.uint8)


class Guarded(object):
    """`nbytes` of device memory that start `offset` bytes behind a guard band of GUARD bytes and end right in front of another.
    .t is the buffer (a view of `shape` / `dtype`, or the raw bytes); `init` fills it (for buffers that are accumulated into)."""

    def __init__(self, shape=None, dtype=torch.float32, offset=0, nbytes=None, init=None):
        es = torch.empty((), dtype=dtype).element_size()
        n = int(nbytes) if nbytes is not None else es * int(np.prod(shape))
        total = 2 * GUARD + offset + n
        self.raw = torch.full(((total + 3) // 4,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.uint8)
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        body = self.raw[self.lo:self.hi]
        self.t = body if shape is None else body.view(dtype).view(shape)
        if init is not None:
            self.t.copy_(init)

    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def check(self, what, full=True):
        """both guard bands intact; with `full`, no sentinel word left in the buffer either"""
        torch.cuda.synchronize()
        pat = _pattern()
        head = torch.nonzero(self.raw[:self.lo] != pat[:self.lo]).flatten()
        assert head.numel() == 0, "%s: %d bytes in front of the buffer were written (the nearest %d bytes before it)" % (
            what, head.numel(), self.lo - int(head.max()))
        tail_pat = pat[self.hi % 4:self.hi % 4 + self.raw.numel() - self.hi]
        tail = torch.nonzero(self.raw[self.hi:] != tail_pat).flatten()
        assert tail.numel() == 0, "%s: %d bytes behind the end of the buffer were written (the farthest %d bytes behind it)" % (
            what, tail.numel(), int(tail.max()) + 1)
        if full:
            left = int((self.raw[self.lo:self.hi].view(torch.int32) == SENTINEL).sum())
            assert left == 0, "%s: %d elements of an output that is fully overwritten were never written" % (what, left)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    if torch.equal(g, w):
        return
    diff = torch.nonzero((g != w).flatten()).flatten()
    raise AssertionError("%s: %d of %d elements differ from the aligned run (first flat indices %r)" % (
        what, diff.numel(), g.numel(), diff[:8].tolist()))


# ---------------------------------------------------------------------------------------------
# 1 + 2. whole-network forward: every output at every 4-byte offset, exact workspace and weight blob
# ---------------------------------------------------------------------------------------------
NETS = {   # NetEngine arguments of the five FAMILIES of test_gpu_net.py, and the temporal (TRN) ssd4scale net
    "drn_vgg": dict(model=_lib.DRN_VGGBN, bn=True, multihead=True),
    "drn_mobile": dict(model=_lib.DRN_MOBILENET, multihead=True),
    "refinedet_vgg": dict(model=_lib.REFINEDET_VGG, bn=True, multihead=True, use_refine=True),
    "ssd_vgg": dict(model=_lib.SSD4SCALE_VGG, bn=True),
    "ssd_mobile": dict(model=_lib.SSD4SCALE_MOBILE),
    "trn_mobile": dict(model=_lib.SSD4SCALE_MOBILE, deform=True),
}
NET_CASES = [
    # net, dtype, plan flags, batches.  Every route that writes a caller output runs at an odd batch and at 32; the plans that
    # lay out workspace tails (split-K slabs at small batches, the chained split of conv3x3_pp, TDRN_PLAN_CHAIN partials, the
    # transform-then-sample Y ranges -- two at batch 32 -- and TDRN_PLAN_TS_ONE_RANGE) run at 1, 3 and 32.
    ("drn_vgg", "bf16", 0, (1, 3, 32)),                             # ARM loc 40x40 / 20x20 on head3x3.hip
    ("drn_vgg", "fp16", 0, (3, 32)),
    ("drn_vgg", "fp32", 0, (3, 32)),                                # conv_igemm heads, the gather kernel
    ("drn_vgg", "bf16", _lib.PLAN_NO_HEAD3X3, (3, 32)),             # ... the 40x40 / 20x20 ARM heads on conv_igemm's scalar stores
    ("drn_vgg", "fp16", _lib.PLAN_NO_DEFORM_TS, (3, 32)),           # odm_loc / conf through the gather kernel's out0 / out1
    ("drn_vgg", "bf16", _lib.PLAN_CHAIN, (1, 3, 32)),
    ("drn_vgg", "fp16", _lib.PLAN_TS_ONE_RANGE, (1, 3, 32)),
    ("drn_mobile", "bf16", 0, (3, 32)),
    ("drn_mobile", "fp32", 0, (1,)),
    ("refinedet_vgg", "fp16", 0, (3, 32)),                          # odm heads as 5x5 convs (split-K reduce into the outputs)
    ("ssd_vgg", "bf16", 0, (3, 32)),
    ("ssd_mobile", "fp16", 0, (3, 32)),
    ("ssd_mobile", "fp32", 0, (3, 32)),
    ("trn_mobile", "bf16", 0, (3, 32)),                             # deformable ARM heads fed by ref_loc
    ("trn_mobile", "fp32", 0, (1,)),
]
_SD = {}


def _engine(name, dtype, flags):
    """a NetEngine whose packed weights live in a guarded blob of exactly tdrn_net_weight_bytes"""
    eng = NetEngine(size=320, dtype=dtype, plan_flags=flags, **NETS[name])
    specs = eng.param_specs()
    key = (name, tuple(specs))
    if key not in _SD:
        _SD.clear()
        _SD[key] = synth.synth_state_dict(dict(specs), seed=0)
    sd = _SD[key]
    for pname, _ in specs:
        v = np.ascontiguousarray(sd[pname], np.float32)
        _lib.check(eng.lib.tdrn_net_set_param(eng.handle, pname.encode(), v.ctypes.data_as(C.c_void_p), v.size), pname)
    blob = Guarded(dtype=torch.uint8, nbytes=eng.lib.tdrn_net_weight_bytes(eng.handle))
    _lib.check(eng.lib.tdrn_net_pack_weights(eng.handle, blob.ptr(), blob.hi - blob.lo, _lib.current_stream(DEV)), "pack_weights")
    blob.check("weight blob (pack)", full=False)
    eng.weights, eng.device = blob.t, torch.device(DEV)
    return eng, blob


def _assert_routes(name, dtype, flags, eng):
    """the plan really takes the routes this case is meant to exercise (a later plan change must fail here, not quietly test
    something else)"""
    ops, tens = eng.op_infos(), eng.tensor_infos()
    if name == "trn_mobile":
        return
    # the ARM loc heads at 40x40 and 20x20 (H*W >= 400); in the 16-bit plans without TDRN_PLAN_NO_HEAD3X3 with head3x3.hip's
    # geometry (head3x3_supported): 3x3 / s1 / p1, W <= 64, Cin % 64 == 0, one launch (no split-K)
    arm = [(o, tens[o["in"]]) for o in ops if o["kind"] == "conv" and o["out_kind"] == 1]
    big = [(o, t) for o, t in arm if t[2] * t[3] >= 400]
    assert [t[2:] for _, t in big] == [(40, 40), (20, 20)], [t for _, t in arm]
    if dtype != "fp32" and not flags & _lib.PLAN_NO_HEAD3X3:
        for o, (_, cin, h, w) in big:
            assert o["k"] == 3 and o["stride"] == 1 and o["pad"] == 1 and o["dil"] == 1 and o["splitk"] <= 1, o
            assert cin % 64 == 0 and w <= 64, (cin, h, w)
    if name == "drn_vgg":
        heads = [o for o in ops if o["kind"] == "deform_heads"]
        assert len(heads) == 4
        ts = dtype != "fp32" and not flags & _lib.PLAN_NO_DEFORM_TS
        assert all((o["y"] >= 0) == ts for o in heads), [o["y"] for o in heads]


def _outputs(name, eng, B, k):
    """the net's outputs, each starting k floats behind a 16-byte boundary"""
    P, Cn, fm = eng.num_priors, eng.num_classes, eng.fm
    cfg = eng.cfg
    ssd = cfg.model in (_lib.SSD4SCALE_MOBILE, _lib.SSD4SCALE_VGG)
    o = {"arm_loc": Guarded((B, P, 4), offset=4 * k), "conf": Guarded((B * P, Cn), offset=4 * k)}
    if not ssd:
        o["odm_loc"] = Guarded((B, P, 4), offset=4 * k)
    if cfg.model in (_lib.DRN_VGGBN, _lib.DRN_MOBILENET) or cfg.deform:
        for i, f in enumerate(fm):
            o["offsets%d" % i] = Guarded((B, (8 if cfg.deform else cfg.def_groups) * 18, f, f), offset=4 * k)
    if ssd and not cfg.deform:                     # (the temporal net's loc maps are not an output: its ARM heads are deformable)
        for i, f in enumerate(fm):
            o["loc_maps%d" % i] = Guarded((B, 12, f, f), offset=4 * k)
    return o


def _net_forward(eng, blob, ws, x, outs, ref_loc):
    io = _lib.NetIO()
    io.x, io.batch = x.data_ptr(), x.size(0)
    io.arm_loc = outs["arm_loc"].t.data_ptr()
    io.odm_loc = outs["odm_loc"].t.data_ptr() if "odm_loc" in outs else None
    io.conf = outs["conf"].t.data_ptr()
    for i in range(4):
        if "offsets%d" % i in outs:
            io.offsets[i] = outs["offsets%d" % i].t.data_ptr()
        if "loc_maps%d" % i in outs:
            io.loc_maps[i] = outs["loc_maps%d" % i].t.data_ptr()
        if ref_loc is not None:
            io.ref_loc[i] = ref_loc[i].data_ptr()
    _lib.check(eng.lib.tdrn_net_forward(eng.handle, blob.ptr(), ws.ptr(), ws.hi - ws.lo, C.byref(io), _lib.current_stream(DEV)),
               "tdrn_net_forward")


@gpu
@pytest.mark.parametrize("name,dtype,flags,batches", NET_CASES,
                         ids=["%s-%s-%s-b%s" % (c[0], c[1], c[2], "_".join(map(str, c[3]))) for c in NET_CASES])
def test_net_outputs_any_4_byte_offset_exact_workspace(name, dtype, flags, batches):
    eng, blob = _engine(name, dtype, flags)
    _assert_routes(name, dtype, flags, eng)
    for B in batches:
        x = torch.from_numpy(synth.synth_frames(B, 320, seed=B)).to(DEV)
        ref_loc = None
        if eng.cfg.deform:
            r = np.random.Generator(np.random.PCG64(B))
            ref_loc = [torch.from_numpy((0.5 * r.standard_normal((B, 12, f, f))).astype(np.float32)).to(DEV) for f in eng.fm]
        ws = Guarded(dtype=torch.uint8, nbytes=eng.lib.tdrn_net_workspace_bytes(eng.handle, B))
        want = None
        for k in (0, 1, 2, 3):
            outs = _outputs(name, eng, B, k)
            _net_forward(eng, blob, ws, x, outs, ref_loc)
            tag = "%s %s flags=%d B=%d k=%d" % (name, dtype, flags, B, k)
            for key, g in outs.items():
                g.check("%s %s" % (tag, key))
            ws.check(tag + " workspace", full=False)
            blob.check(tag + " weight blob", full=False)
            if want is None:
                want = {key: g.t.clone() for key, g in outs.items()}
            else:
                for key, g in outs.items():
                    _assert_same_bits(g.t, want[key], "%s %s" % (tag, key))
            del outs
        del ws
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# Engine.forward(out=): validated before any launch; a valid misaligned slice gives the plain call's bits, also behind Detect
# ---------------------------------------------------------------------------------------------
def _small_engine(name, dtype="bf16"):
    eng, _ = _engine(name, dtype, 0)
    return eng


@gpu
def test_engine_out_is_validated_before_any_launch():
    eng = _small_engine("drn_vgg")
    B, P, Cn = 3, eng.num_priors, eng.num_classes
    x = torch.from_numpy(synth.synth_frames(B, 320, seed=1)).to(DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    good = {"arm_loc": torch.zeros((B, P, 4), **f32), "odm_loc": torch.zeros((B, P, 4), **f32), "conf": torch.zeros((B * P, Cn), **f32)}
    big = torch.zeros(2 * B * P * 4, **f32)
    bad = [
        {"arm_loc": good["arm_loc"], "loc": good["odm_loc"]},                                    # unknown key
        {"conf": torch.zeros((B * P, Cn), dtype=torch.float64, device=DEV)},                      # not fp32
        {"conf": torch.zeros((B * P, Cn), dtype=torch.float32)},                                   # not on the input's device
        {"odm_loc": torch.zeros((B, 4, P), **f32).transpose(1, 2)},                                # not contiguous
        {"odm_loc": torch.zeros((B, P - 1, 4), **f32)},                                            # wrong shape
        {"conf": torch.zeros((B, P, Cn), **f32)},                                                  # (B, P, C) instead of (B*P, C)
        {"arm_loc": torch.zeros((B + 1, P, 4), **f32)},                                            # another batch's buffer
        {"arm_loc": big[:B * P * 4].view(B, P, 4), "odm_loc": big[B * P * 4 - 1:2 * B * P * 4 - 1].view(B, P, 4)},   # overlap
    ]
    torch.cuda.synchronize()
    for o in bad:
        sentinel = {k: v.clone() for k, v in good.items()}
        with pytest.raises(ValueError):
            eng.forward(x, out=o)
        torch.cuda.synchronize()
        for k, v in good.items():
            assert torch.equal(v, sentinel[k])                  # nothing ran
    assert int(big.abs().sum()) == 0
    ssd = _small_engine("ssd_mobile")
    with pytest.raises(ValueError):                             # ssd4scale has no odm_loc
        ssd.forward(x, out={"odm_loc": good["odm_loc"]})
    rd = NetEngine(size=320, dtype="bf16", model=_lib.REFINEDET_VGG, bn=True, multihead=True, use_refine=False)
    rd.weights, rd.device = torch.zeros(1, dtype=torch.uint8, device=DEV), torch.device(DEV)   # (never reached: raises first)
    with pytest.raises(ValueError):                             # RefineDet without use_refine has no arm_loc
        rd.forward(x, out={"arm_loc": good["arm_loc"]})


@gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_engine_misaligned_out_then_detect_same_bits(dtype):
    """A sliced (4-byte-aligned) out= view: the plain call's bits, and Detect on it (it copies the 16-byte-read inputs) the plain
    call's detections -- the path stream.py takes with its own output buffers."""
    from tdrn_amd.data import mb_cfg
    from tdrn_amd.layers import Detect, PriorBox
    eng = _small_engine("drn_vgg", dtype)
    B, P, Cn = 3, eng.num_priors, eng.num_classes
    x = torch.from_numpy(synth.synth_frames(B, 320, seed=7)).to(DEV)
    plain = eng.forward(x)
    plain = {k: plain[k].clone() for k in ("arm_loc", "odm_loc", "conf")}
    pri = PriorBox(mb_cfg["VOC_320"]).forward().to(DEV)
    det = Detect(Cn, 0, 200, 0.01, 0.45)
    scale = torch.tensor([500.0, 375.0, 500.0, 375.0])
    want = det.forward(plain["odm_loc"], plain["conf"], pri, arm_loc_data=plain["arm_loc"], scale=scale).clone()
    for k in (1, 2, 3):
        g = {"arm_loc": Guarded((B, P, 4), offset=4 * k), "odm_loc": Guarded((B, P, 4), offset=4 * k),
             "conf": Guarded((B * P, Cn), offset=4 * k)}
        r = eng.forward(x, out={n: v.t for n, v in g.items()})
        for n, v in g.items():
            assert r[n].data_ptr() == v.t.data_ptr()
            v.check("forward(out=) k=%d %s" % (k, n))
            _assert_same_bits(v.t, plain[n], "forward(out=) k=%d %s" % (k, n))
        got = det.forward(r["odm_loc"], r["conf"], pri, arm_loc_data=r["arm_loc"], scale=scale)
        _assert_same_bits(got, want, "Detect behind forward(out=) k=%d" % k)
        for n, v in g.items():
            v.check("Detect k=%d %s (input)" % (k, n))


# ---------------------------------------------------------------------------------------------
# 16-byte-vector entries refuse any other address on the host (TDRN_E_ARG), nothing enqueued
# ---------------------------------------------------------------------------------------------
def test_decode_center_size_refuse_unaligned_pointers_on_the_host():
    """Fake addresses with P = 0: the argument checks run before anything is enqueued, so this needs no GPU."""
    lib = _lib.lib()
    a, u = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 4)
    assert lib.tdrn_decode(a, a, 0, 0.1, 0.2, a, None) == 0
    assert lib.tdrn_center_size(a, 0, a, None) == 0
    for loc, pri, out in ((u, a, a), (a, u, a), (a, a, u)):
        assert lib.tdrn_decode(loc, pri, 0, 0.1, 0.2, out, None) == -1
    assert lib.tdrn_center_size(u, 0, a, None) == -1
    assert lib.tdrn_center_size(a, 0, u, None) == -1


def _priors(P, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    return np.concatenate([r.uniform(0.05, 0.95, (P, 2)), r.uniform(0.02, 0.6, (P, 2))], 1).astype(np.float32)


@gpu
def test_detect_decode_refuse_unaligned_inputs_without_launching():
    lib = _lib.lib()
    B, P, Cn, top_k = 2, 1025, 21, 50
    loc, arm, conf = synth.synth_detect_inputs(B, P, Cn, 6.0, seed=3)
    pri = _priors(P, 3)
    nb = lib.tdrn_detect_workspace_bytes(B, P, Cn, top_k)
    scale_h = (C.c_float * 4)(500.0, 375.0, 500.0, 375.0)
    scale_d = torch.tensor([500.0, 375.0, 500.0, 375.0], device=DEV)
    st = _lib.current_stream(DEV)
    for bad in ("loc", "arm", "priors", "ws"):
        g = {n: Guarded(a.shape, offset=4 if n == bad else 0, init=torch.from_numpy(a)) for n, a in
             (("loc", loc), ("arm", arm), ("priors", pri), ("conf", conf))}
        ws = Guarded(dtype=torch.uint8, nbytes=nb, offset=4 if bad == "ws" else 0)
        out = Guarded((B, Cn, top_k, 5))
        cnt = Guarded((B * Cn,), dtype=torch.int32)
        for fn, sc in ((lib.tdrn_detect, scale_h), (lib.tdrn_detect_dev_scale, _lib.ptr(scale_d))):
            rc = fn(g["loc"].ptr(), g["conf"].ptr(), g["priors"].ptr(), g["arm"].ptr(), sc, B, P, Cn, top_k, 0.01, 0.45, out.ptr(),
                    cnt.ptr(), ws.ptr(), nb, st)
            assert rc == -1, (bad, rc)
        torch.cuda.synchronize()
        assert bool((out.raw.view(torch.int32) == SENTINEL).all()) and bool((cnt.raw.view(torch.int32) == SENTINEL).all())
        ws.check("detect ws (%s refused)" % bad, full=False)
    g = Guarded((P, 4), offset=4, init=torch.from_numpy(pri))
    a = Guarded((P, 4), init=torch.from_numpy(pri))
    o = Guarded((P, 4))
    assert lib.tdrn_decode(g.ptr(), a.ptr(), P, 0.1, 0.2, o.ptr(), st) == -1
    assert lib.tdrn_decode(a.ptr(), g.ptr(), P, 0.1, 0.2, o.ptr(), st) == -1
    assert lib.tdrn_center_size(g.ptr(), P, o.ptr(), st) == -1
    o2 = Guarded((P, 4), offset=4)
    assert lib.tdrn_decode(a.ptr(), a.ptr(), P, 0.1, 0.2, o2.ptr(), st) == -1
    assert lib.tdrn_center_size(a.ptr(), P, o2.ptr(), st) == -1
    torch.cuda.synchronize()
    assert bool((o.raw.view(torch.int32) == SENTINEL).all()) and bool((o2.raw.view(torch.int32) == SENTINEL).all())


@gpu
def test_box_utils_wrappers_copy_unaligned_inputs():
    from tdrn_amd.layers.box_utils import center_size, decode
    P = 1025
    r = np.random.Generator(np.random.PCG64(11))
    loc = torch.from_numpy((0.5 * r.standard_normal((P, 4))).astype(np.float32)).to(DEV)
    pri = torch.from_numpy(_priors(P, 11)).to(DEV)
    want_d = decode(loc, pri, [0.1, 0.2])
    want_c = center_size(want_d)
    for k in (1, 2, 3):
        gl, gp = Guarded((P, 4), offset=4 * k, init=loc), Guarded((P, 4), offset=4 * k, init=pri)
        _assert_same_bits(decode(gl.t, gp.t, [0.1, 0.2]), want_d, "decode k=%d" % k)
        gb = Guarded((P, 4), offset=4 * k, init=want_d)
        _assert_same_bits(center_size(gb.t), want_c, "center_size k=%d" % k)
        for g in (gl, gp, gb):
            g.check("box_utils input k=%d" % k)


# ---------------------------------------------------------------------------------------------
# 2 + 3. standalone entries: exact workspaces, outputs at whole 16-byte offsets, compared with a plain run
# ---------------------------------------------------------------------------------------------
OFFSETS = (4, 8)               # floats: whole 16-byte units (catches stores in front of / behind a buffer, not alignment)


def _plain(shape, dtype=torch.float32, init=None):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    if init is not None:
        t.copy_(init)
    return t


@gpu
@pytest.mark.parametrize("case", [(2, 24, 13, 11, 75, 3, 1, 1, 1, 1), (1, 64, 9, 7, 12, 5, 1, 2, 1, 1), (3, 16, 11, 9, 10, 3, 2, 1, 1, 2)],
                         ids=lambda c: "x".join(map(str, c)))
def test_deform_conv_forward_and_backward_guarded(case):
    N, Cin, H, W, Cout, k, st, pad, dil, G = case
    Ho = (H + 2 * pad - (dil * (k - 1) + 1)) // st + 1
    Wo = (W + 2 * pad - (dil * (k - 1) + 1)) // st + 1
    r = np.random.Generator(np.random.PCG64(N * 100 + Cin))
    x = torch.from_numpy(r.standard_normal((N, Cin, H, W)).astype(np.float32)).to(DEV)
    w = torch.from_numpy((r.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)).to(DEV)
    off = torch.from_numpy((1.5 * r.standard_normal((N, G * 2 * k * k, Ho, Wo))).astype(np.float32)).to(DEV)
    gout = torch.from_numpy(r.standard_normal((N, Cout, Ho, Wo)).astype(np.float32)).to(DEV)
    gi0 = torch.from_numpy(r.standard_normal((N, Cin, H, W)).astype(np.float32)).to(DEV)
    gw0 = torch.from_numpy(r.standard_normal((Cout, Cin, k, k)).astype(np.float32)).to(DEV)
    lib = _lib.lib()
    s = _lib.current_stream(DEV)
    geo = (N, Cin, H, W, Cout)
    args = (k, k, st, st, pad, pad, dil, dil, G)                  # kW, kH, dW, dH, padW, padH, dilationH, dilationW, G
    nf = lib.tdrn_deform_conv_workspace_bytes(N, Cin, H, W, Cout, k, k, st, st, pad, pad, dil, dil, G, _lib.F32)
    nbk = lib.tdrn_deform_conv_backward_workspace_bytes(N, Cin, H, W, Cout, k, k, st, st, pad, pad, dil, dil, G)
    assert nf > 0 and nbk > 0

    def run(out, gi, goff, gw, wsf, wsb):
        _lib.check(lib.tdrn_deform_conv_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(off), _lib.ptr(out), *geo, *args, _lib.F32,
                                                _lib.ptr(wsf), nf, s), "forward")
        _lib.check(lib.tdrn_deform_conv_backward_input(_lib.ptr(x), _lib.ptr(off), _lib.ptr(gout), _lib.ptr(gi), _lib.ptr(goff),
                                                       _lib.ptr(w), *geo, *args, _lib.ptr(wsb), nbk, s), "backward_input")
        _lib.check(lib.tdrn_deform_conv_backward_parameters(_lib.ptr(x), _lib.ptr(off), _lib.ptr(gout), _lib.ptr(gw), *geo, *args,
                                                            0.5, _lib.ptr(wsb), nbk, s), "backward_parameters")
    shapes = {"out": (N, Cout, Ho, Wo), "gi": (N, Cin, H, W), "goff": tuple(off.shape), "gw": (Cout, Cin, k, k)}
    inits = {"gi": gi0, "gw": gw0}
    want = {n: _plain(sh, init=inits.get(n)) for n, sh in shapes.items()}
    run(want["out"], want["gi"], want["goff"], want["gw"], _plain((nf,), torch.uint8), _plain((nbk,), torch.uint8))
    for k4 in OFFSETS:
        g = {n: Guarded(sh, offset=4 * k4, init=inits.get(n)) for n, sh in shapes.items()}
        wsf, wsb = Guarded(dtype=torch.uint8, nbytes=nf), Guarded(dtype=torch.uint8, nbytes=nbk)
        run(g["out"].t, g["gi"].t, g["goff"].t, g["gw"].t, wsf.t, wsb.t)
        for n, v in g.items():
            v.check("deform %s k=%d" % (n, k4))
        wsf.check("deform forward workspace", full=False)
        wsb.check("deform backward workspace", full=False)
        for n in ("out", "goff", "gw"):
            _assert_same_bits(g[n].t, want[n], "deform %s k=%d" % (n, k4))
        # grad_input accumulates with float atomics: its low bits depend on arrival order (tdrn_hip.h (i-b)), as in
        # test_gpu_deform_grad.py::test_reproducibility
        assert float((g["gi"].t - want["gi"]).abs().max()) <= 1e-6 * float(want["gi"].abs().max())


@gpu
@pytest.mark.parametrize("B,P", [(1, 257), (3, 1025)])
def test_detect_guarded(B, P):
    lib = _lib.lib()
    Cn, top_k = 21, 200
    loc, arm, conf = (torch.from_numpy(a).to(DEV) for a in synth.synth_detect_inputs(B, P, Cn, 6.0, seed=P))
    pri = torch.from_numpy(_priors(P, P)).to(DEV)
    nb = lib.tdrn_detect_workspace_bytes(B, P, Cn, top_k)
    scale_h = (C.c_float * 4)(500.0, 375.0, 500.0, 375.0)
    scale_d = torch.tensor([500.0, 375.0, 500.0, 375.0], device=DEV)
    s = _lib.current_stream(DEV)
    for fn, sc in ((lib.tdrn_detect, scale_h), (lib.tdrn_detect_dev_scale, _lib.ptr(scale_d))):
        want_o, want_c = _plain((B, Cn, top_k, 5)), _plain((B * Cn,), torch.int32)
        _lib.check(fn(_lib.ptr(loc), _lib.ptr(conf), _lib.ptr(pri), _lib.ptr(arm), sc, B, P, Cn, top_k, 0.01, 0.45, _lib.ptr(want_o),
                      _lib.ptr(want_c), _lib.ptr(_plain((nb,), torch.uint8)), nb, s), "detect")
        torch.cuda.synchronize()
        assert int(want_c.sum()) > 0
        for k in OFFSETS:
            o, c = Guarded((B, Cn, top_k, 5), offset=4 * k), Guarded((B * Cn,), torch.int32, offset=4 * k)
            ws = Guarded(dtype=torch.uint8, nbytes=nb)
            _lib.check(fn(_lib.ptr(loc), _lib.ptr(conf), _lib.ptr(pri), _lib.ptr(arm), sc, B, P, Cn, top_k, 0.01, 0.45, o.ptr(),
                          c.ptr(), ws.ptr(), nb, s), "detect")
            o.check("detect rows k=%d" % k)
            c.check("detect counts k=%d" % k)
            ws.check("detect workspace k=%d" % k, full=False)
            _assert_same_bits(o.t, want_o, "detect rows k=%d" % k)
            _assert_same_bits(c.t, want_c, "detect counts k=%d" % k)


def _dets(n, seed, normalised=False):
    r = np.random.Generator(np.random.PCG64(seed))
    span = 1.0 if normalised else 300.0
    xy = r.uniform(0, 0.8 * span, (n, 2))
    wh = r.uniform(0.02 * span, 0.2 * span, (n, 2))
    return np.concatenate([xy, xy + wh, r.uniform(0, 1, (n, 1))], 1).astype(np.float32)


def _keep_prefix(keep, num):
    torch.cuda.synchronize()
    n = int(num[0])
    return keep[:n].clone(), n


@gpu
@pytest.mark.parametrize("n", [257, 16385])            # (above 16384 boxes the sort keys live in the workspace)
def test_nms_guarded(n):
    lib = _lib.lib()
    nb = lib.tdrn_nms_workspace_bytes(n)
    s = _lib.current_stream(DEV)
    d = torch.from_numpy(_dets(n, n)).to(DEV)
    dn = torch.from_numpy(_dets(n, n + 1, normalised=True)).to(DEV)

    def both(keep, num, keep2, num2, ws):
        _lib.check(lib.tdrn_nms(_lib.ptr(d), n, 0.45, 0, _lib.ptr(keep), _lib.ptr(num), _lib.ptr(ws), nb, s), "nms")
        _lib.check(lib.tdrn_nms_topk(_lib.ptr(dn), n, 0.45, 0.3, 200, _lib.ptr(keep2), _lib.ptr(num2), _lib.ptr(ws), nb, s), "nms_topk")
    wk, wn, wk2, wn2 = _plain((n,), torch.int32), _plain((1,), torch.int32), _plain((n,), torch.int32), _plain((1,), torch.int32)
    both(wk, wn, wk2, wn2, _plain((nb,), torch.uint8))
    want, wcount = _keep_prefix(wk, wn)
    want2, wcount2 = _keep_prefix(wk2, wn2)
    assert 0 < wcount < n and 0 < wcount2 <= 200
    for k in OFFSETS:
        keep, num = Guarded((n,), torch.int32, offset=4 * k), Guarded((1,), torch.int32, offset=4 * k)
        keep2, num2 = Guarded((n,), torch.int32, offset=4 * k), Guarded((1,), torch.int32, offset=4 * k)
        ws = Guarded(dtype=torch.uint8, nbytes=nb)
        both(keep.t, num.t, keep2.t, num2.t, ws.t)
        for what, g in (("keep", keep), ("keep topk", keep2)):
            g.check("nms %s k=%d" % (what, k), full=False)
        for what, g in (("num", num), ("num topk", num2)):
            g.check("nms %s k=%d" % (what, k))
        ws.check("nms workspace k=%d" % k, full=False)
        got, cnt = _keep_prefix(keep.t, num.t)
        got2, cnt2 = _keep_prefix(keep2.t, num2.t)
        assert cnt == wcount and torch.equal(got, want)
        assert cnt2 == wcount2 and torch.equal(got2, want2)


@gpu
def test_nms_topk_classes_guarded():
    lib = _lib.lib()
    n, ncls, top_k = 257, 21, 200
    r = np.random.Generator(np.random.PCG64(4))
    boxes = torch.from_numpy(_dets(n, 4, normalised=True)[:, :4].copy()).to(DEV)
    logits = r.standard_normal((n, ncls)).astype(np.float32)
    logits[:, 0] += 3.0
    sc = torch.softmax(torch.from_numpy(logits), 1).to(DEV)
    nb = lib.tdrn_nms_topk_classes_workspace_bytes(n, ncls)
    s = _lib.current_stream(DEV)

    def run(keep, num, ws):
        _lib.check(lib.tdrn_nms_topk_classes(_lib.ptr(boxes), _lib.ptr(sc), n, ncls, 1, 0.45, 0.01, top_k, _lib.ptr(keep), _lib.ptr(num),
                                             _lib.ptr(ws), nb, s), "nms_topk_classes")
    wk, wn = _plain((ncls, n), torch.int32), _plain((ncls,), torch.int32)
    run(wk, wn, _plain((nb,), torch.uint8))
    torch.cuda.synchronize()
    assert int(wn[1:].sum()) > 0
    for k in OFFSETS:
        keep, num = Guarded((ncls, n), torch.int32, offset=4 * k), Guarded((ncls,), torch.int32, offset=4 * k)
        ws = Guarded(dtype=torch.uint8, nbytes=nb)
        run(keep.t, num.t, ws.t)
        keep.check("nms_topk_classes keep k=%d" % k, full=False)      # (rows below first_class and slots behind num: not written)
        num.check("nms_topk_classes num k=%d" % k, full=False)
        ws.check("nms_topk_classes workspace k=%d" % k, full=False)
        _assert_same_bits(num.t[1:], wn[1:], "nms_topk_classes num k=%d" % k)
        for c in range(1, ncls):
            m = int(wn[c])
            _assert_same_bits(keep.t[c, :m], wk[c, :m], "nms_topk_classes keep class %d k=%d" % (c, k))


@gpu
def test_decode_center_size_guarded():
    P = 1025
    r = np.random.Generator(np.random.PCG64(8))
    loc = torch.from_numpy((0.5 * r.standard_normal((P, 4))).astype(np.float32)).to(DEV)
    pri = torch.from_numpy(_priors(P, 8)).to(DEV)
    lib = _lib.lib()
    s = _lib.current_stream(DEV)
    wd, wc = _plain((P, 4)), _plain((P, 4))
    _lib.check(lib.tdrn_decode(_lib.ptr(loc), _lib.ptr(pri), P, 0.1, 0.2, _lib.ptr(wd), s))
    _lib.check(lib.tdrn_center_size(_lib.ptr(wd), P, _lib.ptr(wc), s))
    for k in OFFSETS:
        d, c = Guarded((P, 4), offset=4 * k), Guarded((P, 4), offset=4 * k)
        _lib.check(lib.tdrn_decode(_lib.ptr(loc), _lib.ptr(pri), P, 0.1, 0.2, d.ptr(), s))
        _lib.check(lib.tdrn_center_size(d.ptr(), P, c.ptr(), s))
        d.check("decode k=%d" % k)
        c.check("center_size k=%d" % k)
        _assert_same_bits(d.t, wd, "decode k=%d" % k)
        _assert_same_bits(c.t, wc, "center_size k=%d" % k)


def test_prior_box_writes_exactly_its_priors():
    """tdrn_prior_box fills HOST memory: the same guard bands around a numpy buffer (no GPU needed)."""
    lib = _lib.lib()
    fm = (C.c_int * 3)(5, 3, 1)
    steps, mins, maxs = (C.c_double * 3)(8, 16, 32), (C.c_double * 3)(30, 60, 111), (C.c_double * 3)(60, 111, 162)
    arc = (C.c_int * 3)(1, 2, 1)
    ars = (C.c_double * 4)(2, 2, 3, 2)
    P = lib.tdrn_prior_box(3, fm, 320.0, steps, mins, maxs, 3, arc, ars, 1, 1, None)
    assert P == 25 * 4 + 9 * 6 + 1 * 4
    want = np.empty((P, 4), np.float32)
    assert lib.tdrn_prior_box(3, fm, 320.0, steps, mins, maxs, 3, arc, ars, 1, 1, want.ctypes.data_as(C.c_void_p)) == P
    g = GUARD // 4
    for k in OFFSETS:
        buf = np.full(2 * g + k + 4 * P, SENTINEL, np.uint32)
        body = buf[g + k:g + k + 4 * P]
        assert lib.tdrn_prior_box(3, fm, 320.0, steps, mins, maxs, 3, arc, ars, 1, 1, body.ctypes.data_as(C.c_void_p)) == P
        assert (buf[:g + k] == SENTINEL).all() and (buf[g + k + 4 * P:] == SENTINEL).all()
        assert not (body == SENTINEL).any()
        assert np.array_equal(body.view(np.float32).reshape(P, 4).view(np.uint32), want.view(np.uint32))


@gpu
def test_roi_resample_and_ota_similarity_guarded():
    lib = _lib.lib()
    s = _lib.current_stream(DEV)
    r = np.random.Generator(np.random.PCG64(6))
    Cf, Hf, Wf, S, n = 13, 19, 17, 7, 65
    feat = torch.from_numpy(r.standard_normal((Cf, Hf, Wf)).astype(np.float32)).to(DEV)
    x0 = r.integers(0, Wf - 1, n)
    y0 = r.integers(0, Hf - 1, n)
    cells = np.stack([x0, y0, np.minimum(Wf, x0 + r.integers(1, 8, n)), np.minimum(Hf, y0 + r.integers(1, 8, n))], 1).astype(np.int32)
    cd = torch.from_numpy(cells).to(DEV)
    Fd = Cf * S * S
    want_roi = _plain((n, Fd))
    _lib.check(lib.tdrn_roi_resample(_lib.ptr(feat), Cf, Hf, Wf, _lib.ptr(cd), n, S, _lib.ptr(want_roi), s), "roi")
    lens = [1, 4, 2, 3, 1, 5]
    rows = torch.from_numpy(r.standard_normal((sum(lens), 5 + Fd)).astype(np.float32))
    xy = torch.from_numpy(r.uniform(0, 0.6, (sum(lens), 2)).astype(np.float32))
    rows[:, 1:3], rows[:, 3:5] = xy, xy + 0.3
    rows = rows.to(DEV)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).to(DEV)
    bxy = r.uniform(0, 0.6, (n, 2)).astype(np.float32)
    boxes = torch.from_numpy(np.concatenate([bxy, bxy + 0.25], 1)).to(DEV)
    want_b, want_a = _plain((n,)), _plain((n,), torch.int32)
    _lib.check(lib.tdrn_ota_similarity(_lib.ptr(boxes), _lib.ptr(want_roi), n, Fd, _lib.ptr(rows), _lib.ptr(off), len(lens), _lib.ptr(want_b),
                                       _lib.ptr(want_a), s), "sim")
    for k in OFFSETS:
        roi, best, arg = Guarded((n, Fd), offset=4 * k), Guarded((n,), offset=4 * k), Guarded((n,), torch.int32, offset=4 * k)
        _lib.check(lib.tdrn_roi_resample(_lib.ptr(feat), Cf, Hf, Wf, _lib.ptr(cd), n, S, roi.ptr(), s), "roi")
        _lib.check(lib.tdrn_ota_similarity(_lib.ptr(boxes), roi.ptr(), n, Fd, _lib.ptr(rows), _lib.ptr(off), len(lens), best.ptr(), arg.ptr(),
                                           s), "sim")
        roi.check("roi_resample k=%d" % k)
        best.check("ota_similarity best k=%d" % k)
        arg.check("ota_similarity arg k=%d" % k)
        _assert_same_bits(roi.t, want_roi, "roi_resample k=%d" % k)
        _assert_same_bits(best.t, want_b, "ota_similarity best k=%d" % k)
        _assert_same_bits(arg.t, want_a, "ota_similarity arg k=%d" % k)


@gpu
def test_preprocess_guarded():
    lib = _lib.lib()
    s = _lib.current_stream(DEV)
    B, H0, W0, S = 3, 41, 57, 67                                  # (B*3*S*S odd: no whole vector width)
    r = np.random.Generator(np.random.PCG64(2))
    fr = torch.from_numpy(r.integers(0, 256, (B, H0, W0, 3), dtype=np.uint8)).to(DEV)
    mean = (C.c_float * 3)(104.0, 117.0, 123.0)
    want, want8 = _plain((B, 3, S, S)), _plain((B, 3, S, S), torch.uint8)
    _lib.check(lib.tdrn_preprocess(_lib.ptr(fr), B, H0, W0, S, mean, 1, _lib.ptr(want), s), "preprocess")
    _lib.check(lib.tdrn_preprocess_u8(_lib.ptr(fr), B, H0, W0, S, 1, _lib.ptr(want8), s), "preprocess_u8")
    for k in OFFSETS:
        out, out8 = Guarded((B, 3, S, S), offset=4 * k), Guarded((B, 3, S, S), torch.uint8, offset=4 * k)
        _lib.check(lib.tdrn_preprocess(_lib.ptr(fr), B, H0, W0, S, mean, 1, out.ptr(), s), "preprocess")
        _lib.check(lib.tdrn_preprocess_u8(_lib.ptr(fr), B, H0, W0, S, 1, out8.ptr(), s), "preprocess_u8")
        out.check("preprocess k=%d" % k)
        out8.check("preprocess_u8 k=%d" % k, full=False)        # (uint8 values may equal a sentinel byte: compared bitwise below)
        _assert_same_bits(out.t, want, "preprocess k=%d" % k)
        _assert_same_bits(out8.t, want8, "preprocess_u8 k=%d" % k)


# ---------------------------------------------------------------------------------------------
# 4. the training losses (tdrn_hip.h ii-b): tdrn_match, tdrn_multibox_loss_forward / _backward, tdrn_encode
# ---------------------------------------------------------------------------------------------
def _loss_inputs(B, P, Cn, refine):
    import _loss_ref as R
    r = np.random.Generator(np.random.PCG64(100 * B + Cn + (7 if refine else 0)))
    counts = [9, 0, 40][:B]
    targets = R.synth_targets(r, B, 1, 1, max(Cn, 2), counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(truths=t(np.concatenate(targets)), off=t(off), T=int(off[-1]), Tmax=max(counts), pri=t(_priors(P, P + B)),
                arm=t((0.3 * r.standard_normal((B, P, 4))).astype(np.float32)) if refine else None,
                loc=t((0.5 * r.standard_normal((B, P, 4))).astype(np.float32)),
                conf=t((1.5 * r.standard_normal((B, P, Cn))).astype(np.float32)),
                gloss=torch.tensor([0.7, 1.3], device=DEV))


def _loss_calls(d, B, P, Cn, o, only_loc=False):
    """tdrn_match, the forward and the backward on the output buffers o (a dict of tensors), workspaces of exactly the queried size"""
    lib = _lib.lib()
    s = _lib.current_stream(DEV)
    conf = None if only_loc else d["conf"]
    _lib.check(lib.tdrn_match(_lib.ptr(d["truths"]), _lib.ptr(d["off"]), d["T"], d["Tmax"], B, _lib.ptr(d["pri"]), P, _lib.ptr(d["arm"]),
                              0.5, 0.1, 0.2, _lib.ptr(o["loc_t"]), _lib.ptr(o["conf_t"]), _lib.ptr(o["ws_match"]), o["ws_match"].numel(), s),
               "match")
    _lib.check(lib.tdrn_multibox_loss_forward(_lib.ptr(d["loc"]), _lib.ptr(conf), _lib.ptr(o["loc_t"]), _lib.ptr(o["conf_t"]), B, P,
                                              0 if only_loc else Cn, 3, _lib.ptr(o["loss"]), _lib.ptr(o["sel"]), _lib.ptr(o["num_pos"]),
                                              _lib.ptr(o["ws_loss"]), o["ws_loss"].numel(), s), "loss forward")
    _lib.check(lib.tdrn_multibox_loss_backward(_lib.ptr(d["loc"]), _lib.ptr(conf), _lib.ptr(o["loc_t"]), _lib.ptr(o["conf_t"]),
                                               _lib.ptr(o["sel"]), _lib.ptr(o["num_pos"]), _lib.ptr(d["gloss"]), B, P, 0 if only_loc else Cn,
                                               _lib.ptr(o["grad_loc"]), None if only_loc else _lib.ptr(o["grad_conf"]), s), "loss backward")


@gpu
@pytest.mark.parametrize("refine", [False, True], ids=["plain", "refine"])
@pytest.mark.parametrize("B,P,Cn", [(1, 257, 3), (3, 1025, 21)])
def test_loss_entries_guarded(B, P, Cn, refine):
    lib = _lib.lib()
    d = _loss_inputs(B, P, Cn, refine)
    nm = lib.tdrn_match_workspace_bytes(B, P, d["Tmax"])
    assert nm > 0
    shapes = {"loc_t": ((B, P, 4), torch.float32), "conf_t": ((B, P), torch.int32), "sel": ((B, P), torch.uint8),
              "num_pos": ((B,), torch.int32), "loss": ((2,), torch.float32), "grad_loc": ((B, P, 4), torch.float32),
              "grad_conf": ((B, P, Cn), torch.float32)}
    vec16 = ("loc_t", "grad_loc")                  # read / written as 16-byte vectors; the others need their element alignment only
    for only_loc in (False, True):
        nl = lib.tdrn_multibox_loss_workspace_bytes(B, P, 0 if only_loc else Cn)
        assert nl > 0
        want = {n: _plain(sh, dt) for n, (sh, dt) in shapes.items()}
        want.update(ws_match=_plain((nm,), torch.uint8), ws_loss=_plain((nl,), torch.uint8))
        _loss_calls(d, B, P, Cn, want, only_loc)
        torch.cuda.synchronize()
        assert int(want["num_pos"].sum()) > 0 and (only_loc or int((want["sel"] == 2).sum()) > 0)
        for k in OFFSETS:
            g = {n: Guarded(sh, dt, offset=(16 * k if n in vec16 else 2 * k - 1 if n == "sel" else 4 * (k - 3)))
                 for n, (sh, dt) in shapes.items()}                                   # sel at an odd byte, the rest at 4 or 20 bytes
            wsm, wsl = Guarded(dtype=torch.uint8, nbytes=nm), Guarded(dtype=torch.uint8, nbytes=nl)
            o = {n: v.t for n, v in g.items()}
            o.update(ws_match=wsm.t, ws_loss=wsl.t)
            _loss_calls(d, B, P, Cn, o, only_loc)
            tag = "loss B=%d P=%d C=%d %s%s k=%d" % (B, P, Cn, "refine" if refine else "plain", " only_loc" if only_loc else "", k)
            for n, v in g.items():
                partly = n == "sel" or (only_loc and n in ("loss", "grad_conf"))      # (sel: bytes at an odd offset, compared below)
                v.check("%s %s" % (tag, n), full=not partly)
            wsm.check(tag + " match workspace", full=False)
            wsl.check(tag + " loss workspace", full=False)
            for n in shapes:
                if only_loc and n in ("loss", "grad_conf"):
                    continue
                _assert_same_bits(g[n].t, want[n], "%s %s" % (tag, n))
            if only_loc:                           # conf NULL: loss_out[1] and grad_conf are left as they were
                words = g["loss"].t.view(torch.int32)
                assert int(words[1]) == SENTINEL and int(words[0]) != SENTINEL, tag
                assert int(words[0]) == int(want["loss"].view(torch.int32)[0]), tag
                assert bool((g["grad_conf"].t.view(torch.int32) == SENTINEL).all()), tag


@gpu
def test_encode_guarded():
    import _loss_ref as R
    P = 1025
    r = np.random.Generator(np.random.PCG64(12))
    pri = torch.from_numpy(_priors(P, 12)).to(DEV)
    matched = torch.from_numpy(R.synth_targets(r, 1, 1, 1, 21, [P])[0][:, :4].copy()).to(DEV)
    lib = _lib.lib()
    s = _lib.current_stream(DEV)
    want = _plain((P, 4))
    _lib.check(lib.tdrn_encode(_lib.ptr(matched), _lib.ptr(pri), P, 0.1, 0.2, _lib.ptr(want), s))
    for k in OFFSETS:
        o = Guarded((P, 4), offset=4 * k)
        _lib.check(lib.tdrn_encode(_lib.ptr(matched), _lib.ptr(pri), P, 0.1, 0.2, o.ptr(), s))
        o.check("encode k=%d" % k)
        _assert_same_bits(o.t, want, "encode k=%d" % k)
    u = Guarded((P, 4), offset=4)                                  # not a 16-byte address: refused on the host, nothing written
    assert lib.tdrn_encode(_lib.ptr(matched), _lib.ptr(pri), P, 0.1, 0.2, u.ptr(), s) == -1
    torch.cuda.synchronize()
    assert bool((u.raw.view(torch.int32) == SENTINEL).all())


@gpu
@pytest.mark.parametrize("refine", [False, True], ids=["plain", "refine"])
def test_match_clamps_offsets_that_break_the_promise(refine):
    """tdrn_hip.h: 'offsets that break the promise are clamped, never followed out of bounds'.  The truths are a view INSIDE a
    larger NaN-filled allocation, so a read that did follow a bad offset lands in mapped memory and shows as NaN or as a changed
    result, not as a fault."""
    import _loss_ref as R
    lib = _lib.lib()
    s = _lib.current_stream(DEV)
    B, P, counts, Tmax, pad = 3, 1025, [20, 30, 25], 30, 600
    T = sum(counts)
    r = np.random.Generator(np.random.PCG64(21))
    rows = np.concatenate(R.synth_targets(r, B, 1, 1, 21, counts))
    big = torch.full(((T + 2 * pad) * 5,), float("nan"), device=DEV)
    truths = big[pad * 5:(pad + T) * 5].view(T, 5)
    truths.copy_(torch.from_numpy(rows))
    pri = torch.from_numpy(_priors(P, 21)).to(DEV)
    arm = torch.from_numpy((0.3 * r.standard_normal((B, P, 4))).astype(np.float32)).to(DEV) if refine else None
    nb = lib.tdrn_match_workspace_bytes(B, P, Tmax)

    def run(off, loc_t, conf_t, ws):
        off_d = torch.tensor(off, dtype=torch.int32, device=DEV)
        _lib.check(lib.tdrn_match(_lib.ptr(truths), _lib.ptr(off_d), T, Tmax, B, _lib.ptr(pri), P, _lib.ptr(arm), 0.5, 0.1, 0.2,
                                  _lib.ptr(loc_t), _lib.ptr(conf_t), _lib.ptr(ws), nb, s), "match")
        torch.cuda.synchronize()
    want_l, want_c = _plain((B, P, 4)), _plain((B, P), torch.int32)
    run([0, 20, 50, 75], want_l, want_c, _plain((nb,), torch.uint8))
    assert bool(torch.isfinite(want_l).all()) and int((want_c[0] > 0).sum()) > 0
    bad_offsets = {"decreasing": [0, 20, 17, 75], "beyond T_total": [0, 20, T + 150, T + 400],
                   "count above max_truths": [0, 20, 20 + Tmax + 25, 75]}
    for name, off in bad_offsets.items():
        loc_t, conf_t = Guarded((B, P, 4), offset=16), Guarded((B, P), torch.int32, offset=4)
        ws = Guarded(dtype=torch.uint8, nbytes=nb)
        run(off, loc_t.t, conf_t.t, ws.t)
        loc_t.check("match loc_t, truth_off %s" % name)
        conf_t.check("match conf_t, truth_off %s" % name)
        ws.check("match workspace, truth_off %s" % name, full=False)
        assert bool(torch.isfinite(loc_t.t).all()), "truth_off %s: a truth was read from outside the buffer" % name
        assert int(conf_t.t.min()) >= 0 and int(conf_t.t.max()) <= 20, name
        _assert_same_bits(loc_t.t[0], want_l[0], "image 0 loc_t, truth_off %s" % name)
        _assert_same_bits(conf_t.t[0], want_c[0], "image 0 conf_t, truth_off %s" % name)
    assert bool(torch.isnan(big[:pad * 5]).all()) and bool(torch.isnan(big[(pad + T) * 5:]).all())
