"""RefineSSD.forward_train pinned op by op: a recorder of every differentiable-op call of one training step, float64 references of
each call from its OWN recorded inputs and grad_output, and the checker (test helper: device-agnostic, torch and numpy only;
product code never imports it).

Why.  tests/test_gpu_train_net.py compares the whole step with a float64 restatement, which can only be done per tensor and by
relative L2: one flipped ReLU or pool decision shifts every gradient upstream of it.  Here a decision that flips in op k changes the
input of op k + 1, which the reference of op k + 1 shares: every comparison is elementwise, holds at any batch and in any compute
type, and separates kernel error from drift (the rule of test_gpu_pin16.py for the inference engine).

Recorder.  `with Recorder(net) as rec:` replaces conv2d, batch_norm, max_pool2d, l2norm, conv_transpose2d and conv_offset2d of
tdrn_amd.model.networks (forward_train looks them up at call time) by wrappers and restores them on exit.  A wrapper passes every
activation input that requires grad (the offset of conv_offset2d too) through t.view_as(t): a fresh autograd node with this op as
its only consumer, so a hook on it receives this op's own grad_input and not the sum over all consumers of t.  A hook on the output
receives the grad_output the op's backward is given (the sum over the output's consumers).  An input that does not require grad
(the image) gets no hook and no grad_input check.  Kept per call: kind, non-tensor arguments, a clone of every tensor input taken at
call time (the running buffers before the call among them), the parameter objects, the output.  rec.finish(), after loss.backward()
and before anything moves the parameters, reads each parameter's .grad and the running buffers and asserts: every parameter of the
module belongs to exactly one stage; the number of stages of each kind is the number of nn.Conv2d / nn.BatchNorm2d / nn.MaxPool2d /
nn.ConvTranspose2d / L2Norm / ConvOffset2d holders of the module; every hook fired, once; every recorded input but the running
buffers is still bit-equal to its clone (no op wrote into a tensor it was handed or had saved).

References (float64, CPU, from the stage's recorded inputs and grad_output) and bounds -- the per-op files' own, with one change:

  fp32       |got - ref| <= 1e-4 max|ref| per tensor, elementwise, WITHOUT the floor max(1, .) of the per-op files: the gradients
             of this net are 1e-3 and smaller (max|grad_output| at the BatchNorms 6e-4 ... 3.3e-3, at the deformable heads
             7e-5 ... 4e-4: float64 restatement, 192 px, batch 2), so a floor of 1 would make the bound 300 to 10000 times wider
             than what it guards.  The bound is scale-free; the per-op files measure 0.3 to 0.6 % of it at unit scale.  A
             reference that is all zero asks for exact zeros.
  conv2d (stride 1 and 2), conv_transpose2d
             F.conv2d / F.conv_transpose2d with autograd, as tests/_conv_train_harness.py's users; in a 16-bit mode input, weight
             and grad_output are rounded to the type first (the bias is not) and |got - ref| <= C_ACC[mode] S elementwise, S the
             same op on absolute values (_conv_train_harness.compare).
  cancelling bias gradients
             the one cancellation the net contains: the bias of a conv that feeds a training-mode BatchNorm has the gradient
             sum(grad_output), and the BatchNorm backward makes that sum 0 exactly (_train_model_ref.bn_after_conv lists the 17).
             Bound C_ACC["bf16"] S with S = sum|grad_output|: 2e-6 is the project's constant for plain fp32 accumulation noise
             relative to the absolute sum, and a bias sum has no products, so it applies in every mode.
  batch_norm (fused ReLU)
             F.batch_norm in the call's mode.  The ReLU decision is the op's own: mask = (device output > 0).  Asserted first:
             the mask differs from float64's z > 0 only where |z_ref| <= tau = 1e-4 max|y_ref|, and the elements within tau are at
             most 1 % of the stage (a condition, not a measurement: the float64 restatement alone has 2.7e-4 ... 5.2e-4 there).
             Gradients: float64 BN backward of grad_output * mask; no element exempted.  Training: the running buffers after the
             step against float64 from the recorded old buffers, running_mean 1e-5 max(1, |ref|), running_var 1e-5 |ref|
             (test_gpu_batch_norm.py's abs5 / rel5).  Eval: the buffers bit-equal to before.
  max_pool2d test_gpu_max_pool.py::_compare: output bits equal torch's; the saved codes (when the output's grad_fn holds them) give
             torch's indices; grad_input of 2 x 2 / 2 bit-equal to torch's (the inputs are post-ReLU: all-zero windows occur and the
             tie must go where torch sends it); 3 x 3 / 1 / 1 by the fp32 bound.  Nothing exempted.
  l2norm     weight x / (sqrt(sum_c x^2) + eps) with autograd (test_gpu_l2norm.py); asserted: no all-zero pixel in the input.
  conv_offset2d
             backward (fp32 whatever `compute` is) and the fp32 forward: _deform_grad_ref.grads, image by image.  near_decision
             exempts entries of grad_offset only, at most max(2, numel // 1000) of them (asserted).  16-bit forward:
             _deform_gather_ref.gather_ref as test_gpu_deform_gather16.py uses it, |got - ref| <= C_ACC S + extra on every pixel
             that is not `near`, and near.sum() * 10 <= near.size (asserted).

check_stages prints, per stage and tensor, the worst share of its bound before asserting, and takes a selection of stages (a kind,
kinds, an index range or a predicate), as check_stages of test_gpu_pin16.py does.
"""
import collections
import concurrent.futures
import inspect

import numpy as np
import torch
import torch.nn.functional as F

import _deform_gather_ref as G16
import _deform_grad_ref as D
from _conv_train_harness import C_ACC, compare, round_to

KINDS = ("conv2d", "batch_norm", "max_pool2d", "l2norm", "conv_transpose2d", "conv_offset2d")
HOLDERS = {"Conv2d": "conv2d", "BatchNorm2d": "batch_norm", "MaxPool2d": "max_pool2d", "L2Norm": "l2norm",
           "ConvTranspose2d": "conv_transpose2d", "ConvOffset2d": "conv_offset2d"}
ACTIVATIONS, PARAMETERS, BUFFERS = ("input", "offset"), ("weight", "bias"), ("running_mean", "running_var")
CONV_TYPE = ("conv2d", "conv_transpose2d")


def bits_equal(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


class Stage(object):
    """one call of one of the six ops, and after Recorder.finish() everything its backward received and returned"""

    def __init__(self, index, kind, args):
        self.index, self.kind, self.args = index, kind, args        # args: the non-tensor arguments by name, defaults filled in
        self.name = None              # the parameter prefix ("backbone.0", "odm_loc.2"); "max_pool2d.<n>" for a pool
        self.inputs = {}              # role -> clone at call time (activations, parameters, running buffers)
        self.live = {}                # role -> what the op was handed (an activation's view_as node; the parameter / buffer object)
        self.output = self.grad_output = self.code = None
        self.grad_input = {}          # role -> this op's own grad_input, for the activations that require grad
        self.param_grad = {}          # role -> the parameter's .grad after backward (None: no gradient arrived)
        self.param_names = {}         # role -> the parameter's name in the module
        self.buffers_after = {}       # role -> the running buffer after the step
        self.fired = {}               # hook -> how often it fired

    def __repr__(self):
        return "<stage %d %s %s>" % (self.index, self.kind, self.name)


class Recorder(object):
    def __init__(self, module):
        from tdrn_amd.model import networks
        self.module, self.networks, self.stages, self.done, self._saved = module, networks, [], False, {}

    def __enter__(self):
        for kind in KINDS:
            self._saved[kind] = getattr(self.networks, kind)
            setattr(self.networks, kind, self._wrapper(kind, self._saved[kind]))
        return self

    def __exit__(self, *exc):
        for kind, fn in self._saved.items():
            setattr(self.networks, kind, fn)
        self._saved = {}
        return False

    def _hook(self, st, key, role=None):
        st.fired[key] = 0

        def hook(g):
            if self.done:                     # a later torch.autograd.grad on the kept graph records nothing
                return
            st.fired[key] += 1
            if role is None:
                st.grad_output = g.detach().clone()
            else:
                st.grad_input[role] = g.detach().clone()
        return hook

    def _wrapper(self, kind, fn):
        sig = inspect.signature(fn)

        def wrapper(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            named = dict(bound.arguments)
            tensors = ACTIVATIONS + PARAMETERS + BUFFERS
            st = Stage(len(self.stages), kind, {k: v for k, v in named.items() if k not in tensors})
            for role in tensors:
                t = named.get(role)
                if not torch.is_tensor(t):
                    continue
                if role in ACTIVATIONS and t.requires_grad and torch.is_grad_enabled():
                    t = named[role] = t.view_as(t)
                    t.register_hook(self._hook(st, "grad_input." + role, role))
                st.live[role], st.inputs[role] = t, t.detach().clone()
            out = fn(**named)
            if out.requires_grad:
                out.register_hook(self._hook(st, "grad_output"))
            if kind == "max_pool2d":          # the product's backward keeps one uint8 code per output element and nothing else
                codes = [t for t in getattr(out.grad_fn, "saved_tensors", ()) if t.dtype == torch.uint8 and t.shape == out.shape]
                st.code = codes[0] if codes else None
            st.output = out
            self.stages.append(st)
            return out
        return wrapper

    def finish(self):
        """after loss.backward(), before anything moves the parameters: completes the stages and asserts the recorder's four facts"""
        self.done = True
        names = {id(p): n for n, p in self.module.named_parameters()}
        owner, nth = {}, collections.Counter()
        for st in self.stages:
            for role in PARAMETERS:
                p = st.live.get(role)
                if p is None:
                    continue
                assert id(p) in names, "%r: %s is no parameter of the module" % (st, role)
                n = names[id(p)]
                assert n not in owner, "%s is used by stages %d and %d" % (n, owner[n], st.index)
                owner[n] = st.index
                st.param_names[role] = n
                st.param_grad[role] = None if p.grad is None else p.grad.detach().clone()
            for role in BUFFERS:
                if role in st.live:
                    st.buffers_after[role] = st.live[role].detach().clone()
            st.name = st.param_names["weight"].rpartition(".")[0] if "weight" in st.param_names else "%s.%d" % (st.kind, nth[st.kind])
            nth[st.kind] += 1
        missing = sorted(set(names.values()) - set(owner))
        assert not missing, "parameters that no recorded op used: %r" % missing
        holders = collections.Counter(HOLDERS[type(m).__name__] for m in self.module.modules() if type(m).__name__ in HOLDERS)
        assert dict(nth) == dict(holders), "stages per kind %r, holders of the module %r" % (dict(nth), dict(holders))
        for st in self.stages:
            silent = [k for k, n in st.fired.items() if n != 1]
            assert not silent, "%r: hooks that did not fire exactly once: %r" % (st, {k: st.fired[k] for k in silent})
            for role, clone in st.inputs.items():
                if role not in BUFFERS:
                    assert bits_equal(st.live[role], clone), "%r: %s was written to after it was handed to the op" % (st, role)
        return self.stages


# ---- references -----------------------------------------------------------------------------------------------------------------
def _cpu64(t):
    return t.detach().cpu().double()


def _tag(st):
    return "%03d %s %s" % (st.index, st.kind, st.name)


def _param_grad(st, role):
    g = st.param_grad.get(role)
    assert g is not None, "%s: no gradient arrived at %s" % (_tag(st), st.param_names.get(role, role))
    return g


def _fp32(st, name, got, ref, shares):
    shares.append((name, compare(_tag(st), "fp32", name, got, ref, None, floor=0.0)))


def _check_conv(st, cancelling, shares):
    mode, has_bias, need_x = st.args["compute"], "bias" in st.inputs, "input" in st.grad_input
    x, w, go = (round_to(t.detach().cpu().float(), mode).double() for t in (st.inputs["input"], st.inputs["weight"], st.grad_output))
    b = _cpu64(st.inputs["bias"]) if has_bias else None
    a = st.args

    def op(xx, ww, bb):
        if st.kind == "conv2d":
            return F.conv2d(xx, ww, bb, a["stride"], a["padding"], a["dilation"])
        return F.conv_transpose2d(xx, ww, bb, a["stride"])

    def run(xx, ww, bb, gg):
        xx, ww = xx.clone().requires_grad_(need_x), ww.clone().requires_grad_(True)
        bb = None if bb is None else bb.clone().requires_grad_(True)
        y = op(xx, ww, bb)
        wanted = {"grad_input": xx if need_x else None, "grad_weight": ww, "grad_bias": bb}
        keys = [k for k, v in wanted.items() if v is not None]
        res = dict(zip(keys, torch.autograd.grad(y, [wanted[k] for k in keys], gg)))
        res["output"] = y.detach()
        return res

    ref = run(x, w, b, go)
    S = run(x.abs(), w.abs(), None if b is None else b.abs(), go.abs()) if mode != "fp32" else {}
    got = {"output": st.output}
    if need_x:
        got["grad_input"] = st.grad_input["input"]
    got["grad_weight"] = _param_grad(st, "weight")
    if has_bias:
        got["grad_bias"] = _param_grad(st, "bias")
    for name, g in got.items():
        if name == "grad_bias" and st.param_names["bias"] in cancelling:
            s = go.abs().sum((0, 2, 3))
            # mode "bf16" selects the constant 2e-6, whatever the stage's compute type is
            shares.append(("grad_bias (cancelling)", compare(_tag(st) + " cancelling sum, c S in every mode:", "bf16", name, g, ref[name], s)))
        else:
            shares.append((name, compare(_tag(st), mode, name, g, ref[name], S.get(name), floor=0.0)))


def _check_batch_norm(st, shares):
    a = st.args
    training, need_x = bool(a["training"]), "input" in st.grad_input
    x, w, b = _cpu64(st.inputs["input"]).requires_grad_(need_x), _cpu64(st.inputs["weight"]).requires_grad_(True), \
        _cpu64(st.inputs["bias"]).requires_grad_(True)
    rm, rv = (_cpu64(st.inputs[r]).clone() if r in st.inputs else None for r in BUFFERS)
    z = F.batch_norm(x, rm, rv, w, b, training, a["momentum"], a["eps"])          # updates rm and rv in training
    y_ref = F.relu(z) if a["relu"] else z
    got_y, go = _cpu64(st.output), _cpu64(st.grad_output)
    if a["relu"]:
        mask = got_y > 0
        tau = 1e-4 * float(y_ref.detach().abs().max())
        near = z.detach().abs() <= tau
        stray = int(((mask != (z.detach() > 0)) & ~near).sum())
        share = float(near.double().mean())
        print("%s ReLU decisions: %.2e of the elements within tau = %.3e of the kink (cap 1e-2), %d decisions differ, %d of them outside tau"
              % (_tag(st), share, tau, int((mask != (z.detach() > 0)).sum()), stray))
        assert stray == 0, "%s: %d ReLU decisions differ from float64's outside tau" % (_tag(st), stray)
        assert share <= 0.01, "%s: %.2f %% of the elements sit on the ReLU kink" % (_tag(st), 100 * share)
        go = go * mask.double()
    wanted = {"grad_input": x if need_x else None, "grad_weight": w, "grad_bias": b}
    keys = [k for k, v in wanted.items() if v is not None]
    ref = dict(zip(keys, torch.autograd.grad(z, [wanted[k] for k in keys], go)))
    _fp32(st, "output", st.output, y_ref.detach(), shares)
    if need_x:
        _fp32(st, "grad_input", st.grad_input["input"], ref["grad_input"], shares)
    _fp32(st, "grad_weight", _param_grad(st, "weight"), ref["grad_weight"], shares)
    _fp32(st, "grad_bias", _param_grad(st, "bias"), ref["grad_bias"], shares)
    for role, r in zip(BUFFERS, (rm, rv)):
        if r is None:
            continue
        if not training:
            assert bits_equal(st.buffers_after[role], st.inputs[role]), "%s: eval mode changed %s" % (_tag(st), role)
            shares.append((role, 0.0))
            continue
        d = (_cpu64(st.buffers_after[role]) - r).abs()
        assert torch.isfinite(d).all(), "%s %s: non-finite values" % (_tag(st), role)
        bound = 1e-5 * (r.abs().clamp_min(1.0) if role == "running_mean" else r.abs())
        share = float((d / bound).max())
        print("%s %-12s max|d| %.3e  worst share of the bound %.4f" % (_tag(st), role, float(d.max()), share))
        assert share <= 1.0, (_tag(st), role, float(d.max()), share)
        shares.append((role, share))


def _check_max_pool(st, shares):
    a = st.args
    k = a["kernel_size"]
    s, p, ceil = (k if a["stride"] is None else a["stride"]), a["padding"], bool(a["ceil_mode"])
    assert all(isinstance(v, int) for v in (k, s, p)), "%s: square geometries only" % _tag(st)
    need_x = "input" in st.grad_input
    x = _cpu64(st.inputs["input"]).requires_grad_(need_x)
    y, idx = F.max_pool2d(x, k, s, p, ceil_mode=ceil, return_indices=True)
    assert bits_equal(st.output.cpu(), y.detach().float()), "%s: output bits" % _tag(st)
    shares.append(("output", 0.0))
    if st.code is not None:
        Ho, Wo = y.shape[2:]
        c = st.code.cpu().long()
        index = (torch.arange(Ho).view(1, 1, Ho, 1) * s - p + c // k) * x.shape[3] + torch.arange(Wo).view(1, 1, 1, Wo) * s - p + c % k
        assert torch.equal(index, idx), "%s: codes" % _tag(st)
        shares.append(("codes", 0.0))
    if need_x:
        gi, = torch.autograd.grad(y, x, _cpu64(st.grad_output))
        if k == 2:
            assert bits_equal(st.grad_input["input"].cpu(), gi.float()), "%s: grad_input bits" % _tag(st)
            shares.append(("grad_input", 0.0))
        else:
            _fp32(st, "grad_input", st.grad_input["input"], gi, shares)
    print("%s output%s%s bit for bit" % (_tag(st), ", codes" if st.code is not None else "", ", grad_input" if need_x and k == 2 else ""))


def _check_l2norm(st, shares):
    need_x = "input" in st.grad_input
    x, w = _cpu64(st.inputs["input"]).requires_grad_(need_x), _cpu64(st.inputs["weight"]).requires_grad_(True)
    assert bool((x.detach().abs().sum(1) > 0).all()), "%s: the input has an all-zero pixel" % _tag(st)
    y = w.view(1, -1, 1, 1) * (x / (x.pow(2).sum(dim=1, keepdim=True).sqrt() + st.args["eps"]))
    grads = torch.autograd.grad(y, ([x] if need_x else []) + [w], _cpu64(st.grad_output))
    _fp32(st, "output", st.output, y.detach(), shares)
    if need_x:
        _fp32(st, "grad_input", st.grad_input["input"], grads[0], shares)
    _fp32(st, "grad_weight", _param_grad(st, "weight"), grads[-1], shares)


def _check_conv_offset(st, shares):
    a = st.args
    mode, geo = a["compute"], (a["stride"], a["padding"], a["dilation"], a["deform_groups"])
    x, off, w, go = (t.detach().cpu().float() for t in (st.inputs["input"], st.inputs["offset"], st.inputs["weight"], st.grad_output))
    N = x.shape[0]
    per = [D.grads(x[n:n + 1], off[n:n + 1], w, go[n:n + 1], *geo) for n in range(N)]          # image by image: memory
    out, gx, goff = (torch.cat([p[i] for p in per]) for i in range(3))
    gw = sum(p[3] for p in per)
    if mode == "fp32":
        _fp32(st, "output", st.output, out, shares)
    else:
        x16, w16 = G16.round16(x.numpy(), mode), G16.round16(w.numpy(), mode)
        with concurrent.futures.ThreadPoolExecutor(N) as pool:          # image by image, side by side: numpy releases the GIL
            parts = list(pool.map(lambda n: G16.gather_ref(x16[n:n + 1], off.numpy()[n:n + 1], w16, *geo, mode), range(N)))
        ref, S, extra, near = (np.concatenate([p[i] for p in parts]) for i in range(4))
        keep = torch.from_numpy(~near)
        sel = lambda t: torch.as_tensor(t).double().permute(0, 2, 3, 1)[keep]
        err, tol = (sel(_cpu64(st.output)) - sel(ref)).abs(), C_ACC[mode] * sel(S) + sel(extra)
        assert torch.isfinite(err).all(), "%s output: non-finite values" % _tag(st)
        share = float((err / tol.clamp_min(1e-300)).max())
        print("%s %s output      worst error / (c S + extra) %.3e, near %d of %d pixels" % (_tag(st), mode, share, int(near.sum()), near.size))
        assert bool((err <= tol).all()), (_tag(st), mode, "output", share)
        assert near.sum() * 10 <= near.size, "%s: %d of %d pixels near the rejection test's discontinuity" % (_tag(st), int(near.sum()), near.size)
        shares.append(("output", share))
    if "input" in st.grad_input:
        _fp32(st, "grad_input", st.grad_input["input"], gx, shares)
    if "offset" in st.grad_input:
        exempt = torch.cat([D.near_decision(off[n:n + 1], x[n:n + 1].shape, w.shape, *geo) for n in range(N)])
        got = _cpu64(st.grad_input["offset"])
        assert tuple(got.shape) == tuple(goff.shape) and bool(torch.isfinite(got).all()), "%s grad_offset: shape or non-finite values" % _tag(st)
        d, bound = (got - goff).abs(), 1e-4 * float(goff.abs().max())
        bad = d > bound
        n = int((bad & exempt).sum())
        share = float(d[~exempt].max()) / bound if bound > 0 else float(d[~exempt].max() > 0)
        print("%s grad_offset max|d| %.3e  bound %.3e  ratio %.3e, %d of %d entries exempt at a sampling decision (cap %d)"
              % (_tag(st), float(d[~exempt].max()), bound, share, n, got.numel(), max(2, got.numel() // 1000)))
        assert int((bad & ~exempt).sum()) == 0, (_tag(st), "grad_offset", int((bad & ~exempt).sum()), share)
        assert n <= max(2, got.numel() // 1000), (_tag(st), "grad_offset: exempt entries", n)
        shares.append(("grad_offset", share))
    _fp32(st, "grad_weight", _param_grad(st, "weight"), gw, shares)


def check_stage(st, cancelling=()):
    """-> [(tensor, worst share of its bound)]; raises AssertionError at the first tensor outside its bound.  `cancelling`: the names
    of the conv biases in front of a training-mode BatchNorm (_train_model_ref.bn_after_conv), empty in eval mode."""
    shares = []
    if st.kind in CONV_TYPE:
        _check_conv(st, cancelling, shares)
    elif st.kind == "batch_norm":
        _check_batch_norm(st, shares)
    elif st.kind == "max_pool2d":
        _check_max_pool(st, shares)
    elif st.kind == "l2norm":
        _check_l2norm(st, shares)
    else:
        _check_conv_offset(st, shares)
    return shares


def select_stages(stages, select=None):
    """select: None (all), a kind, a collection of kinds, a range of stage indices, or a predicate on a Stage"""
    if select is None:
        return list(stages)
    if isinstance(select, str):
        select = (select,)
    if isinstance(select, range):
        return [st for st in stages if st.index in select]
    if callable(select):
        return [st for st in stages if select(st)]
    return [st for st in stages if st.kind in select]


def check_stages(stages, cancelling=(), select=None, failures=None):
    """checks the selected stages -> {kind: (worst share, stage name, tensor)}.  With `failures` (a dict) a stage outside its bounds is
    entered there as name -> message and the walk goes on (the mutation tests); without, it raises."""
    worst = {}
    chosen = select_stages(stages, select)
    assert chosen, "the selection holds no stage"
    for st in chosen:
        try:
            shares = check_stage(st, cancelling)
        except AssertionError as e:
            if failures is None:
                raise
            failures[st.name] = str(e)
            continue
        for name, share in shares:
            if st.kind not in worst or share > worst[st.kind][0]:
                worst[st.kind] = (share, st.name, name)
    for kind, (share, name, tensor) in sorted(worst.items()):
        print("worst share of a bound, %-16s %.4f (%s %s)" % (kind, share, name, tensor))
    return worst
