"""SGD in HIP: a drop-in torch.optim.SGD whose step() is one fused multi-tensor launch (tdrn_hip.h section i-j).

    from tdrn_amd.optim import SGD          # instead of torch.optim.SGD; train.py:259-270 and train_trn.py:218-221 stay as they are

Per element, every operation rounded to fp32 on its own:

    d = (wd != 0) ? g + wd*p : g
    if (mom != 0) { b = mom*b + d;  u = nesterov ? d + mom*b : b; } else u = d
    p = p - lr*u

bit for bit and run to run.  Momentum buffers start as zeros, which equals torch's buf = clone(d) except for the sign of a zero.
dampening and maximize are not covered.

The hyper-parameters live in one small device tensor, (groups, 4) rows of {lr, momentum, weight_decay, nesterov}, which the kernel
reads when it runs.  sync_hyper() brings that tensor up to date with param_groups; an eager step() calls it, so the reference's
adjust_learning_rate (it writes param_group['lr']) works unchanged.  A captured step cannot: call sync_hyper() before the capture
and before every replay whose hyper-parameters changed.  The replay then uses the new values.

fp16 training: tdrn_amd.amp.GradScaler.step(optimizer) calls step(grad_scaler=scaler), which checks the gradients for inf / NaN and
runs the same step with the unscale and the skip decided on the device (tdrn_hip.h section i-m).
"""
import array
import ctypes as C

import torch

from . import _lib

_COVERED = "tdrn_amd.optim.SGD covers lr, momentum, weight_decay and nesterov"


def warmup_step_lr(base_lr, gamma, epoch, step_index, iteration, epoch_size, warm_epoch):
    """adjust_learning_rate of train.py:321-326"""
    if epoch <= warm_epoch:
        return 1e-6 + (base_lr - 1e-6) * iteration / (epoch_size * warm_epoch)
    return base_lr * (gamma ** (step_index))


def step_lr(base_lr, gamma, step_index):
    """adjust_learning_rate of train_trn.py:262"""
    return base_lr * (gamma ** (step_index))


class SGD(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 zero_grads=False):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: %r" % (momentum,))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        # the keys of torch.optim.SGD's groups, so that state dicts go both ways; the last three mean nothing here
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=None, differentiable=False, fused=None)
        self.zero_grads = bool(zero_grads)
        self._hyper = None                 # (groups, 4) fp32 on the parameters' device
        self._mirror = None                # what _hyper holds, as host floats
        self._seen = {}                    # parameter -> (its momentum buffer, its address) when both were last checked
        super(SGD, self).__init__(params, defaults)

    def add_param_group(self, param_group):
        super(SGD, self).add_param_group(param_group)
        group = self.param_groups[-1]
        self._check_group(group)
        for p in group["params"]:
            if p.dtype != torch.float32:
                raise TypeError("%s on fp32 parameters only, got %s" % (_COVERED, p.dtype))
            if not p.is_contiguous():
                raise ValueError("tdrn_amd.optim.SGD needs contiguous parameters, got strides %r for shape %r"
                                 % (tuple(p.stride()), tuple(p.shape)))
        self._hyper = self._mirror = None  # one more row

    @staticmethod
    def _check_group(group):
        if group["dampening"] != 0:
            raise ValueError("%s: dampening must be 0, got %r" % (_COVERED, group["dampening"]))
        if group["maximize"]:
            raise ValueError("%s: maximize must be False" % _COVERED)

    def _wanted(self):
        rows = []
        for group in self.param_groups:
            self._check_group(group)
            rows.append([float(group["lr"]), float(group["momentum"]), float(group["weight_decay"]),
                         1.0 if group["nesterov"] else 0.0])
        return rows

    def _device(self):
        for group in self.param_groups:
            for p in group["params"]:
                _lib.require_cuda(p, "a parameter of tdrn_amd.optim.SGD")
                return p.device
        return None

    def sync_hyper(self):
        """Bring the device copy of the hyper-parameters up to date with param_groups: one fill kernel per changed entry, on the
        current stream, in stream order with the steps around it.  No pinned copy, no synchronisation."""
        dev = self._device()
        if dev is None:
            return
        wanted = self._wanted()
        if self._hyper is None or self._hyper.device != dev or len(self._mirror) != len(wanted):
            self._hyper = torch.zeros(len(wanted), 4, dtype=torch.float32, device=dev)
            self._mirror = [[0.0] * 4 for _ in wanted]
        for i, (have, want) in enumerate(zip(self._mirror, wanted)):
            for j in range(4):
                if have[j] != want[j]:
                    self._hyper[i, j].fill_(want[j])
                    have[j] = want[j]

    def _hyper_for_step(self, dev):
        if torch.cuda.is_current_stream_capturing():
            if self._hyper is None or self._hyper.device != dev or self._mirror != self._wanted():
                raise RuntimeError("tdrn_amd.optim.SGD.step() under stream capture: param_groups changed since the last "
                                   "sync_hyper(); call sync_hyper() before the capture (and before a replay whose lr changed)")
        else:
            self.sync_hyper()
        return self._hyper

    def zero_grad(self, set_to_none=True):
        """With zero_grads=True the step has left every gradient zeroed and allocated: nothing to do."""
        if not self.zero_grads:
            super(SGD, self).zero_grad(set_to_none)

    def _new_buffer(self, p, b):
        """the momentum buffer of `p`: made as zeros, or checked once when the caller or a state dict brought it"""
        if b is None:
            return torch.zeros_like(p, memory_format=torch.contiguous_format)
        if b.shape != p.shape or b.dtype != torch.float32 or b.device != p.device or not b.is_contiguous():
            raise ValueError("tdrn_amd.optim.SGD: the momentum buffer of a parameter of shape %r must be a contiguous fp32 tensor "
                             "of that shape on its device" % (tuple(p.shape),))
        return b

    def step(self, closure=None, *, grad_scaler=None):
        """grad_scaler: a tdrn_amd.amp.GradScaler (scaler.step(optimizer) passes itself).  The gradients are then those of the scaled
        loss: they are checked for inf / NaN, all of them before the first launch of the step, and the step divides the scale out
        and writes nothing if the check found one (tdrn_hip.h section i-m).  Without it the step is the plain one."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # The host's share of a step is this loop: per tensor it reads three addresses and checks what can have changed since
        # the last step (the gradient is a new tensor after every backward; the buffer is checked when it is a new object).
        # torch itself refuses a .grad of another shape, dtype or device than its parameter's.
        flat, dev, state, seen = [], None, self.state, self._seen
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("tdrn_amd.optim.SGD does not cover sparse gradients")
                if not g.is_contiguous():
                    with torch.no_grad():
                        g = p.grad = g.contiguous()
                st = state.get(p)
                b = st.get("momentum_buffer") if st is not None else None
                at = p.data_ptr()
                was = seen.get(p)
                if b is None or was is None or was[0] is not b or was[1] != at:     # first step, a loaded state dict, p.data replaced
                    _lib.require_cuda(p, "a parameter of tdrn_amd.optim.SGD")
                    if not p.is_contiguous():
                        raise ValueError("tdrn_amd.optim.SGD needs contiguous parameters")
                    b = state[p]["momentum_buffer"] = self._new_buffer(p, b)
                    seen[p] = (b, at)
                if dev is None:
                    dev = p.device
                elif p.device != dev:
                    raise ValueError("tdrn_amd.optim.SGD needs all parameters on one device")
                flat += (at, g.data_ptr(), b.data_ptr(), p.numel(), gi)
        if not flat:
            return loss
        hyper = self._hyper_for_step(dev)
        # tdrn_sgd_tensor as five 8-byte words (little-endian: group is the low half of the last)
        recs = array.array("q", flat)
        assert recs.itemsize == 8 and C.sizeof(_lib.SgdTensor) == 40
        at, n, flags = recs.buffer_info()[0], len(flat) // 5, _lib.SGD_ZERO_GRADS if self.zero_grads else 0
        with torch.cuda.device(dev):
            if grad_scaler is None:
                _lib.check(_lib.lib().tdrn_sgd_step(at, n, hyper.data_ptr(), len(self.param_groups), flags, _lib.current_stream(dev)),
                           "tdrn_sgd_step")
            else:
                state, stream = grad_scaler.state_for_step(dev).data_ptr(), _lib.current_stream(dev)
                _lib.check(_lib.lib().tdrn_amp_check_finite(at, n, state, stream), "tdrn_amp_check_finite")
                _lib.check(_lib.lib().tdrn_sgd_step_scaled(at, n, hyper.data_ptr(), len(self.param_groups), state, flags, stream),
                           "tdrn_sgd_step_scaled")
        return loss

    def load_state_dict(self, state_dict):
        """Takes torch.optim.SGD's state dict as well; a momentum_buffer of None (torch before its first step) loads as zeros."""
        super(SGD, self).load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
            for p in group["params"]:
                st = self.state.get(p)
                if st is None or "momentum_buffer" not in st:
                    continue
                b = st["momentum_buffer"]
                if b is None:
                    st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                elif b.dtype != torch.float32 or not b.is_contiguous():
                    st["momentum_buffer"] = b.to(torch.float32).contiguous()
        self._hyper = self._mirror = None
