"""Dynamic loss scaling for fp16 training: torch.cuda.amp.GradScaler's interface on the kernels of tdrn_hip.h section (i-m).

    from tdrn_amd.amp import GradScaler
    from tdrn_amd.optim import SGD

    scaler = GradScaler()                      # torch's arguments and defaults
    out = net.forward_train(x, "fp16", resident=True)
    scaler.scale(loss).backward()              # the gradients of loss * scale: fp16 activation gradients stay above 2^-24
    scaler.step(optimizer)                     # checks them for inf / NaN, then the SGD step with g / scale; skipped on the device
    scaler.update()                            # halves the scale after a skipped step, doubles it after growth_interval good ones

The scale, the flag of the check, the count of good steps and the count of skipped ones are four fp32 words on the device
({scale, good_steps, found_inf, skipped}); the kernels read and write them when they run.  Nothing above reads them on the host, so
the three lines can be captured into one graph, and a replay follows the scale as it follows the learning rate (optim.SGD).  The
state is made by the first scale() on the loss's device; that allocates and copies, so before a capture call scaler.init(device).

Unscaling is fused into the step: there is no unscale_(), hence no gradient clipping between the two.  One scale for all groups.
bf16 has fp32's exponent range and needs none of this.
"""
import math

import torch

from . import _lib
from .optim import SGD

SCALE, GOOD_STEPS, FOUND_INF, SKIPPED = range(4)         # the words of the state (tdrn_hip.h section i-m)


class GradScaler(object):
    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        self._enabled = bool(enabled)
        self._check(init_scale, growth_factor, backoff_factor, growth_interval)
        self._init_scale, self._init_growth_tracker = float(init_scale), 0
        self._growth_factor, self._backoff_factor = float(growth_factor), float(backoff_factor)
        self._growth_interval = int(growth_interval)
        self._state = None                 # (4,) fp32 on the device
        self._scale = None                 # its first word, as a (1,) and as a 0-dim view

    @staticmethod
    def _check(scale, growth_factor, backoff_factor, growth_interval):
        if not (scale > 0.0 and math.isfinite(scale)):
            raise ValueError("GradScaler: the scale must be positive and finite, got %r" % (scale,))
        if not growth_factor > 1.0:
            raise ValueError("GradScaler: growth_factor must be above 1, got %r" % (growth_factor,))
        if not 0.0 < backoff_factor < 1.0:
            raise ValueError("GradScaler: backoff_factor must lie inside (0, 1), got %r" % (backoff_factor,))
        if not 1 <= growth_interval < (1 << 24):
            raise ValueError("GradScaler: growth_interval must lie in [1, 2^24), got %r" % (growth_interval,))

    def is_enabled(self):
        return self._enabled

    def init(self, device):
        """Make the device state now.  The first scale() does it by itself, except under stream capture: there, call this first."""
        device = torch.device(device)
        if device.type != "cuda":
            raise NotImplementedError("tdrn_amd.amp.GradScaler keeps its state on the GPU, got device %r (no CPU path)" % (device,))
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("tdrn_amd.amp.GradScaler.init() under stream capture: it allocates and copies; call it before the capture")
        if self._state is None or self._state.device != device:
            old = self._host_state() if self._state is not None else [self._init_scale, float(self._init_growth_tracker), 0.0, 0.0]
            self._state = torch.tensor(old, dtype=torch.float32, device=device)
            assert self._state.data_ptr() % 16 == 0
            self._scale = (self._state[0:1], self._state[0])
        return self

    def _ready(self, device, what):
        if self._state is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("tdrn_amd.amp.GradScaler.%s under stream capture before the state exists: call scaler.init(device) "
                                   "before the capture" % what)
            self.init(device)
        elif self._state.device != device:
            raise ValueError("tdrn_amd.amp.GradScaler: the state lives on %s, %s came with %s" % (self._state.device, what, device))
        return self._state

    def scale(self, loss):
        """loss * scale, a device multiply that autograd differentiates: the scale is read when the multiply runs."""
        if not self._enabled:
            return loss
        _lib.require_cuda(loss, "the loss given to tdrn_amd.amp.GradScaler.scale()")
        self._ready(loss.device, "scale()")
        return loss * self._scale[0 if loss.dim() else 1]

    def state_for_step(self, device):
        """the state tensor, for optim.SGD.step(grad_scaler=self)"""
        return self._ready(device, "step()")

    def step(self, optimizer, closure=None):
        if not self._enabled:
            return optimizer.step() if closure is None else optimizer.step(closure)
        if not isinstance(optimizer, SGD):
            raise TypeError("tdrn_amd.amp.GradScaler.step() drives tdrn_amd.optim.SGD only (the unscale is fused into its kernel), "
                            "got %s" % type(optimizer).__name__)
        if closure is not None:
            raise RuntimeError("tdrn_amd.amp.GradScaler.step() does not take a closure: the loss must be scaled before its backward")
        return optimizer.step(grad_scaler=self)

    def unscale_(self, optimizer):
        raise NotImplementedError("tdrn_amd.amp.GradScaler has no unscale_(): unscaling is fused into the SGD step's kernel.")

    def update(self):
        """After the step(s) of an iteration: one launch on the current stream (tdrn_amp_update)."""
        if not self._enabled:
            return
        if self._state is None:
            raise RuntimeError("tdrn_amd.amp.GradScaler.update() before the first scale(), step() or init()")
        dev = self._state.device
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().tdrn_amp_update(self._state.data_ptr(), self._growth_factor, self._backoff_factor,
                                                  self._growth_interval, _lib.current_stream(dev)), "tdrn_amp_update")

    def _host_state(self):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("tdrn_amd.amp.GradScaler: reading the state on the host synchronises and cannot be captured; read "
                               "it between replays")
        return self._state.tolist()

    def get_scale(self):
        """The scale as a host float.  Synchronises with the device; not under capture."""
        if not self._enabled:
            return 1.0
        return self._init_scale if self._state is None else self._host_state()[SCALE]

    def skipped_steps(self):
        """How many updates followed a skipped step.  Synchronises with the device; not under capture."""
        return 0 if not self._enabled or self._state is None else int(self._host_state()[SKIPPED])

    def get_growth_factor(self):
        return self._growth_factor

    def get_backoff_factor(self):
        return self._backoff_factor

    def get_growth_interval(self):
        return self._growth_interval

    def state_dict(self):
        """torch.amp.GradScaler's keys, so that checkpoints move both ways.  Synchronises with the device."""
        if not self._enabled:
            return {}
        host = self._host_state() if self._state is not None else [self._init_scale, self._init_growth_tracker]
        return {"scale": host[SCALE], "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": int(host[GOOD_STEPS])}

    def load_state_dict(self, state_dict):
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of GradScaler.")
        scale, tracker = float(state_dict["scale"]), int(state_dict["_growth_tracker"])
        self._check(scale, state_dict["growth_factor"], state_dict["backoff_factor"], state_dict["growth_interval"])
        if not 0 <= tracker < (1 << 24):
            raise ValueError("GradScaler: _growth_tracker must lie in [0, 2^24), got %r" % (tracker,))
        self._init_scale, self._init_growth_tracker = scale, tracker
        self._growth_factor, self._backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        if self._state is not None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("tdrn_amd.amp.GradScaler.load_state_dict() under stream capture")
            self._state[SCALE].fill_(scale)
            self._state[GOOD_STEPS].fill_(float(tracker))
