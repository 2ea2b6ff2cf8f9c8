"""Why fp16 training needs loss scaling, and that tdrn_amd.amp.GradScaler gives the lost gradient back, with exact inputs
(tests/_amp_chain.py): without a scaler the conv receives an activation gradient of at most half of fp16's smallest subnormal and
its weight gradient is exactly zero; with GradScaler(init_scale=2^16) the updated weight and momentum buffer equal, bit for bit, the
SGD step's restatement (tests/_sgd_ref.py) on the float64 gradient of the same loss."""
import numpy as np
import pytest
import torch

import _amp_chain as chain
import _amp_ref as A
import _sgd_ref as R
from tdrn_amd.amp import GradScaler
from tdrn_amd.optim import SGD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HYPER = dict(lr=0.05, momentum=0.9)


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(a).reshape(-1).view(np.int32)


def _on_device():
    x, m, w0 = chain.inputs()
    return x.to(DEV), m.to(DEV), torch.nn.Parameter(w0.to(DEV))


def test_without_a_scaler_the_weight_gradient_is_exactly_zero():
    """the loss of signal, documented: the float64 gradient is nonzero in most elements, ours is +0 everywhere"""
    x, m, w = _on_device()
    loss = chain.loss_of(x, m, w)
    loss.backward()
    assert np.count_nonzero(chain.gradient()) > 0 and float(loss) != 0.0
    assert w.grad is not None and w.grad.shape == w.shape
    assert not _bits(w.grad).any(), "%d elements of the weight gradient survived" % np.count_nonzero(_bits(w.grad))


def test_with_the_scaler_the_step_lands_on_the_float64_gradient_bit_for_bit():
    x, m, w = _on_device()
    _, _, w0 = chain.inputs()
    opt = SGD([w], **HYPER)
    scaler = GradScaler(init_scale=2.0 ** 16)
    scaler.scale(chain.loss_of(x, m, w)).backward()
    # the scaled gradient itself is exact: 2^16 times the float64 one
    assert np.array_equal(_bits(w.grad), _bits(chain.gradient() * np.float32(2.0 ** 16)))
    scaler.step(opt)
    scaler.update()
    want_w, want_b = R.sgd_step(w0.numpy(), chain.gradient(), np.zeros(tuple(w0.shape), np.float32), **HYPER)
    assert np.array_equal(_bits(w), _bits(want_w)), "the updated weight"
    assert np.array_equal(_bits(opt.state[w]["momentum_buffer"]), _bits(want_b)), "the momentum buffer"
    assert not np.array_equal(_bits(want_w), _bits(w0.numpy()))
    ref = A.update(A.check_finite([chain.gradient()], A.new_state(2.0 ** 16)))
    assert np.array_equal(_bits(scaler._state), _bits(ref))
    assert scaler.get_scale() == 2.0 ** 16 and scaler.skipped_steps() == 0
    assert scaler.state_dict()["_growth_tracker"] == 1
