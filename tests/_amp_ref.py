"""Dynamic loss scaling (tdrn_hip.h section i-m) restated in numpy fp32, on top of the SGD step's restatement (tests/_sgd_ref.py):
the check of the gradients, the scaled step, and the update of the state {scale, good_steps, found_inf, skipped}.

Every line is one fp32 operation per element, rounded on its own: 1 / scale is one division, g * inv one product, and the step
behind them is _sgd_ref.sgd_step unchanged.  tests/test_amp_ref.py pins all of it against torch's CPU primitives.
"""
import numpy as np

import _sgd_ref

SCALE, GOOD_STEPS, FOUND_INF, SKIPPED = range(4)

# the update sequences that test_amp_ref.py runs against torch and test_gpu_amp.py on the device:
# (what, scale, the found_inf of each update in turn, growth, backoff, interval)
UPDATE_SEQUENCES = [
    ("growth at the interval", 65536.0, [0, 0, 0, 0, 0, 0, 0], 2.0, 0.5, 3),
    ("backoff, then the counter restarts", 65536.0, [0, 0, 1, 0, 0, 0, 1, 1, 0], 2.0, 0.5, 3),
    ("a skip one step before the interval", 1024.0, [0, 0, 0, 1, 0, 0, 0, 0], 2.0, 0.5, 4),
    ("interval 1 grows every good step", 8.0, [0, 0, 1, 0], 2.0, 0.5, 1),
    ("factors that are no powers of two", 1000.0, [0, 0, 1, 0, 0, 1, 0, 0], 1.5, 0.75, 2),
    ("a scale that is no power of two", 3.0e4, [0, 1, 0, 0, 1], 1.25, 0.75, 2),
    ("growth that would overflow is refused, the counter restarts", 3.0e38, [0, 0, 0, 0], 2.0, 0.5, 2),
    ("backoff into the subnormal range", 2.0 ** -125, [1, 1, 1, 0], 2.0, 0.5, 5),
]


def new_state(scale=65536.0, good_steps=0):
    return np.array([scale, good_steps, 0, 0], np.float32)


def check_finite(grads, state):
    """grads: the gradient arrays of the records that are not skipped.  Raises found_inf, never lowers it.  Returns the new state."""
    state = state.copy()
    if not all(bool(np.isfinite(g).all()) for g in grads):
        state[FOUND_INF] = 1
    return state


def unscale(g, scale):
    """what the scaled step feeds its four lines"""
    assert g.dtype == np.float32
    with np.errstate(all="ignore"):
        out = g * (np.float32(1) / np.float32(scale))
    assert out.dtype == np.float32
    return out


def sgd_step_scaled(p, g, b, state, lr, momentum=0.0, weight_decay=0.0, nesterov=False):
    """One scaled step on fp32 arrays: the new (p, b); the inputs themselves when the state holds found_inf."""
    if state[FOUND_INF] != 0:
        return p, b
    return _sgd_ref.sgd_step(p, unscale(g, state[SCALE]), b, lr, momentum, weight_decay, nesterov)


def update(state, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    """torch's _amp_update_scale_ in fp32 on the four words.  Returns the new state."""
    scale, good, found, skipped = (np.float32(v) for v in state)
    growth, backoff = np.float32(growth_factor), np.float32(backoff_factor)
    with np.errstate(all="ignore"):
        if found != 0:
            scale, good, skipped = scale * backoff, np.float32(0), skipped + np.float32(1)
        else:
            good = good + np.float32(1)
            if good == np.float32(growth_interval):
                s = scale * growth
                if np.isfinite(s):
                    scale = s
                good = np.float32(0)
    return np.array([scale, good, 0, skipped], np.float32)
