"""tests/_amp_ref.py against torch's own CPU primitives, so that the restatement the GPU tests compare with is torch's arithmetic:
torch._amp_foreach_non_finite_check_and_unscale_ for the check and the unscaled values (bit for bit), torch._amp_update_scale_ for
the update of the scale and the growth tracker.

torch's update multiplies the fp32 scale by the factor as a double and rounds once; the restatement and the kernel multiply two fp32
values.  With a factor that fp32 holds exactly the double product is exact before its one rounding, so the two agree in every bit:
the factors here are such (2, 0.5, 1.5, 0.75, 1.25)."""
import numpy as np
import pytest
import torch

import _amp_ref as A
import _sgd_ref as R


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.int32)


def _grads(seed, sizes=(1, 3, 4, 5, 257)):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen).numpy().copy() for n in sizes]


def _torch_unscale(grads, scale):
    """-> (the unscaled arrays, found_inf) by torch's primitive, with inv_scale = 1 / scale as ONE fp32 division"""
    ts = [torch.from_numpy(g.copy()) for g in grads]
    found = torch.zeros(1)
    inv = torch.ones(1) / torch.tensor([scale], dtype=torch.float32)
    assert np.array_equal(_bits(inv.numpy()), _bits(np.float32(1) / np.float32(scale)))
    torch._amp_foreach_non_finite_check_and_unscale_(ts, found, inv)
    return [t.numpy() for t in ts], float(found)


@pytest.mark.parametrize("scale", [65536.0, 3.0, 1000.0, 1.0, 2.0 ** -3, 7.0e4, 1.0 / 3.0])
def test_unscaled_values_equal_torchs_bit_for_bit(scale):
    grads = _grads(1)
    tiny = np.float32(2.0 ** -149)
    # subnormal gradients, subnormal quotients, the largest finite value and zeros of both signs
    grads.append(np.array([tiny, -tiny, 3 * tiny, 2.0 ** -127, -2.0 ** -130, 2.0 ** -126, 1e-38, 0.0, -0.0,
                           np.finfo(np.float32).max, -np.finfo(np.float32).max, 1.0, -65504.0], np.float32))
    want, found = _torch_unscale(grads, scale)
    assert found == 0.0
    state = A.check_finite(grads, A.new_state(scale))
    assert state[A.FOUND_INF] == 0 and state[A.SCALE] == np.float32(scale)
    for g, w in zip(grads, want):
        assert np.array_equal(_bits(A.unscale(g, scale)), _bits(w))      # (FLT_MAX / a scale below 1 is inf in both)


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("where", [(0, 0), (2, 3), (4, 256)])
def test_check_agrees_with_torchs_and_is_sticky(bad, where):
    grads = _grads(2)
    grads[where[0]][where[1]] = bad
    _, found = _torch_unscale(grads, 4.0)
    assert found == 1.0
    state = A.check_finite(grads, A.new_state(4.0))
    assert state[A.FOUND_INF] == 1
    again = A.check_finite(_grads(3), state)                 # a finite list does not lower the flag
    assert again[A.FOUND_INF] == 1
    assert A.check_finite([], A.new_state())[A.FOUND_INF] == 0


def test_scaled_step_is_the_plain_step_on_the_unscaled_gradient_or_nothing():
    p, g, b = (a for a in _grads(4, (300, 300, 300)))
    hp = dict(lr=4e-3, momentum=0.9, weight_decay=5e-4, nesterov=True)
    state = A.new_state(3.0)
    (want_g,), _ = _torch_unscale([g], 3.0)
    got, want = A.sgd_step_scaled(p, g, b, state, **hp), R.sgd_step(p, want_g, b, **hp)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    state[A.FOUND_INF] = 1
    kept = A.sgd_step_scaled(p, g, b, state, **hp)
    assert kept[0] is p and kept[1] is b


def _torch_update(scale, tracker, found, growth, backoff, interval):
    s, t = torch.tensor([scale], dtype=torch.float32), torch.tensor([tracker], dtype=torch.int32)
    torch._amp_update_scale_(s, t, torch.tensor([found], dtype=torch.float32), growth, backoff, interval)
    return s.numpy()[0], int(t)


SEQUENCES = A.UPDATE_SEQUENCES


@pytest.mark.parametrize("what,scale,found,growth,backoff,interval", SEQUENCES, ids=[s[0] for s in SEQUENCES])
def test_update_follows_torchs_amp_update_scale(what, scale, found, growth, backoff, interval):
    state = A.new_state(scale)
    t_scale, t_tracker, skipped = np.float32(scale), 0, 0
    for k, f in enumerate(found):
        state[A.FOUND_INF] = f
        state = A.update(state, growth, backoff, interval)
        t_scale, t_tracker = _torch_update(t_scale, t_tracker, float(f), growth, backoff, interval)
        skipped += f
        assert np.array_equal(_bits(state[A.SCALE:A.SCALE + 1]), _bits(np.float32(t_scale))), (what, k)
        assert state[A.GOOD_STEPS] == t_tracker and state[A.FOUND_INF] == 0 and state[A.SKIPPED] == skipped, (what, k)
    assert state.dtype == np.float32


def test_scale_3e38_with_growth_2_stays_with_the_tracker_at_zero():
    assert _torch_update(3.0e38, 0, 0.0, 2.0, 0.5, 1) == (np.float32(3.0e38), 0)
    state = A.update(A.new_state(3.0e38), 2.0, 0.5, 1)
    assert state[A.SCALE] == np.float32(3.0e38) and state[A.GOOD_STEPS] == 0 and state[A.SKIPPED] == 0
