"""scaler.scale(loss).backward() -> scaler.step(opt) -> scaler.update() captured once into a graph, on one stream, over the chain of
test_gpu_amp_underflow.py (tests/_amp_chain.py) with static input, gradient and momentum buffers: the scale, the flag of the check
and both counts live on the device (tdrn_hip.h section i-m), so a replay follows them -- a replay with an inf in the input skips
its step and halves the scale, and the next replay unscales by the halved scale.  The chain's gradient is exact at either scale and
the same at every step, so the reference sequence is the SGD step's restatement (tests/_sgd_ref.py) on the float64 gradient, bit
for bit.  The scale is read on the host only between replays."""
import numpy as np
import pytest
import torch

import _amp_chain as chain
import _sgd_ref as R
from tdrn_amd.amp import GradScaler
from tdrn_amd.optim import SGD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HYPER = dict(lr=0.05, momentum=0.9)


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(a).reshape(-1).view(np.int32)


def test_a_captured_step_follows_the_scale_from_replay_to_replay():
    x, m, w0 = chain.inputs()
    xs, md = x.to(DEV), m.to(DEV)                                # xs: the static input
    w = torch.nn.Parameter(w0.to(DEV))
    opt = SGD([w], zero_grads=True, **HYPER)                     # the step leaves +0 in the static gradient, skipped or not
    w.grad = torch.zeros_like(w)
    opt.state[w]["momentum_buffer"] = torch.zeros_like(w)
    scaler = GradScaler(init_scale=2.0 ** 16)
    scaler.init(DEV)
    opt.sync_hyper()

    def step():
        scaler.scale(chain.loss_of(xs, md, w)).backward()
        scaler.step(opt)
        scaler.update()

    ref_w, ref_b = w0.numpy(), np.zeros(tuple(w0.shape), np.float32)

    def ref_step():
        return R.sgd_step(ref_w, chain.gradient(), ref_b, **HYPER)

    def same(what):
        torch.cuda.synchronize()
        assert np.array_equal(_bits(w), _bits(ref_w)), what + ": the weight"
        assert np.array_equal(_bits(opt.state[w]["momentum_buffer"]), _bits(ref_b)), what + ": the momentum buffer"
        assert not _bits(w.grad).any(), what + ": the static gradient is not +0"

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        step()                                                   # warm-up: every lazy initialisation happens outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    ref_w, ref_b = ref_step()
    same("eager warm-up")
    assert scaler._state.tolist() == [65536.0, 1.0, 0.0, 0.0]

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    same("after the capture, which runs nothing")

    graph.replay()
    ref_w, ref_b = ref_step()
    same("replay, finite")
    assert scaler.get_scale() == 65536.0 and scaler.skipped_steps() == 0

    xs[0, 3, 5, 7] = float("inf")
    graph.replay()
    same("replay with an inf in the input: nothing moves")
    assert scaler.get_scale() == 32768.0 and scaler.skipped_steps() == 1
    assert scaler._state.tolist() == [32768.0, 0.0, 0.0, 1.0]

    xs.copy_(x)
    graph.replay()
    ref_w, ref_b = ref_step()
    same("replay, finite, at the halved scale")
    assert scaler._state.tolist() == [32768.0, 1.0, 0.0, 1.0]
    assert not np.array_equal(_bits(ref_w), _bits(w0.numpy()))
    del graph


def test_the_first_scale_under_capture_asks_for_init():
    loss = torch.ones((), device=DEV, requires_grad=True)
    scaler, ready = GradScaler(), GradScaler().init(DEV)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match=r"scaler\.init\(device\)"):
        with torch.cuda.graph(graph):
            doubled = ready.scale(loss) * 2.0                    # a scaler whose state exists is captured like any other op
            with pytest.raises(RuntimeError, match="between replays"):
                ready.get_scale()                                # but its state is not read on the host under capture
            scaler.scale(loss)
    torch.cuda.synchronize()
    del graph, doubled
    assert scaler._state is None
    assert float(scaler.init(DEV).scale(loss).detach()) == 65536.0       # and outside a capture all is well
