"""Child process of tests/test_gpu_conv5x5.py::test_conv5x5_replays_under_graph_capture: the three 5x5 entries captured on one side
stream (no parallel branches), replayed once, compared bit for bit with their eager results, for each compute type named on the
command line.  Started fresh, so that its graphs share no process state with the rest of the suite: on this host stack a
hipGraphLaunch of the engine's two-pipeline graphs has crashed in a process that had captured other graphs before (INTEGRATION.md,
"hipGraphLaunch after the destruction of captured handles").  That isolates the known issue; it does not explain it.  The graphs are
kept until the process ends, as bench.py keeps its own."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

import test_gpu_conv5x5 as G
from _conv_train_harness import NAMES, bits_equal

KEEP_ALIVE = []


def run(mode):
    a = G.Abi("conf_6", mode)
    want = [t.clone() for t in a.all()]
    out, gi = torch.full_like(a.go, float("nan")), torch.full_like(a.x, float("nan"))
    gw, gb = torch.zeros_like(a.w), torch.zeros_like(a.b)

    def work():
        gw.zero_()
        gb.zero_()
        a.forward(out)
        a.backward_input(gi)
        a.backward_parameters(gw, gb)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()                                     # warm-up on the side stream: lazy initialisation happens outside the capture
    side.synchronize()
    for name, p, q in zip(NAMES, want, (out, gi, gw, gb)):
        assert bits_equal(p, q), (mode, name, "side stream")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):     # a capture refuses an allocation by the runtime and any synchronisation
        work()
    out.fill_(float("nan"))
    gi.fill_(float("nan"))
    a.ws.fill_(0xFF)                               # NaN bytes in every type: the entries write what they read on the replay
    graph.replay()
    torch.cuda.synchronize()
    for name, p, q in zip(NAMES, want, (out, gi, gw, gb)):
        assert bits_equal(p, q), (mode, name, "replay")
    KEEP_ALIVE.append((graph, side, a, out, gi, gw, gb))
    print("replayed %s" % mode, flush=True)


if __name__ == "__main__":
    for mode in sys.argv[1:]:
        run(mode)
