"""Experiment: two full batches in flight on two HIP streams (each its own engine + workspace + hipGraph, weights shared), so
that the latency-bound middle of one step (28 small dependent launches, ~0.8 ms, <5 % of the FLOPs) runs under the other
step's trunk.  Prints frames/s for 1 and 2 (and 3) pipelines, interleaved."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from tdrn_amd.data import mb_cfg
from tdrn_amd.engine import GraphedCall, NetEngine
from tdrn_amd.layers import Detect, PriorBox
from tdrn_amd.model.dualrefinedet_vggbn import build_net
from tdrn_amd.utils import synth

dev = torch.device("cuda:0")
B, K = 32, 30
net = build_net("test", 320, 21, 1024, 1, True, True)
net.set_compute_dtype("bf16")
sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)
net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
net.eval()
net.set_plan_flags(int(os.environ.get("FLAGS", "0")))
eng0 = net.engine(dev)
pri = PriorBox(mb_cfg["VOC_320"]).forward().to(dev)
NP = int(sys.argv[1]) if len(sys.argv) > 1 else 3
fns = []
engines, streams, graphs, keep = [eng0], [torch.cuda.Stream(dev) for _ in range(NP)], [], []
for i in range(1, NP):
    e = NetEngine(**dict(net._engine_args, dtype="bf16", plan_flags=int(os.environ.get("FLAGS", "0"))))
    e.share_weights(eng0)
    engines.append(e)
for i in range(NP):
    det = Detect(21, 0, 200, 0.01, 0.45)
    x = torch.from_numpy(synth.synth_frames(B, 320, seed=100 + i)).to(dev)
    def one(xin, e=engines[i], d=det):
        r = e.forward(xin)
        return d.forward(r["odm_loc"], r["conf"], pri, arm_loc_data=r["arm_loc"], scale=[500.0, 375.0, 500.0, 375.0])
    fns.append(one)
    with torch.cuda.stream(streams[i]):
        g = GraphedCall(one, x)
    torch.cuda.synchronize()
    graphs.append(g)

EAGER = os.environ.get("MODE", "graph") == "eager"
def run(np_, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        i = k % np_
        with torch.cuda.stream(streams[i]):
            if EAGER:
                fns[i](graphs[i].inputs[0])
            else:
                graphs[i].graph.replay()
    torch.cuda.synchronize()
    return B * steps / (time.perf_counter() - t0)

for np_ in range(1, NP + 1):
    run(np_, 10)
for rep in range(3):
    print("  ".join("%d in flight: %8.1f frames/s" % (np_, run(np_, K)) for np_ in range(1, NP + 1)), flush=True)
# results identical?
outs = []
for i in range(NP):
    with torch.cuda.stream(streams[i]):
        graphs[i].graph.replay()
torch.cuda.synchronize()
ref = graphs[0].outputs.clone()
with torch.cuda.stream(streams[0]):
    graphs[0].graph.replay()
torch.cuda.synchronize()
print("pipeline 0 output stable under concurrency:", bool(torch.equal(ref, graphs[0].outputs)))
