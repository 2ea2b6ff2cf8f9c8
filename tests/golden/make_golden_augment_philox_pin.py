"""Record tests/golden/augment_philox_pin.npz: what tdrn_augment_sample and tdrn_augment_pair_sample return from Philox
draws for the fixed input of tests/test_gpu_augment_philox_pin.py.  Needs an MI355X and the built library.

    python tests/golden/make_golden_augment_philox_pin.py [DIR] [--search N]   # writes the fixture next to this file (or into DIR)

This is a recording of the library's own output, not of the reference: it was made at the commit before the single-frame
and pair kernels were merged into one F-frame chain, and exists so that a rewrite of the samplers' lane-parallel crop trials
has bytes to be compared with.  Re-record it only with a change that is meant to alter the Philox path (draw slots, the
trial-to-lane mapping), and say so there.  The suite does not run this script.

The inputs and the calls are test_gpu_augment_philox_pin's own (sample_single, sample_pair): _ragged(17, SEED, supplied),
sample ids 40..56, Philox seed SEED.  Everything is recorded twice and written only when the two recordings agree byte for
byte.  The seed must give at least one cropped image in every recording and a pair with two or more translation attempts;
--search N tries SEED, SEED + 1, ... and reports the first that does (then set SEED in the test module to it).

Stored: seed; single_params (17, 80) uint8, single_offsets (18,) int32, single_rows (offsets[-1], 5) fp32; and for
pair_translated_ (no second frames: a translation is drawn) and pair_supplied_ (second frames and truths given): params
(17, 112) uint8, offsets, rows and rows_t."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_gpu_augment_philox_pin as T  # noqa: E402
from tdrn_amd.utils.augmentations import pair_params_to_dicts, params_to_dicts  # noqa: E402


def record(seed):
    out = {"seed": np.int64(seed)}
    _, params, _, pin = T.sample_single(seed)
    ok = any(p["cropped"] == 1 for p in params_to_dicts(params))
    out.update({"single_" + k: v for k, v in pin.items()})
    for supplied, prefix in ((False, "pair_translated_"), (True, "pair_supplied_")):
        _, _, params, _, _, pin = T.sample_pair(supplied, seed)
        ps = pair_params_to_dicts(params)
        ok = ok and any(p["cropped"] == 1 for p in ps) and (supplied or any(p["attempts"] >= 2 for p in ps))
        out.update({prefix + k: v for k, v in pin.items()})
    return out, ok


def main():
    args = sys.argv[1:]
    search = 1
    if "--search" in args:
        i = args.index("--search")
        search = int(args[i + 1])
        del args[i:i + 2]
    out_dir = args[0] if args else HERE
    for seed in range(T.SEED, T.SEED + search):
        first, ok = record(seed)
        if ok:
            break
        print("seed %d: no cropped image or no second translation attempt" % seed)
    else:
        raise SystemExit("no seed in [%d, %d) meets the conditions" % (T.SEED, T.SEED + search))
    second, _ = record(seed)
    assert first.keys() == second.keys()
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), "%s differs between two recordings: not written" % k
    path = os.path.join(out_dir, "augment_philox_pin.npz")
    np.savez_compressed(path, **first)
    print("seed %d -> %s (%d bytes), rows %d / %d / %d" % (seed, path, os.path.getsize(path), len(first["single_rows"]),
                                                           len(first["pair_translated_rows"]), len(first["pair_supplied_rows"])))


if __name__ == "__main__":
    main()
