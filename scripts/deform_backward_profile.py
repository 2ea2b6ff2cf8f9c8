"""Per-set device time per kernel (rocprofv3 --kernel-trace) and TCC_EA0_ATOMIC_sum per kernel (--pmc) of
scripts/deform_backward_bench.py --ours-only runs, apportioned to the (set, batch) runs by dispatch order.

    python scripts/deform_backward_profile.py TRACE_DB PMC_DB EXECS_TRACE EXECS_PMC OUT_JSON
EXECS_*: executions of every op per (set, batch) in that run (warm-up 2 + reps)."""
import json
import sqlite3
import sys

RUNS = [("odm_b8", 16), ("odm_b32", 16), ("trn_b8", 8), ("trn_b32", 8)]     # (run, members) in the bench's order


def per_run(db, execs, value):
    c = sqlite3.connect(db)
    rows = list(c.execute("select name, %s from kernels order by start" % value)) if value == "duration" else None
    if rows is None:
        rows = list(c.execute("select kernel_name, value from counters_collection where counter_name = 'TCC_EA0_ATOMIC_sum' "
                              "order by start"))
    bounds, acc = [], 0
    for _, members in RUNS:
        acc += members * execs
        bounds.append(acc)
    out = {r: {} for r, _ in RUNS}
    gemm = 0
    for name, v in rows:
        short = name.split("(")[0].replace("void ", "")
        if "deform_gemm_kernel" in name:
            gemm += 1
        run = next((RUNS[i][0] for i, b in enumerate(bounds) if max(gemm, 1) <= b), RUNS[-1][0])
        out[run][short] = out[run].get(short, 0.0) + float(v or 0) / execs
    return out


def main():
    trace, pmc, et, ep, dst = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    t = per_run(trace, et, "duration")
    a = per_run(pmc, ep, "pmc")
    res = {}
    for run, _ in RUNS:
        k = {n: {"device_us": round(v / 1e3, 1)} for n, v in sorted(t[run].items(), key=lambda kv: -kv[1])}
        for n, v in a[run].items():
            k.setdefault(n, {})["TCC_EA0_ATOMIC_sum"] = v
        data = k.get("tdrn::deform_bwd_data_kernel<16>", {})
        if "TCC_EA0_ATOMIC_sum" in data and "device_us" in data:
            data["atomic_TBps"] = round(data["TCC_EA0_ATOMIC_sum"] * 64 / (data["device_us"] * 1e-6) / 1e12, 3)
        res[run] = k
    with open(dst, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
