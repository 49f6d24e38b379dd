"""mode="influence" (K7i) next to mode="statistics" on the two shapes of bench_robust_stats.py: 10 000 groups x 1 000 rows x 8
features + intercept (f32) and 1 group x 5M rows x 8 features + intercept (f64), device-resident columns and outputs.
Whole calls, interleaved in one process after WARM warm-up rounds: non-robust statistics, HC3, influence with all outputs, with the
leverage only, with the four interval ends only; ms = mean over REPS rounds of the time between two device events around one call.
Kernel times: run under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python scripts/bench_influence.py`,
then `python scripts/bench_influence.py --stats DIR/.../NAME_kernel_stats.csv` prints the row pass next to K7r's meat kernel under
HC3 with the achieved bytes/s over the row pass's algorithmic bytes: b n (k + 1) read + b n per written output."""
import csv
import json
import os
import sys
import time

import numpy as np

K = 8
SHAPES = [("10k x 1k f32", [1_000] * 10_000, "float32"), ("1 x 5M f64", [5_000_000], "float64")]
INTERVALS = ("mean_lo", "mean_hi", "obs_lo", "obs_hi")


def summarise(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows[r["Name"]] = (int(r["Calls"]), float(r["AverageNs"]))
    for name, sizes, dt in SHAPES:
        ctype = "float" if dt == "float32" else "double"
        b, n = (4 if dt == "float32" else 8), int(np.sum(sizes))
        rowk = [(k, v) for k, v in rows.items() if "k7i_rows_kernel<" + ctype in k]
        meat = [(k, v) for k, v in rows.items() if "k7r_meat_kernel<" + ctype + ", true" in k]
        if not rowk or not meat:
            print(json.dumps({"shape": name, "error": "kernel not in the trace"}))
            continue
        # the process runs the row pass with 11, 1 and 4 outputs equally often: one kernel name, so the trace's mean mixes them;
        # ROWPASS_ONLY=all restricts the process to the eleven-output call, which is what the comparison wants
        (kn, (kc, kns)), (mn, (mc, mns)) = rowk[0], meat[0]
        outs = 11
        bytes_ = b * n * (K + 1) + b * n * outs
        print(json.dumps({"shape": name, "row_pass": kn[:60], "row_pass_calls": kc, "row_pass_us": round(kns / 1e3, 1),
                          "meat_hc3": mn[:60], "meat_calls": mc, "meat_us": round(mns / 1e3, 1), "ratio": round(kns / mns, 3),
                          "row_pass_bytes": bytes_, "row_pass_TBps": round(bytes_ / kns / 1e3, 3)}))


def main():
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from polars_ols_amd._lib import INFLUENCE_FIELDS
    from polars_ols_amd.engine import Engine

    warm, reps = int(os.environ.get("WARM", 5)), int(os.environ.get("REPS", 20))
    only_all = os.environ.get("ROWPASS_ONLY", "") == "all"
    eng = Engine(0)
    time.sleep(2.0)                                           # (let a benchmark process that has just exited finish tearing down)
    for name, sizes, dt in SHAPES:
        tdt = getattr(torch, dt)
        offs = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
        n = int(offs[-1])
        gen = torch.Generator(device="cuda").manual_seed(0)
        cols = [torch.randn(n, device="cuda", generator=gen, dtype=tdt) for _ in range(K)]
        y = sum(cols) + 0.1 * torch.randn(n, device="cuda", generator=gen, dtype=tdt)
        cases = {
            "statistics nonrobust": lambda: eng.least_squares_statistics(y, cols, offs, add_intercept=True),
            "statistics HC3": lambda: eng.least_squares_statistics(y, cols, offs, add_intercept=True, cov_type="HC3"),
            "influence all": lambda: eng.least_squares_influence(y, cols, offs, add_intercept=True, want=INFLUENCE_FIELDS),
            "influence leverage": lambda: eng.least_squares_influence(y, cols, offs, add_intercept=True, want=("leverage",)),
            "influence intervals": lambda: eng.least_squares_influence(y, cols, offs, add_intercept=True, want=INTERVALS),
        }
        if only_all:
            cases = {k: v for k, v in cases.items() if k in ("statistics HC3", "influence all")}
        total = {k: 0.0 for k in cases}
        for rnd in range(warm + reps):
            for key, call in cases.items():
                eng.synchronize()
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call()
                eng.synchronize()
                t1.record()
                t1.synchronize()
                if rnd >= warm:
                    total[key] += t0.elapsed_time(t1)
        base = total["statistics HC3"] / reps
        for key in cases:
            ms = total[key] / reps
            print(json.dumps({"shape": name, "call": key, "ms": round(ms, 4), "vs_hc3": round(ms / base, 3)}), flush=True)
    eng.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--stats":
        summarise(sys.argv[2])
    else:
        main()
