"""mode="statistics" with cluster-robust standard errors (K7c) next to the non-robust and HC1 calls on the shapes of
bench_robust_stats.py: 10 000 groups x 1 000 rows x 8 features + intercept (f32, 20 clusters per group, ids sorted inside every
group or shuffled) and 1 group x 5M rows x 8 features + intercept (f64, 5 000 firms interleaved by date: one-way by firm, two-way by
firm and date).  Device-resident columns and outputs; each figure is the mean of REPS calls between two device events after WARM
calls.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python scripts/bench_cluster_stats.py`.  One JSON line per case."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polars_ols_amd.engine import Engine  # noqa: E402

WARM, REPS = int(os.environ.get("WARM", 5)), int(os.environ.get("REPS", 20))

eng = Engine(0)
time.sleep(2.0)                                               # (let a benchmark process that has just exited finish tearing down)
k = 8


def frame(sizes, dt):
    offs = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
    n = int(offs[-1])
    gen = torch.Generator(device="cuda").manual_seed(0)
    cols = [torch.randn(n, device="cuda", generator=gen, dtype=dt) for _ in range(k)]
    y = sum(cols) + 0.1 * torch.randn(n, device="cuda", generator=gen, dtype=dt)
    return offs, n, y, cols


def shapes():
    offs, n, y, cols = frame([1_000] * 10_000, torch.float32)
    row = torch.arange(n, device="cuda", dtype=torch.int64)
    sorted_ids = (row % 1_000) // 50                           # 20 clusters of 50 rows, sorted inside every group
    gen = torch.Generator(device="cuda").manual_seed(1)
    shuffled = torch.randint(0, 20, (n,), device="cuda", generator=gen, dtype=torch.int64)
    yield "10k x 1k f32", offs, y, cols, [("nonrobust", None), ("HC1", None), ("cluster sorted", sorted_ids),
                                          ("cluster shuffled", shuffled)]
    offs, n, y, cols = frame([5_000_000], torch.float64)
    row = torch.arange(n, device="cuda", dtype=torch.int64)
    firm, date = row % 5_000, row // 5_000                    # a panel stored date by date
    yield "1 x 5M f64", offs, y, cols, [("nonrobust", None), ("HC1", None), ("cluster firm", firm),
                                        ("cluster firm x date", (firm, date))]


for name, offs, y, cols, cases in shapes():
    base = None
    for label, ids in cases:
        cov_type = "cluster" if label.startswith("cluster") else label

        def call():
            if cov_type == "cluster":
                return eng.least_squares_statistics(y, cols, offs, add_intercept=True, cov_type="cluster", clusters=ids)
            return eng.least_squares_statistics(y, cols, offs, add_intercept=True, cov_type=cov_type)
        for _ in range(WARM):
            call()
        eng.synchronize()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(REPS):
            call()
        eng.synchronize()
        t1.record()
        t1.synchronize()
        ms = t0.elapsed_time(t1) / REPS
        base = ms if cov_type == "nonrobust" else base
        print(json.dumps({"shape": name, "cov_type": label, "ms": round(ms, 4), "vs_nonrobust": round(ms / base, 3)}), flush=True)
eng.close()
