"""mode="statistics" with robust standard errors (K7r): non-robust vs HC1, HC3, HAC(5), HAC(21) on two shapes,
10 000 groups x 1 000 rows x 8 features + intercept (f32) and 1 group x 5M rows x 8 features + intercept (f64).
Device-resident columns and outputs; each figure is the mean of REPS calls between two device events after WARM calls.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python scripts/bench_robust_stats.py`.  One JSON line per case."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polars_ols_amd.engine import Engine  # noqa: E402

WARM, REPS = int(os.environ.get("WARM", 5)), int(os.environ.get("REPS", 20))
SHAPES = [("10k x 1k f32", [1_000] * 10_000, torch.float32), ("1 x 5M f64", [5_000_000], torch.float64)]
CASES = [("nonrobust", None), ("HC1", None), ("HC3", None), ("HAC", 5), ("HAC", 21)]

eng = Engine(0)
time.sleep(2.0)                                               # (let a benchmark process that has just exited finish tearing down)
k = 8
for name, sizes, dt in SHAPES:
    offs = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
    n = int(offs[-1])
    gen = torch.Generator(device="cuda").manual_seed(0)
    cols = [torch.randn(n, device="cuda", generator=gen, dtype=dt) for _ in range(k)]
    y = sum(cols) + 0.1 * torch.randn(n, device="cuda", generator=gen, dtype=dt)
    base = None
    for cov_type, lags in CASES:
        def call():
            return eng.least_squares_statistics(y, cols, offs, add_intercept=True, cov_type=cov_type, maxlags=lags)
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
        label = cov_type if lags is None else f"{cov_type}({lags})"
        print(json.dumps({"shape": name, "cov_type": label, "ms": round(ms, 4), "vs_nonrobust": round(ms / base, 3)}), flush=True)
eng.close()
