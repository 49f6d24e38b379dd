"""K3c on cfg4's shape (ONE 1 000 000-row sequence x 6 features, f64, RLS half_life = 21: the look-back form) and rlsg's (10 000 x 1 000 x 6),
stationary and with a silent column -- the cost of the DEEP carry-in (k3c_scan.hip).  Frames: N(0, 1) columns; "stretch": column 2 is zero
over rows [200 000, 300 000); "zero": column 2 is zero throughout (every tile walks its predecessors' records); also the halo form
(RLS_ENGINE=halo) and the look-back form's fallback (RLS_SPINS=0) on the stretch frame.  Device-resident columns and outputs; each figure
is the mean of REPS calls between two device events after WARM calls.  One JSON line per case.  LIB=<path>: another build of the library."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polars_ols_amd import _lib  # noqa: E402

if os.environ.get("LIB"):
    from pathlib import Path

    _lib.LIB_PATH = Path(os.environ["LIB"])
from polars_ols_amd.engine import Engine  # noqa: E402

WARM, REPS = int(os.environ.get("WARM", 5)), int(os.environ.get("REPS", 30))
k = 6
eng = Engine(0)
time.sleep(2.0)                                               # (let a benchmark process that has just exited finish tearing down)
for shape, sizes in (("cfg4 1 x 1M", [1_000_000]), ("rlsg 10k x 1k", [1_000] * 10_000)):
    offs = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
    n = int(offs[-1])
    gen = torch.Generator(device="cuda").manual_seed(0)
    base = [torch.randn(n, device="cuda", generator=gen, dtype=torch.float64) for _ in range(k)]
    for frame in ("stationary", "stretch", "zero"):
        cols = [c.clone() for c in base]
        if frame == "stretch":
            cols[2][200_000:300_000] = 0.0
        elif frame == "zero":
            cols[2].zero_()
        y = sum(cols) + 0.1 * torch.randn(n, device="cuda", generator=gen, dtype=torch.float64)
        for opts in ({}, {"RLS_ENGINE": "halo"}, {"RLS_SPINS": "0"}):
            if opts and frame != "stretch":
                continue
            for key, v in opts.items():
                eng.set_option(key, v)

            def call():
                return eng.recursive_least_squares(y, cols, offs, half_life=21.0, null_free=True)
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
            print(json.dumps({"shape": shape, "frame": frame, "opts": opts, "kernel": eng.last_kernel,
                              "us": round(1e3 * t0.elapsed_time(t1) / REPS, 2)}), flush=True)
            for key in opts:
                eng.set_option(key, None)
eng.close()
