"""Host time per call of the seven per-group fit entries on one small DEVICE frame (groups of 60, 200, 0, 35 and 120 rows, 4 features, f64:
the kernels have next to nothing to do, so the host code of csrc/api_fits.hip and of the Python front end dominates).

    python scripts/fits_host_cost.py <label> [calls]

One process is one pass: per entry WARM calls, then `calls` timed ones and a synchronise; prints one JSON line {"build": label, "us":
{entry: microseconds per call}}.  To compare two builds run passes of both alternately, in both orders, and set the median of the new
build against the min .. max range of the old one (profiles/fits_host_cost.txt)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
WARM = 20


def main(label, calls):
    import numpy as np
    import torch

    import fits_record as FR
    from polars_ols_amd import Engine

    eng = Engine(0)
    us = {}
    for entry in FR.ENTRIES:
        f = FR.frame(dict(entry=entry, k=4, sizes=FR.BASE, seed=7), np.float64)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        y, cols, offs = put(f["y"]), [put(c) for c in f["cols"]], f["offs"]
        z, ids = [put(c) for c in f["z"]], [put(c) for c in f["ids"]]
        want = FR.COMMON + FR.OWN[entry]
        call = {"ridge_cv": lambda: eng.ridge_cv(y, cols, offs, FR.RIDGE_GRID, want=want),
                "rlm": lambda: eng.rlm(y, cols, offs, want=want),
                "elastic_net_cv": lambda: eng.elastic_net_cv(y, cols, offs, FR.ENET_GRID, want=want, **FR.ENET_KW),
                "glm": lambda: eng.glm(y, cols, offs, want=want),
                "iv2sls": lambda: eng.iv2sls(y, cols, z, offs, n_endog=1, want=want),
                "absorb": lambda: eng.absorb(y, cols, ids[0], offs, want=want),
                "absorb2": lambda: eng.absorb2(y, cols, ids[0], ids[1], offs, want=want)}[entry]
        for _ in range(WARM):
            call()
        eng.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        eng.synchronize()
        us[entry] = round(1e6 * (time.perf_counter() - t0) / calls, 2)
    eng.close()
    print(json.dumps({"build": label, "calls": calls, "us": us}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 200)
