"""Host time per call of the static and dynamic entries on small frames (the kernels have next to nothing to do, so the host code of
csrc/api.hip, api_static.hip, api_dynamic.hip, api_stats.hip and of the Python front end dominates): the static entry on a device batch,
on a host batch and streamed, multi-target under "drop", rolling on packed tiles and on a compacted frame, RLS on the row kernel, plain
statistics on a host batch.  f64; the static frames are groups of 60, 200, 0, 35 and 120 rows with 4 features, the dynamic ones those of
tests/dynamic_routes.py.

    python scripts/entries_host_cost.py <label> [calls] [library]

One process is one pass: per entry WARM calls, then `calls` timed ones and a synchronise; prints one JSON line {"build": label, "us":
{entry: microseconds per call}}.  `library`: the shared library of the build to measure (default: the tree's).  To compare builds run
passes of all of them alternately, in both orders; several entries repeat to within 0.1 %, so the yardstick is the union of the min .. max
ranges of TWO separate builds of the old code, and the median of the new build has to lie inside it (profiles/entries_host_cost.txt)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
WARM = 20


def main(label, calls, library=None):
    import numpy as np
    import torch

    from polars_ols_amd import _lib

    if library:
        _lib.LIB_PATH = Path(library).resolve()
    import dynamic_routes as DR
    import entries_record as ER
    from polars_ols_amd import Engine

    eng = Engine(0)
    put = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    f = ER.frame(dict(entry="static", k=4, sizes=ER.BASE, seed=7), np.float64)
    y, cols, offs = put(f["y"]), [put(c) for c in f["cols"]], f["offs"]
    fm = ER.frame(dict(entry="multi", k=4, sizes=ER.BASE, seed=8, m=3, nulls=0.1), np.float64)
    ys, mcols = [put(fm["y"])] + [put(t) for t in fm["ys"]], [put(c) for c in fm["cols"]]
    dyn = {}
    for name, cid in (("rolling_packed", "roll-tiles-packed"), ("rolling_compacted", "roll-compacted"), ("rls_rows", "rls-rows-packed")):
        case = next(c for c in DR.CASES if c["id"] == cid)
        dy, dcols, doffs, dvalid, _ = DR.frame(case, np.float64)
        fn = eng.rolling_least_squares if case["entry"] == "rolling" else eng.recursive_least_squares
        dyn[name] = (lambda fn=fn, a=(put(dy), [put(c) for c in dcols], doffs), kw=dict(case["kw"], valid=put(dvalid), null_free=dvalid is None):
                     fn(*a, **kw))
    entries = {"static_device": (lambda: eng.least_squares(y, cols, offs, want=ER.ALL), {}),
               "static_host": (lambda: eng.least_squares(f["y"], f["cols"], offs, want=ER.ALL), {}),
               "static_streamed": (lambda: eng.least_squares(y, cols, offs, want=ER.ALL), ER.STREAM),
               "multi_target_drop": (lambda: eng.multi_target_least_squares(ys, mcols, fm["offs"], null_policy="drop", want=("coef", "pred")), {}),
               "rolling_packed": (dyn["rolling_packed"], {}), "rolling_compacted": (dyn["rolling_compacted"], {}), "rls_rows": (dyn["rls_rows"], {}),
               "statistics_host": (lambda: eng.least_squares_statistics(f["y"], f["cols"], offs), {})}
    us = {}
    for entry, (call, opts) in entries.items():
        for key, v in opts.items():
            eng.set_option(key, v)
        for _ in range(WARM):
            call()
        eng.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        eng.synchronize()
        us[entry] = round(1e6 * (time.perf_counter() - t0) / calls, 2)
        for key in opts:
            eng.set_option(key, None)
    eng.close()
    print(json.dumps({"build": label, "calls": calls, "us": us}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 200, sys.argv[3] if len(sys.argv) > 3 else None)
