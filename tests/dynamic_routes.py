"""The recorded routes of the dynamic entries (rolling / expanding and recursive least squares) and the frames they were recorded on.

CASES describes every case -- entry, columns, a recipe for the sequence lengths, the null pattern, solver parameters, library options,
host or device batch -- and frame() rebuilds its frame from the case's seed.  tests/dynamic_routes.json holds, per case and dtype, the exact
``last_kernel`` string the library produced BEFORE the dynamic entries moved to csrc/api_dynamic.hip and were split into a route picker and
one function per route (the commit is named in the file).  It is a measurement of that parent, never of the code under test:
scripts/record_dynamic_routes.py wrote it, test_dynamic_route_gpu.py holds the library to it."""
import json
from pathlib import Path

import numpy as np

PATH = Path(__file__).resolve().parent / "dynamic_routes.json"
DTYPES = {"f32": np.float32, "f64": np.float64}

LONG = [1500, 300, 40]                     # one sequence longer than a 1 024-row tile beside short ones
SHORT = ["rand", 40, 20, 60]               # 40 sequences of 20 .. 60 rows: whole sequences per tile
THREE = [150, 150, 150]


def _roll(id, k, sizes, window, policy="drop", nulls=0.0, **more):
    kw = {"window_size": window, "null_policy": policy}
    for key in ("min_periods", "alpha"):
        if key in more:
            kw[key] = more.pop(key)
    return dict(id=id, entry="rolling", k=k, sizes=sizes, nulls=nulls, kw=kw, **more)


def _rls(id, k, sizes, half_life=None, nulls=0.0, **more):
    kw = {"half_life": half_life, "null_policy": "drop"}
    if "mean" in more:
        kw["initial_state_mean"] = [more.pop("mean")] * k
    return dict(id=id, entry="rls", k=k, sizes=sizes, nulls=nulls, kw=kw, **more)


CASES = [
    # ---- rolling
    _roll("roll-tiles-packed", 3, SHORT, 5),
    _roll("roll-tiles-halo", 3, LONG, 20),
    _roll("roll-tiles-halo-opt-halo", 3, LONG, 20, opts={"ROLLING_ENGINE": "halo"}),
    _roll("roll-tiles-halo-opt-halowave", 3, LONG, 20, opts={"ROLLING_ENGINE": "halowave"}),
    _roll("roll-tiles-k10", 10, LONG, 60),
    _roll("roll-beyond-halo-k8", 8, LONG, 400),
    _roll("roll-beyond-halo-k9", 9, LONG, 400),
    _roll("roll-beyond-halo-k3-chunk", 3, LONG, 400, opts={"ROLLING_ENGINE": "chunk"}),
    _roll("roll-beyond-halo-k12-chunk", 12, LONG, 400, opts={"ROLLING_ENGINE": "chunk"}),
    _roll("roll-width-k12", 12, THREE, 100),
    _roll("roll-width-k33", 33, THREE, 1000, alpha=0.5, min_periods=10),
    _roll("roll-width-k130", 130, THREE, 1000, alpha=0.5, min_periods=10),
    _roll("roll-compacted", 3, LONG, 20, nulls=0.1),
    _roll("roll-compacted-scatter", 3, LONG, 20, nulls=0.1, opts={"ROLLING_ENGINE": "scatter"}),
    _roll("roll-compacted-nocompact", 3, LONG, 20, nulls=0.1, opts={"ROLLING_ENGINE": "nocompact"}),
    _roll("roll-compacted-k12", 12, LONG, 40, nulls=0.1),
    _roll("roll-compacted-declines", 3, [400, 30, 500], 50, min_periods=8, special="starved"),
    _roll("roll-masked", 3, LONG, 20, policy="drop_window", nulls=0.1),
    _roll("roll-masked-declines", 3, [200, 100], 10, policy="drop_window", min_periods=5, special="never_dropped"),
    _roll("roll-masked-k12", 12, LONG, 40, policy="drop_window", nulls=0.1),
    _roll("roll-packed-weights-intercept", 2, SHORT, 5, weights=True, icpt=True),   # (3 columns with the ones column)
    _roll("roll-packed-host", 3, SHORT, 5, host=True),
    _roll("roll-compacted-host", 3, LONG, 20, nulls=0.1, host=True),
    _roll("roll-min-periods-beyond-window", 2, SHORT, 5, min_periods=10),
    _roll("roll-packed-window-3000", 3, SHORT, 3000),
    # ---- recursive
    _rls("rls-rows-packed", 3, SHORT, 20.0),
    _rls("rls-rows-long-scan", 3, [3000]),
    _rls("rls-rows-long-lookback", 3, [3000], 20.0),
    _rls("rls-rows-long-halo", 3, [3000], 20.0, opts={"RLS_ENGINE": "halo"}),
    _rls("rls-rows-long-k8", 8, [3000], 20.0),
    _rls("rls-rows-masked", 3, [3000, 50], 20.0, nulls=0.1),
    _rls("rls-seq", 3, SHORT, 20.0, opts={"RLS_ENGINE": "seq"}),
    _rls("rls-chunk", 3, SHORT, 20.0, opts={"RLS_ENGINE": "chunk"}),
    _rls("rls-wide-k12", 12, [300, 150, 40]),
    _rls("rls-wide-k12-chunk", 12, [300, 150, 40], opts={"RLS_ENGINE": "chunk"}),
    _rls("rls-wide-k33", 33, [300, 150, 40]),
    _rls("rls-wide-k130", 130, [300, 150, 40]),
    _rls("rls-prior-mean", 3, SHORT, 20.0, mean=0.25),
    _rls("rls-host", 3, SHORT, 20.0, host=True),
]
for _i, _c in enumerate(CASES):
    _c["seed"] = 1000 + _i


def load(path=PATH):
    """-> {(case id, dtype name): recorded last_kernel string}"""
    doc = json.loads(Path(path).read_text())
    return {(cid, dt): name for cid, by_dt in doc["kernels"].items() for dt, name in by_dt.items()}


def frame(case, dtype):
    """-> y, cols, offsets, valid (uint8 or None), weights (or None), as host arrays of `dtype`; y holds no NaN (nulls are validity bytes)"""
    rng = np.random.default_rng(case["seed"])
    sizes = case["sizes"]
    if sizes[0] == "rand":
        sizes = rng.integers(sizes[2], sizes[3] + 1, size=sizes[1])
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, k = int(offs[-1]), case["k"]
    cols = [rng.standard_normal(n).astype(dtype) for _ in range(k)]
    y = (sum(c.astype(np.float64) for c in cols) + 0.1 * rng.standard_normal(n)).astype(dtype)
    valid = (rng.random(n) >= case["nulls"]).astype(np.uint8) if case["nulls"] > 0 else None
    special = case.get("special")
    if special == "starved":               # one valid row in the middle sequence: fewer than min_periods
        valid = np.ones(n, dtype=np.uint8)
        valid[int(offs[1]):int(offs[2])] = 0
        valid[int(offs[1]) + 3] = 1
    elif special == "never_dropped":       # a valid first row, then nulls far beyond the window: the warm-up ends with row 0 older than the window
        valid = np.ones(n, dtype=np.uint8)
        valid[1:50] = 0
    w = rng.uniform(0.5, 2.0, n).astype(dtype) if case.get("weights") else None
    return y, cols, offs, valid, w


def run(eng, case, dtype):
    """One case through the engine -> (coef, pred) as float64 host arrays, last_kernel."""
    import torch

    y, cols, offs, valid, w = frame(case, dtype)
    put = (lambda a: a) if case.get("host") else (lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda())
    fn = eng.rolling_least_squares if case["entry"] == "rolling" else eng.recursive_least_squares
    opts = case.get("opts", {})
    try:
        for key, v in opts.items():
            eng.set_option(key, v)
        out = fn(put(y), [put(c) for c in cols], offs, valid=put(valid), weights=put(w), add_intercept=bool(case.get("icpt")),
                 null_free=valid is None, **case["kw"])
        eng.synchronize()
        name = eng.last_kernel
    finally:
        for key in opts:
            eng.set_option(key, None)
    host = lambda t: (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)).astype(np.float64)  # noqa: E731
    return host(out["coef"]), host(out["pred"]), name
