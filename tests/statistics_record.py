"""The recorded results of statistics mode (the plain, robust, cluster and influence entries) and the frames they were recorded on.

CASES describes every case -- kind, columns, group sizes, the null pattern and policy, solver parameters, library options, host or device
batch -- and frame() rebuilds its frame from a seed derived from the case id.  tests/statistics_record.json holds, per case and dtype, what the
library produced BEFORE statistics mode moved to csrc/api_stats.hip and was split into two levels and one function per stage (the commit is
named in the file): the ``last_kernel`` string, a sha256 of the input frame and a sha256 of the raw bytes of every returned array -- or, for
the cases the library rejects, the error code and message.  It is a measurement of that parent, never of the code under test:
scripts/record_statistics.py wrote it, test_statistics_record_gpu.py holds the library to it."""
import hashlib
import json
import zlib
from pathlib import Path

import numpy as np

PATH = Path(__file__).resolve().parent / "statistics_record.json"
DTYPES = {"f32": np.float32, "f64": np.float64}

BASE = [60, 200, 0, 35, 120]               # ragged, one empty group
KT31 = [80, 150, 64]
SEG = [1500, 40, 0, 700]                   # with SEG_TARGET=256: two groups cut into segments beside an unsplit and an empty one
SEG_OPT = {"SEG_TARGET": "256"}
KINDS = ("plain", "HC1", "HC3", "HAC", "cluster1", "cluster2", "influence")
DRIFTED = "frame generator drifted: re-record on the parent"


def _case(id, kind, k=4, sizes=BASE, **more):
    """kw: solver parameters; opts: library options; host / weights / icpt; nulls + policy (+ mask: validity bytes instead of NaNs);
    null_free; use_correction; reject: the library is expected to refuse the call"""
    assert kind in KINDS, kind
    return dict(id=id, kind=kind, k=k, sizes=sizes, **more)


def _both(id, kind, **more):
    return [_case(f"{id}-dev", kind, **more), _case(f"{id}-host", kind, host=True, **more)]


CASES = []
# 1. every kind, device and host
for _k in KINDS:
    CASES += _both(_k, _k)
CASES += [_case("cluster1-nocorrection-dev", "cluster1", use_correction=False)]
# 2. null policies: 10 % of the rows hold a NaN (in y, a feature or the weight)
for _k in ("plain", "HAC", "cluster2", "influence"):
    CASES += _both(f"drop-{_k}", _k, nulls=0.1, policy="drop")
for _k in ("cluster2", "influence"):
    CASES += _both(f"drop_y_zero_x-{_k}", _k, nulls=0.1, policy="drop_y_zero_x")
for _k in ("plain", "influence"):
    CASES += _both(f"zero-{_k}", _k, nulls=0.1, policy="zero")
CASES += _both("drop-mask-plain", "plain", nulls=0.1, policy="drop", mask=True)
CASES += [_case("drop-null_free-plain-dev", "plain", policy="drop", null_free=True)]      # stays on the fit level
# 3. weights + intercept
for _k in ("plain", "HC3", "cluster1", "influence"):
    CASES += [_case(f"wi-{_k}-dev", _k, weights=True, icpt=True)]
CASES += [_case("wi-drop-influence-host", "influence", weights=True, icpt=True, host=True, nulls=0.1, policy="drop")]
# 4. solver branches
CASES += [_case("ridge-plain-dev", "plain", kw={"alpha": 2.5}),
          _case("ridge-influence-dev", "influence", kw={"alpha": 2.5}),
          _case("enet-plain-dev", "plain", kw={"alpha": 0.3, "l1_ratio": 0.5}),
          _case("svd-plain-dev", "plain", kw={"solve_method": "svd"})]
# 5. width: kt = 31 is the last of K7, 32 .. the first of the wide kernels, kt + 1 > 128 their factored form
for _k in ("plain", "HC1", "influence"):
    CASES += [_case(f"kt31-{_k}-dev", _k, k=30, sizes=KT31, icpt=True)]
CASES += _both("k36-plain", "plain", k=36)
CASES += _both("k36-drop-plain", "plain", k=36, nulls=0.1, policy="drop")
CASES += [_case("k130-plain-dev", "plain", k=130, sizes=[300, 200])]
# 6. long groups cut into segments
for _k in ("plain", "HAC", "cluster2", "influence"):
    CASES += [_case(f"seg-{_k}-dev", _k, k=3, sizes=SEG, opts=SEG_OPT)]
for _k in ("plain", "influence"):
    CASES += [_case(f"seg-{_k}-host", _k, k=3, sizes=SEG, opts=SEG_OPT, host=True)]
CASES += [_case("seg-drop-influence-dev", "influence", k=3, sizes=SEG, opts=SEG_OPT, nulls=0.1, policy="drop"),   # row pass over the ORIGINAL segments
          _case("seg-stream-plain-dev", "plain", k=3, sizes=SEG, opts=dict(SEG_OPT, STATIC_ENGINE="stream"))]      # the solve hands back its Gram matrices
# 7. the 16-slice Gram reduce: one group of >= 256 segments, at most 256 groups, a solve route that keeps no Gram matrix (ridge by SVD with a
# caller's rcond: every group goes to the Jacobi-SVD pass)
CASES += [_case("seg-slices-svd_all-dev", "plain", k=3, sizes=[70000], opts=SEG_OPT, kw={"alpha": 1.0, "solve_method": "svd", "rcond": 1e-12})]
# 8. rejections: (code, message)
CASES += [_case("reject-mask-ignore", "plain", nulls=0.1, policy="ignore", mask=True, reject=True),
          _case("reject-kt32-HC1", "HC1", k=31, sizes=KT31, icpt=True, reject=True),
          _case("reject-kt32-cluster", "cluster1", k=31, sizes=KT31, icpt=True, reject=True),
          _case("reject-kt32-influence", "influence", k=31, sizes=KT31, icpt=True, reject=True),
          _case("reject-maxlags", "HAC", maxlags=256, reject=True),
          _case("reject-qr-ridge-kt31", "plain", k=30, sizes=KT31, icpt=True, kw={"solve_method": "qr", "alpha": 1.0}, reject=True),
          _case("reject-qr-ridge-kt32", "plain", k=31, sizes=KT31, icpt=True, kw={"solve_method": "qr", "alpha": 1.0}, reject=True)]
for _c in CASES:
    _c["seed"] = zlib.crc32(_c["id"].encode())
assert len({c["id"] for c in CASES}) == len(CASES)


def load(path=PATH):
    """-> (commit, {(case id, dtype name): recorded entry})"""
    doc = json.loads(Path(path).read_text())
    return doc["recorded_on_commit"], {(cid, dt): e for cid, by_dt in doc["cases"].items() for dt, e in by_dt.items()}


def frame(case, dtype):
    """-> y, cols, offsets, valid (uint8 or None), weights (or None), ids (list of int64 columns), as host arrays"""
    rng = np.random.default_rng(case["seed"])
    offs = np.concatenate([[0], np.cumsum(case["sizes"])]).astype(np.int64)
    n, k = int(offs[-1]), case["k"]
    cols = [rng.standard_normal(n).astype(dtype) for _ in range(k)]
    y = (sum(c.astype(np.float64) for c in cols) + 0.5 * rng.standard_normal(n)).astype(dtype)
    w = rng.uniform(0.5, 2.0, n).astype(dtype) if case.get("weights") else None
    ways = {"cluster1": 1, "cluster2": 2}.get(case["kind"], 0)
    ids = [rng.integers(0, 7 - 2 * i, n).astype(np.int64) for i in range(ways)]
    valid = None
    if case.get("nulls", 0.0) > 0:
        hit = rng.random(n) < case["nulls"]
        if case.get("mask"):
            valid = (~hit).astype(np.uint8)
        else:                                  # one NaN per null row, in a column drawn for the row: the target, a feature, the weight
            rows = np.flatnonzero(hit)
            into = [y] + cols + ([w] if w is not None else [])
            for r, j in zip(rows, rng.integers(0, len(into), size=len(rows))):
                into[j][r] = np.nan
    return y, cols, offs, valid, w, ids


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def frame_digest(case, dtype):
    y, cols, offs, valid, w, ids = frame(case, dtype)
    return digest(y, *cols, offs, valid, w, *ids)


def run(eng, case, dtype):
    """One case through the engine -> ("ok", last_kernel, {field: sha256 of the array's bytes}) or ("rejected", code, message)"""
    import torch

    from polars_ols_amd import _lib as L

    y, cols, offs, valid, w, ids = frame(case, dtype)
    put = (lambda a: a) if case.get("host") else (lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda())
    kw = dict(weights=put(w), valid=put(valid), add_intercept=bool(case.get("icpt")), null_policy=case.get("policy", "ignore"),
              null_free=bool(case.get("null_free")), **case.get("kw", {}))
    kind, opts = case["kind"], case.get("opts", {})
    try:
        for key, v in opts.items():
            eng.set_option(key, v)
        if kind == "influence":
            out = eng.least_squares_influence(put(y), [put(c) for c in cols], offs,
                                              want=L.INFLUENCE_FIELDS + L.INFLUENCE_GROUP_FIELDS + ("coef", "status"), **kw)
        elif ids:
            out = eng.least_squares_statistics(put(y), [put(c) for c in cols], offs, cov_type="cluster", clusters=[put(a) for a in ids],
                                               use_correction=case.get("use_correction", True), **kw)
        else:
            out = eng.least_squares_statistics(put(y), [put(c) for c in cols], offs, cov_type="nonrobust" if kind == "plain" else kind,
                                               maxlags=case.get("maxlags", 3) if kind == "HAC" else None, **kw)
        eng.synchronize()
        name = eng.last_kernel
    except L.PolsError as e:
        if e.code == -3:                       # POLS_ERR_HIP: a device error is no rejection
            raise
        return "rejected", e.code, str(e)
    finally:
        for key in opts:
            eng.set_option(key, None)
    return "ok", name, {f: digest(a.cpu().numpy() if hasattr(a, "cpu") else a) for f, a in sorted(out.items())}
