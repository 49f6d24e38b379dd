"""The recorded results of the static and dynamic entries (least_squares and its streamed, wide, multi-target and sharded forms; rolling and
recursive least squares) and the frames they were recorded on.

CASES describes every case -- entry, columns, group sizes, the null pattern and policy, solver parameters, library options, host or device
batch, the fields wanted -- and frame() rebuilds its frame from a seed derived from the case id (the cases taken over from
tests/dynamic_routes.py keep that file's frames).  tests/entries_record.json holds, per case and dtype, what the library produced BEFORE the
work buffers of csrc/api.hip, api_static.hip, api_dynamic.hip and api_stats.hip were cut by the scratch carver (the commit is named in the
file): the ``last_kernel`` string, a sha256 of the input frame and a sha256 of the raw bytes of every returned array (the first 16 hex
digits of each, one line per case).  It is a measurement of that parent, never of the code under test: scripts/record_entries.py wrote it,
test_entries_record_gpu.py holds the library to it.  Each case reaches one work buffer or one branch of a buffer's layout."""
import zlib
from pathlib import Path

import numpy as np

import dynamic_routes as DR
import static_routes as ST
from fits_record import DIGEST_HEX, digest, dump, load as _load  # noqa: F401  (the file format is the fits recording's)
from statistics_record import BASE, DRIFTED, DTYPES, SEG, SEG_OPT  # noqa: F401

PATH = Path(__file__).resolve().parent / "entries_record.json"
STREAM = {"STATIC_ENGINE": "stream"}
CLASSES = ["lognormal", 2040, 300, 0.5, [[8, 9000]]]       # static_routes.json, classes_streamed_top: the long groups' size class is streamed
ALL = ("coef", "pred", "resid", "status")


def load(path=PATH):
    return _load(path)


def _case(id, entry, k=4, sizes=BASE, **more):
    """kw: solver parameters; opts: library options; host / weights / icpt; nulls + policy (+ mask: validity bytes instead of NaNs);
    want: the fields asked for; m: targets (multi); dr: the case of tests/dynamic_routes.py that is run instead"""
    assert entry in ("dr", "rolling", "rls", "static", "multi", "sharded"), entry
    return dict(id=id, entry=entry, k=k, sizes=sizes, **more)


def _both(id, entry, **more):
    return [_case(f"{id}-dev", entry, **more), _case(f"{id}-host", entry, host=True, **more)]


CASES = []
# 1. every route of the dynamic entries
CASES += [_case(f"dr-{c['id']}", "dr", k=c["k"], sizes=c["sizes"], dr=c) for c in DR.CASES]
# 2. the prologue's forms those do not reach: NaN nulls without validity bytes (the scan decides), weights without the ones column, a
# validity mask whose zero-filling rewrite is deferred to the masked tile kernel
_ROLL = {"window_size": 20}
CASES += _both("roll-scan-nan", "rolling", k=3, sizes=DR.LONG, nulls=0.1, policy="drop", kw=_ROLL)
CASES += _both("rls-scan-nan", "rls", k=3, sizes=[3000, 50], nulls=0.1, policy="drop", kw={"half_life": 20.0})
CASES += _both("roll-weights-only", "rolling", k=3, sizes=DR.LONG, weights=True, policy="drop", kw=_ROLL)
CASES += _both("rls-weights-only", "rls", k=3, sizes=[300, 150, 40], weights=True, policy="drop", kw={"half_life": 20.0})
CASES += _both("roll-mask-deferred", "rolling", k=3, sizes=DR.LONG, nulls=0.1, mask=True, policy="drop_window", kw=_ROLL)
# 3. static entry, host batch: which output slots are staged, with and without weights, nulls as validity bytes or as NaNs under "drop"
for _n, _want in (("pred", ("pred",)), ("coef_resid", ("coef", "resid")), ("all", ALL)):
    for _w in (False, True):
        for _m in (False, True):
            CASES += [_case(f"static-{_n}{'-w' if _w else ''}{'-mask' if _m else '-nan'}-host", "static", host=True, want=_want, weights=_w,
                            nulls=0.1, mask=_m, policy="drop")]
CASES += _both("static-plain", "static", want=ALL)
# 4. the streamed route
CASES += _both("stream-whole", "static", want=ALL, opts=STREAM)
CASES += _both("stream-seg", "static", k=3, sizes=SEG, want=ALL, opts=dict(SEG_OPT, **STREAM))
CASES += _both("stream-seg-drop", "static", k=3, sizes=SEG, want=ALL, opts=dict(SEG_OPT, **STREAM), nulls=0.1, policy="drop")
CASES += [_case("stream-slices-dev", "static", k=3, sizes=[70000], want=ALL, opts=dict(SEG_OPT, **STREAM))]
CASES += [_case("stream-classes-dev", "static", k=3, sizes=CLASSES, want=ALL)]
# 5. the wide route
for _n, _more in (("plain", {}), ("drop", dict(nulls=0.1, policy="drop")), ("enet", dict(kw={"alpha": 0.3, "l1_ratio": 0.5})),
                  ("nostatus", dict(want=("coef", "pred", "resid")))):
    CASES += _both(f"wide-{_n}", "static", k=36, **dict(dict(want=ALL), **_more))
# 6. several targets
for _n, _more in (("pred", dict(want=("coef", "pred"))), ("nopred", dict(want=("coef",))),
                  ("drop", dict(want=("coef", "pred"), nulls=0.1, policy="drop")), ("drop-nopred", dict(want=("coef",), nulls=0.1, policy="drop")),
                  ("wide", dict(want=("coef", "pred"), k=36))):
    CASES += _both(f"multi-{_n}", "multi", m=3, **_more)
# 7. a world of one, assembled on the device
CASES += [_case("sharded-device", "sharded", k=6, sizes=[300, 0, 120, 999, 41], host=True, weights=True, want=ALL, kw={"alpha": 0.3, "l1_ratio": 0.0})]
for _c in CASES:
    _c["seed"] = zlib.crc32(_c["id"].encode())
assert len({c["id"] for c in CASES}) == len(CASES)


def frame(case, dtype):
    """-> dict of host arrays: y, cols, offs, valid (uint8 or None), w (or None), ys (multi: the further targets)"""
    if case["entry"] == "dr":
        y, cols, offs, valid, w = DR.frame(case["dr"], dtype)
        return dict(y=y, cols=cols, offs=offs, valid=valid, w=w, ys=[])
    rng = np.random.default_rng(case["seed"])
    sizes = case["sizes"]
    if sizes and isinstance(sizes[0], str):
        sizes = ST.group_sizes({"sizes": sizes}, rng)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, k = int(offs[-1]), case["k"]
    cols = [rng.standard_normal(n).astype(dtype) for _ in range(k)]
    signal = sum(c.astype(np.float64) for c in cols)
    y = (signal + 0.5 * rng.standard_normal(n)).astype(dtype)
    ys = [((i + 2) * signal + 0.5 * rng.standard_normal(n)).astype(dtype) for i in range(case.get("m", 1) - 1)]
    w = rng.uniform(0.5, 2.0, n).astype(dtype) if case.get("weights") else None
    valid = None
    if case.get("nulls", 0.0) > 0:
        hit = rng.random(n) < case["nulls"]
        if case.get("mask"):
            valid = (~hit).astype(np.uint8)
        else:                                  # one NaN per null row, in a column drawn for the row: a target, a feature, the weight
            rows = np.flatnonzero(hit)
            into = [y] + ys + cols + ([w] if w is not None else [])
            for r, j in zip(rows, rng.integers(0, len(into), size=len(rows))):
                into[j][r] = np.nan
    return dict(y=y, cols=cols, offs=offs, valid=valid, w=w, ys=ys)


def frame_digest(case, dtype):
    f = frame(case, dtype)
    return digest(f["y"], *f["cols"], f["offs"], f["valid"], f["w"], *f["ys"])


def run(eng, case, dtype):
    """One case through the engine -> ("ok", last_kernel, {field: sha256 of the array's bytes})"""
    import torch

    entry = case["entry"]
    if entry == "dr":
        coef, pred, name = DR.run(eng, case["dr"], dtype)
        return "ok", name, {"coef": digest(coef), "pred": digest(pred)}
    f = frame(case, dtype)
    put = (lambda a: a) if case.get("host") else (lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda())
    opts, kw = case.get("opts", {}), dict(case.get("kw", {}))
    kw.update(weights=put(f["w"]), valid=put(f["valid"]), add_intercept=bool(case.get("icpt")), null_policy=case.get("policy", "ignore"))
    y, cols = put(f["y"]), [put(c) for c in f["cols"]]
    try:
        for key, v in opts.items():
            eng.set_option(key, v)
        if entry == "static":
            out = eng.least_squares(y, cols, f["offs"], want=case["want"], **kw)
        elif entry == "multi":
            out = eng.multi_target_least_squares([y] + [put(t) for t in f["ys"]], cols, f["offs"], want=case["want"], **kw)
            for j, p in enumerate(out.pop("pred", [])):
                out[f"pred{j}"] = p
        elif entry == "sharded":
            from polars_ols_amd import comm_create_all, least_squares_sharded

            comms = comm_create_all([eng])
            try:
                out = least_squares_sharded([eng], y, cols, f["offs"], comms=comms, out="device", want=case["want"], **kw)
                out = {key: v.cpu() for key, v in out.items()}
            finally:
                for c in comms:
                    c.close()
        else:
            fn = eng.rolling_least_squares if entry == "rolling" else eng.recursive_least_squares
            out = fn(y, cols, f["offs"], **kw)
        eng.synchronize()
        name = eng.last_kernel
    finally:
        for key in opts:
            eng.set_option(key, None)
    return "ok", name, {k: digest(a.cpu().numpy() if hasattr(a, "cpu") else a) for k, a in sorted(out.items())}
