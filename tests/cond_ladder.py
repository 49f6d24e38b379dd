"""Conditioning ladders: frames whose groups have a KNOWN smallest Cholesky pivot ratio, for the tests of the rule that flags a group of a
static solve for the fix-up pass (``pivot_tol``, csrc/api_static.hip resolve_solve_plan; DESIGN.md "K6 fix_up").  Plain numpy, no device.

Every group of a frame is one rung -- a target pivot ratio r -- of one of three kinds:

* ``pair``    the last feature is x0 + sqrt(r / (1 - r)) z: sin^2 of its angle to x0 is r (r = 1: an independent column)
* ``factor``  every feature is sqrt(1 - r) f + sqrt(r) z_j with one common f per group (asset returns that share a market factor)
* ``level``   every feature is z_j + c, fitted with an intercept (price levels).  The kernels append the ones column last, so it is the
              late pivot, and what the m features leave of it is 1 / (1 + m c^2): c = sqrt((1 / r - 1) / m) puts that ratio at r.
              (With c = sqrt(1 / r - 1) the ratio would be r / m, more than half a decade off the rung from four features on.)

y = X beta + 0.1 noise with DISTINCT coefficients linspace(-2, 2, kt), so that a permuted coefficient row is caught.  Columns are rounded to
the batch dtype before anything else is computed from them.  Three seeds per rung; the rungs of a ladder are the groups of one frame, shuffled.

``exact_ratio`` is what the tests reason about, never the nominal r: the smallest d_j / (G_jj + alpha) of an unpivoted Cholesky of
X'X + alpha I, in extended precision, from the rounded, sqrt(w)-scaled columns in the kernels' column order, on the rows the fit keeps."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

KINDS = ("pair", "factor", "level")
SEEDS_PER_RUNG = 3
TOL = {"f32": 1e-4, "f64": 1e-6}                     # the project's parity tolerance (atol = rtol)
KEEP_LINE = {"f32": 0.1, "f64": 1e-4}                # exact ratio >= this: ordinary data, must NOT reach the fix-up pool (status 0)
FLAG_LINE = {"f32": 1e-4, "f64": 1e-11}              # exact ratio <= this: must be flagged (status 1)
DTYPES = {"f32": np.float32, "f64": np.float64}


def rungs(dt: str) -> np.ndarray:
    """target pivot ratios: f32 half-decades 1 .. 1e-6; f64 1, 1e-2, 1e-4, then half-decades 1e-6 .. 1e-12"""
    if dt == "f32":
        return 10.0 ** (-0.5 * np.arange(13))
    return np.concatenate([[1.0, 1e-2, 1e-4], 10.0 ** (-6.0 - 0.5 * np.arange(13))])


def _group(kind: str, r: float, kt: int, n: int, rng) -> np.ndarray:
    """the n x (features) block of one rung, f64, before rounding; ``level`` has kt - 1 features (the intercept is the kt-th column)"""
    if kind == "pair":
        x = rng.standard_normal((n, kt))
        if r < 1.0:
            x[:, -1] = x[:, 0] + np.sqrt(r / (1.0 - r)) * x[:, -1]
        return x
    if kind == "factor":
        z, f = rng.standard_normal((n, kt)), rng.standard_normal(n)
        return np.sqrt(1.0 - r) * f[:, None] + np.sqrt(r) * z
    if kind == "level":
        m = kt - 1
        return rng.standard_normal((n, m)) + np.sqrt((1.0 / r - 1.0) / m)
    raise ValueError(kind)


def ladder(kind: str, dt: str, kt: int, rows, seed: int = 0, weights: bool = False, nan_frac: float = 0.0) -> Dict:
    """One frame: every rung of ``dt`` x SEEDS_PER_RUNG groups of ``rows`` rows (an int, or (lo, hi): drawn per group), shuffled.
    kt counts the columns of the solve (``level``: kt - 1 features + the intercept).  -> dict(y, cols, offs, w, icpt, target, kind, dt, kt)"""
    dtype = DTYPES[dt]
    order = np.random.default_rng([seed, 7]).permutation(len(rungs(dt)) * SEEDS_PER_RUNG)
    target = np.repeat(rungs(dt), SEEDS_PER_RUNG)[order]
    icpt = kind == "level"
    beta = np.linspace(-2.0, 2.0, kt)
    xs, ys, ws, sizes = [], [], [], []
    for g, r in enumerate(target):
        rng = np.random.default_rng([seed, KINDS.index(kind), kt, int(order[g])])
        n = int(rows) if np.isscalar(rows) else int(rng.integers(rows[0], rows[1] + 1))
        x = _group(kind, float(r), kt, n, rng).astype(dtype)                 # rounded first ...
        x64 = x.astype(np.float64)
        if icpt:
            x64 = np.column_stack([x64, np.ones(n)])
        y = (x64 @ beta + 0.1 * rng.standard_normal(n)).astype(dtype)        # ... everything else from the rounded columns
        if nan_frac > 0:
            y[rng.random(n) < nan_frac] = np.nan
        ws.append(rng.uniform(0.5, 2.0, n).astype(dtype))
        xs.append(x); ys.append(y); sizes.append(n)
    x = np.concatenate(xs, axis=0)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return {"y": np.concatenate(ys), "cols": [np.ascontiguousarray(x[:, j]) for j in range(x.shape[1])], "offs": offs,
            "w": np.concatenate(ws) if weights else None, "icpt": icpt, "target": target, "kind": kind, "dt": dt, "kt": kt}


def design(fr: Dict, g: int, drop_null_targets: bool = False):
    """(X, y) of group g as the solve sees them: f64 copies of the rounded columns, the ones column last, sqrt(w)-scaled, and under a
    drop policy only the rows with a target"""
    s, e = int(fr["offs"][g]), int(fr["offs"][g + 1])
    X = np.column_stack([c[s:e] for c in fr["cols"]]).astype(np.float64)
    if fr["icpt"]:
        X = np.column_stack([X, np.ones(e - s)])
    y = fr["y"][s:e].astype(np.float64)
    if fr["w"] is not None:
        sw = np.sqrt(fr["w"][s:e].astype(np.float64))
        X, y = X * sw[:, None], y * sw
    if drop_null_targets:
        ok = ~np.isnan(y)
        X, y = X[ok], y[ok]
    return X, y


def min_pivot_ratio(X: np.ndarray, alpha: float = 0.0) -> float:
    """smallest d_j / (G_jj + alpha) of the unpivoted Cholesky of X'X + alpha I, in np.longdouble (<= 0: the factorisation broke down)"""
    Xl = X.astype(np.longdouble)
    A = Xl.T @ Xl + np.longdouble(alpha) * np.eye(X.shape[1], dtype=np.longdouble)
    diag0 = np.diag(A).copy()
    worst = np.longdouble(np.inf)
    for j in range(A.shape[0]):
        d = A[j, j]
        worst = min(worst, d / diag0[j])
        if not d > 0:
            break
        v = A[j + 1:, j].copy()
        A[j + 1:, j + 1:] -= np.outer(v, v) / d
    return float(worst)


def exact_ratio(fr: Dict, g: int, alpha: float = 0.0, drop_null_targets: bool = False) -> float:
    return min_pivot_ratio(design(fr, g, drop_null_targets)[0], alpha)


def exact_ratios(fr: Dict, alpha: float = 0.0, drop_null_targets: bool = False) -> np.ndarray:
    return np.array([exact_ratio(fr, g, alpha, drop_null_targets) for g in range(len(fr["offs"]) - 1)])


def zones(ratio: np.ndarray, dt: str):
    """(keep, between, flag) masks of the groups by exact ratio"""
    keep, flag = ratio >= KEEP_LINE[dt], ratio <= FLAG_LINE[dt]
    return keep, ~keep & ~flag, flag


def bound_units(got, ref, tol: float) -> np.ndarray:
    """|got - ref| in units of the project bound tol + tol |ref|; NaN in ``got`` where ``ref`` is finite counts as inf"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(all="ignore"):
        u = np.abs(got - ref) / (tol + tol * np.abs(ref))
    u[np.isnan(got) & ~np.isnan(ref)] = np.inf
    u[np.isnan(ref)] = 0.0
    return u


# ------------------------------------------------------------------------------------------------------------------ the GPU cases
# (route, options): the library options of a case are set and restored around the call, as test_static_route_gpu.py does
ROUTES = {"default": {}, "mfma": {"K1_ENGINE": "mfma"}, "k2": {"STATIC_ENGINE": "k2"}, "k2w": {"STATIC_ENGINE": "k2w"},
          "stream": {"STATIC_ENGINE": "stream"}, "noclasses": {"NO_CLASSES": "1"}}
TEAM_ROWS = (24, 40)                                  # K1t: several groups per wave


def _case(route, dt, kind, kt, rows, w=0, policy="ignore", ridge=False):
    return {"route": route, "dt": dt, "kind": kind, "kt": kt, "rows": rows, "weights": bool(w), "policy": policy, "ridge": ridge}


def cases() -> list:
    """The ladder cases of test_cond_ladder_gpu.py and scripts/cond_ladder.py.  Shapes are picked to reach every Cholesky of the static
    routes, not for size: K1's unrolled (<= 8 columns), LDS (9-15) and row-per-lane (16+, K1t's 8- and 32-lane teams) solves, K1m, every
    padded width of k2_chol (10 / 12 / 14 / 16) and k2w_chol (20 / 24 / 28 / 32), gram_solve behind the streamed Gram, K8.  The default route's
    grid runs with and without weights; on the forced routes weights alternate, so that every kernel family sees both forms."""
    out, i = [], 0
    for dt in ("f32", "f64"):
        for kind in KINDS:
            for kt in (3, 8, 10, 12, 15, 20, 31):                                 # the default route: every width both ways
                for rows in (200, 1000):
                    for w in (0, 1):
                        out.append(_case("default", dt, kind, kt, rows, w=w))
            for kt in (3, 8, 10, 15):                                            # K1t teams (16 f64 columns: K2)
                out.append(_case("default", dt, kind, kt, TEAM_ROWS, w=i % 2)); i += 1
            for kt in (3, 8, 10, 15):
                out.append(_case("mfma", dt, kind, kt, 200 if kt != 10 else 1000, w=i % 2)); i += 1
            for kt in (3, 10, 12, 14, 15):
                out.append(_case("k2", dt, kind, kt, 200 if kt != 12 else 1000, w=i % 2)); i += 1
            for kt in (20, 24, 28, 31):
                out.append(_case("k2w", dt, kind, kt, 200 if kt != 24 else 1000, w=i % 2)); i += 1
            for kt in (3, 8, 20, 31):
                out.append(_case("stream", dt, kind, kt, 1000 if kt in (8, 31) else 200, w=i % 2)); i += 1
            out.append(_case("noclasses", dt, kind, 8, (150, 1000), w=i % 2)); i += 1
            out.append(_case("default", dt, kind, 40, 200, w=i % 2)); i += 1      # K8
            for kt, rows in ((8, 200), (12, 1000), (20, 200)):                    # the _nulls kernels
                out.append(_case("default", dt, kind, kt, rows, w=i % 2, policy="drop")); i += 1
    # f32 ridge, alpha = 1e-3 x rows: the plan's rule with G_jj + alpha, on every route (f64 ridge: the reference solves the same f64 normal
    # equations, there is no independent truth)
    for kind in KINDS:
        for route, kt, rows in (("default", 8, 200), ("default", 12, 1000), ("default", 20, 200), ("mfma", 10, 200), ("k2w", 24, 200),
                                ("default", 40, 200), ("k2", 12, 200), ("stream", 8, 1000)):
            out.append(_case(route, "f32", kind, kt, rows, w=i % 2, ridge=True)); i += 1
    return out


def case_id(c: Dict) -> str:
    rows = c["rows"] if np.isscalar(c["rows"]) else f"{c['rows'][0]}to{c['rows'][1]}"
    return "-".join([c["route"], c["dt"], c["kind"], f"k{c['kt']}", f"n{rows}"] + (["w"] if c["weights"] else []) +
                    (["drop"] if c["policy"] != "ignore" else []) + (["ridge"] if c["ridge"] else []))


def case_frame(c: Dict) -> Dict:
    seed = 1000 + c["kt"] + (0 if np.isscalar(c["rows"]) else 5)
    return ladder(c["kind"], c["dt"], c["kt"], c["rows"], seed=seed, weights=c["weights"], nan_frac=0.02 if c["policy"] != "ignore" else 0.0)


def case_alpha(c: Dict) -> float:
    """f32 ridge: alpha = 1e-3 x rows"""
    if not c["ridge"]:
        return 0.0
    return 1e-3 * (c["rows"] if np.isscalar(c["rows"]) else c["rows"][1])


def kernel_family(name: str) -> str:
    """last_kernel -> k1 | k1t | k1m | k2 | k2w | streamed | wide | ... (static_routes.family, with the K1 family told apart by prefix)"""
    from static_routes import family

    if name.startswith("k1t_"):
        return "k1t"
    if name.startswith("k1m_"):
        return "k1m"
    return family(name)


def run_case(eng, c: Dict, fr: Optional[Dict] = None, extra_options: Optional[Dict] = None):
    """One library call on the case's frame under the case's options (restored afterwards) -> (outputs as f64 host arrays, last_kernel)"""
    fr = case_frame(c) if fr is None else fr
    opts = dict(ROUTES[c["route"]], **(extra_options or {}))
    kw = {"alpha": case_alpha(c), "l1_ratio": 0.0} if c["ridge"] else {}
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        out = eng.least_squares(fr["y"], fr["cols"], fr["offs"], weights=fr["w"], add_intercept=fr["icpt"], null_policy=c["policy"],
                                want=("coef", "pred", "status"), **kw)
        name = eng.last_kernel
    finally:
        for k in opts:
            eng.set_option(k, None)
    return {k: np.asarray(v, dtype=np.float64 if k != "status" else np.int64) for k, v in out.items()}, name


def case_expected(c: Dict, fr: Dict):
    """(coef, pred) of the oracle: f64 on the rounded inputs, the reference's own solver for the call"""
    from test_nulls_gpu import _expected

    kw = {"alpha": case_alpha(c), "l1_ratio": 0.0} if c["ridge"] else {}
    coef, pred, _ = _expected(fr["y"], fr["cols"], fr["offs"], fr["w"], fr["icpt"], c["policy"], **kw)
    return coef, pred


def group_units(fr: Dict, got: Dict, coef_ref: np.ndarray, pred_ref: np.ndarray) -> np.ndarray:
    """per group: the worst error / bound over its coefficients and its predictions"""
    tol = TOL[fr["dt"]]
    uc = bound_units(got["coef"], coef_ref, tol).max(axis=1)
    up = bound_units(got["pred"], pred_ref, tol)
    offs = fr["offs"]
    return np.array([max(uc[g], up[offs[g]:offs[g + 1]].max()) for g in range(len(offs) - 1)])
