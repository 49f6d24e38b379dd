"""Conditioning ladders for the DYNAMIC entries (rolling_least_squares, recursive_least_squares): frames whose sequences have a known
smallest Cholesky pivot ratio, per-row truths that do not pass through any running update, the rows to compare and the list of cases
that reaches every route of the two entries.  Plain numpy, no device.  test_dyn_ladder_cpu.py holds the conditions the GPU test rests
on (the oracle's own error on every case), test_dyn_ladder_gpu.py the kernels, scripts/dyn_ladder.py prints the figures.

Kinds.  ``level`` and ``factor`` are cond_ladder._group's (features z_j + c fitted with an intercept; features that share one factor).
``scaled`` is the r = 1 panel with every feature multiplied by one common s: rolling OLS is exactly equivariant (beta scales by 1 / s, the
predictions do not move), so an absolute threshold in a kernel -- a pivot, a denominator, a "tiny" -- shows up on it.  RLS is not
equivariant because of its prior; its truth accounts for that.

Rungs.  One nominal pivot ratio r per SEQUENCE, r in RUNGS, two seeds per rung, shuffled.  Columns are rounded to the batch dtype first;
y = X beta + 0.1 noise with beta = linspace(-2, 2, kt) and both truths are computed from the rounded columns.

Exact ratio.  What the tests reason about is cond_ladder.min_pivot_ratio of the system the row's answer solves -- the window's
X'X (+ alpha I), the decayed information matrix of RLS with its prior -- never the nominal r.

Truths, per sampled row.  Both answers are least-squares solutions of a stacked design E beta ~ t:
  rolling   E = the (sqrt(w)-scaled) rows the window holds under the policy (window_matrix_rows), with sqrt(alpha) I below them under a penalty;
  RLS       E = sqrt(ff^(valid rows since s)) x_s for every valid row s up to the row, and sqrt(ff^(n_valid) / p0) I for the prior
            (t = the same weights on y, and sqrt(ff^n / p0) mean0): its normal equations are A = sum ff^.. x x' + ff^n I / p0 and b
            likewise.  Masked rows neither enter nor decay.
E beta ~ t is solved by Householder QR in np.longdouble (lstsq_ld) -- the normal equations are never formed, so the truth keeps
cond(E) eps_longdouble where forming A would cost cond(E)^2 -- and test_dyn_ladder_cpu.py checks it against mpmath at 50 digits.

Sampled rows (sample_rows): at most max_samples(kt) per case -- the first three rows after each sequence's warm-up, its first row that
rests on 2 kt observations (where the every-row comparison with the oracle begins) and its last row; then the rows at -1, 0, +1 around
the first 128- and the first 64-row boundary of every sequence; then around every multiple of 1 024, 512, 128 and 64 (counted from the
sequence start AND from the frame start: chunks are cut per sequence, tiles per frame).  Where that is more than the cap, the classes are
kept in this order and the first class that does not fit is thinned evenly.

Rungs without an oracle (``no_oracle`` of a case): where the reference itself misses the conditions test_dyn_ladder_cpu.py sets for it, the
sequences of that rung stay in the frame and are held to the TRUTH like every other; only the comparison with the oracle leaves them out."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

import cond_ladder as CL
from rls_exact_ref import forgetting_factor

RUNGS = (1.0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6)
SEEDS_PER_RUNG = 2
SCALED_RUNGS = (1.0, 1.0, 1.0)                        # the ``scaled`` kind: every sequence is an r = 1 panel (six of them)
KINDS = ("level", "factor", "scaled")
TOL = CL.TOL
DTYPES = CL.DTYPES
STRICT_RATIO = 1e-4 / np.sqrt(10.0)                   # exact ratio >= this: the plain bound tol + tol |truth|
EPS = float(np.finfo(np.float64).eps)


def max_samples(kt: int) -> int:
    """the cap on sampled rows: 200, fewer where one truth costs a wide QR in extended precision"""
    return 200 if kt <= 48 else 40


# ------------------------------------------------------------------------------------------------------------------ window rule
def window_matrix_rows(offs, valid, i, window, policy) -> np.ndarray:
    """indices of the rows whose outer products make up row i's window state (the rows the reference's deque / fixed window holds)"""
    g = int(np.searchsorted(offs, i, side="right") - 1)
    s = int(offs[g])
    v = np.ones(i + 1 - s, dtype=bool) if valid is None else np.asarray(valid[s:i + 1]).astype(bool)
    idx = s + np.flatnonzero(v)
    if policy == "drop":
        return idx[-window:]                           # the last `window` VALID rows
    return idx[idx > i - window]                       # the valid rows among the last `window` rows


def window_matrix(offs, valid, X, i, window, policy):
    """the feature rows of window_matrix_rows"""
    return X[window_matrix_rows(offs, valid, i, window, policy)]


# ------------------------------------------------------------------------------------------------------------------ frames
def ladder(case: Dict, dt: str, scale: Optional[float] = None) -> Dict:
    """The frame of a case in dtype dt.  -> dict(y, cols, offs, valid, w, icpt, target, kt, dt, X, yv): cols / y / w as the batch passes
    them (rounded), X the n x kt design the solver sees in f64 (ones column last, sqrt(w)-scaled), yv the scaled target.
    ``scale`` overrides the case's common feature scale (the s = 1 twin of a ``scaled`` case)."""
    dtype = DTYPES[dt]
    kind, kt, seed = case["kind"], case["kt"], case["seed"]
    rungs = case.get("rungs", SCALED_RUNGS if kind == "scaled" else RUNGS)
    seeds = case.get("seeds", SEEDS_PER_RUNG)
    order = np.random.default_rng([seed, 11]).permutation(len(rungs) * seeds)
    target = np.repeat(np.asarray(rungs, dtype=np.float64), seeds)[order]
    icpt = kind == "level"
    s = float(case.get("scale", 1.0) if scale is None else scale)
    beta = np.linspace(-2.0, 2.0, kt)
    xs, ys, sizes = [], [], []
    for g, r in enumerate(target):
        rng = np.random.default_rng([seed, KINDS.index(kind), kt, int(order[g])])
        n = int(case["rows"])
        x = CL._group("factor" if kind == "scaled" else kind, float(r), kt, n, rng).astype(dtype)       # rounded first ...
        x64 = x.astype(np.float64)
        if icpt:
            x64 = np.column_stack([x64, np.ones(n)])
        y = (x64 @ beta + 0.1 * rng.standard_normal(n)).astype(dtype)                                  # ... y from the rounded columns
        if s != 1.0:
            x = (s * x.astype(np.float64)).astype(dtype)                                               # the same panel, one common scale
        xs.append(x); ys.append(y); sizes.append(n)
    x = np.concatenate(xs, axis=0)
    y = np.concatenate(ys)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    rng = np.random.default_rng([seed, 13])
    w = rng.uniform(0.5, 2.0, n).astype(dtype) if case.get("weights") else None
    valid = (rng.random(n) >= case["nulls"]).astype(np.uint8) if case.get("nulls", 0.0) > 0 else None
    X = x.astype(np.float64)
    if icpt:
        X = np.column_stack([X, np.ones(n)])
    yv = y.astype(np.float64)
    Xraw = X
    if w is not None:
        sw = np.sqrt(w.astype(np.float64))
        X, yv = X * sw[:, None], yv * sw
    return {"y": y, "cols": [np.ascontiguousarray(x[:, j]) for j in range(x.shape[1])], "offs": offs, "valid": valid, "w": w, "icpt": icpt,
            "target": target, "kt": kt, "dt": dt, "X": X, "yv": yv, "Xraw": Xraw}


# ------------------------------------------------------------------------------------------------------------------ the rows to compare
def warm_up_row(fr: Dict, case: Dict, g: int) -> int:
    """the first row of sequence g that has an answer: the min_periods-th valid row (rolling), the first row (RLS); -1: none"""
    s, e = int(fr["offs"][g]), int(fr["offs"][g + 1])
    if case["entry"] == "rls":
        return s if e > s else -1
    mp = case["kw"].get("min_periods")
    mp = min(fr["kt"], case["kw"]["window_size"]) if mp is None else mp
    v = np.ones(e - s, dtype=bool) if fr["valid"] is None else fr["valid"][s:e].astype(bool)
    idx = np.flatnonzero(v)
    return s + int(idx[mp - 1]) if len(idx) >= mp else -1


def sample_rows(fr: Dict, case: Dict) -> np.ndarray:
    """the sampled rows of the module docstring, sorted.  Under "drop_window" with nulls a masked row repeats an earlier solve (its own window
    is not what was solved), so a masked pick moves to the next valid row of its sequence."""
    offs, cap, kt = fr["offs"], max_samples(fr["kt"]), fr["kt"]
    nobs = observations(fr, case)
    # class 0: warm-up rows, the first row that rests on 2 kt observations, the sequence end; 1: the first 128- and the first 64-boundary of
    # every sequence (KP_REFRESH, the chunk / wave rows); then every 1024, 512, 128, 64 boundary
    classes: List[List[int]] = [[] for _ in range(6)]
    for g in range(len(offs) - 1):
        s, e = int(offs[g]), int(offs[g + 1])
        w0 = warm_up_row(fr, case, g)
        if w0 < 0:
            continue
        well = s + np.flatnonzero(nobs[s:e] >= 2 * kt)
        classes[0] += [i for i in (w0, w0 + 1, w0 + 2) if i < e] + [int(i) for i in well[:1]]
        classes[0] += [i for i in ((e - 3, e - 2, e - 1) if kt > 48 else (e - 1,)) if i >= w0]      # (wide: three rows that rest on 2 kt observations)
        rel = max(1, -(-(w0 - s) // 64))                          # the first 64-row boundary of the sequence at or behind the warm-up
        firsts = [s + 64 * (rel + rel % 2)] + ([s + 64 * (rel + 1 - rel % 2)] if kt <= 48 else [])   # the first multiple of 128; of 64 alone
        classes[1] += [i for m in firsts for i in (m - 1, m, m + 1) if w0 <= i < e]
        for c, step in ((2, 1024), (3, 512), (4, 128), (5, 64)):
            for base in (s, 0):                                  # boundaries counted from the sequence start and from the frame start
                first = base + step * max(1, -(-(w0 - base) // step))
                for m in range(first, e + 1, step):
                    classes[c] += [i for i in (m - 1, m, m + 1) if w0 <= i < e]
    picked: List[int] = []
    for cl in classes:
        fresh = sorted(set(cl) - set(picked))
        room = cap - len(picked)
        if room <= 0:
            break
        if len(fresh) > room:
            fresh = [fresh[j] for j in np.unique(np.linspace(0, len(fresh) - 1, room).astype(int))]
        picked += fresh
    rows = np.array(sorted(set(picked)), dtype=np.int64)
    if fr["valid"] is not None and case["entry"] == "rolling" and case["kw"]["null_policy"] == "drop_window":
        moved = []
        for i in rows:
            g = int(np.searchsorted(offs, i, side="right") - 1)
            nxt = np.flatnonzero(fr["valid"][i:int(offs[g + 1])])
            if len(nxt):
                moved.append(int(i) + int(nxt[0]))
            else:                                                # (nothing valid behind it: the last valid row of the sequence)
                moved.append(int(offs[g]) + int(np.flatnonzero(fr["valid"][int(offs[g]):i])[-1]))
        rows = np.array(sorted(set(moved)), dtype=np.int64)
    return rows


# ------------------------------------------------------------------------------------------------------------------ truths
def lstsq_ld(E: np.ndarray, t: np.ndarray) -> np.ndarray:
    """argmin |E beta - t| by Householder QR in np.longdouble; NaN when E has fewer rows than columns or a zero column remainder"""
    n, k = E.shape
    if n < k:
        return np.full(k, np.nan)
    R = np.column_stack([E, t]).astype(np.longdouble)
    for j in range(k):
        v = R[j:, j].copy()
        nv = np.sqrt(v @ v)
        if not nv > 0:
            return np.full(k, np.nan)
        v[0] += nv if v[0] >= 0 else -nv
        v /= np.sqrt(v @ v)
        R[j:, j:] -= 2.0 * np.outer(v, v @ R[j:, j:])
    beta = np.zeros(k, dtype=np.longdouble)
    for j in range(k - 1, -1, -1):
        beta[j] = (R[j, k] - R[j, j + 1:k] @ beta[j + 1:]) / R[j, j]
    return beta.astype(np.float64)


def stacked_design(fr: Dict, case: Dict, i: int):
    """(E, t) of row i: the least-squares problem whose solution the entry returns on that row (module docstring)"""
    X, yv, offs, valid, kt = fr["X"], fr["yv"], fr["offs"], fr["valid"], fr["kt"]
    kw = case["kw"]
    if case["entry"] == "rolling":
        idx = window_matrix_rows(offs, valid, int(i), kw["window_size"], kw["null_policy"])
        E, t = X[idx], yv[idx]
        alpha = kw.get("alpha")
        if alpha:
            E, t = np.vstack([E, np.sqrt(alpha) * np.eye(kt)]), np.concatenate([t, np.zeros(kt)])
        return E, t
    g = int(np.searchsorted(offs, i, side="right") - 1)
    s = int(offs[g])
    v = np.ones(i + 1 - s, dtype=bool) if valid is None else valid[s:i + 1].astype(bool)
    idx = s + np.flatnonzero(v)
    nv = len(idx)
    ff = np.longdouble(forgetting_factor(kw.get("half_life")))
    age = np.arange(nv - 1, -1, -1).astype(np.longdouble)          # valid rows since s
    sw = np.sqrt(ff ** age)
    p0 = np.longdouble(kw.get("initial_state_covariance", 10.0))
    sp = np.sqrt(ff ** np.longdouble(nv) / p0)
    mean0 = np.asarray(kw.get("initial_state_mean", np.zeros(kt)), dtype=np.longdouble)
    E = np.vstack([X[idx].astype(np.longdouble) * sw[:, None], sp * np.eye(kt, dtype=np.longdouble)])
    t = np.concatenate([yv[idx].astype(np.longdouble) * sw, sp * mean0])
    return E, t


def truth(fr: Dict, case: Dict, rows: np.ndarray) -> Dict:
    """per sampled row: coef, pred (NaN on a masked row), the exact pivot ratio and cond of the normal matrix, the observations held"""
    kt = fr["kt"]
    coef = np.full((len(rows), kt), np.nan)
    pred = np.full(len(rows), np.nan)
    ratio = np.zeros(len(rows))
    cond = np.full(len(rows), np.inf)
    nobs = np.zeros(len(rows), dtype=np.int64)
    for j, i in enumerate(rows):
        E, t = stacked_design(fr, case, int(i))
        nobs[j] = E.shape[0] - (kt if case["entry"] == "rls" or case["kw"].get("alpha") else 0)
        coef[j] = lstsq_ld(E, t)
        if fr["valid"] is None or fr["valid"][i]:
            pred[j] = fr["Xraw"][i] @ coef[j]
        if E.shape[0] >= kt:
            ratio[j] = CL.min_pivot_ratio(np.asarray(E, dtype=np.longdouble))
            E64 = np.asarray(E, dtype=np.float64)
            with np.errstate(all="ignore"):
                c = np.linalg.cond(E64.T @ E64)
            cond[j] = c if np.isfinite(c) else np.inf
    return {"coef": coef, "pred": pred, "ratio": ratio, "cond": cond, "nobs": nobs}


def row_tol(tr: Dict, dt: str) -> np.ndarray:
    """the tolerance of each sampled row: TOL where its exact ratio is at least STRICT_RATIO, max(TOL, 1e3 cond eps) below"""
    tol = TOL[dt]
    return np.where(tr["ratio"] >= STRICT_RATIO, tol, np.maximum(tol, 1e3 * tr["cond"] * EPS))


def sample_units(coef, pred, rows, tr: Dict, tol_rows: np.ndarray) -> np.ndarray:
    """per sampled row: the worst |got - truth| / (tol_i + tol_i |truth|) over its coefficients and its prediction"""
    out = np.zeros(len(rows))
    for j, i in enumerate(rows):
        if not np.isfinite(tol_rows[j]) or np.isnan(tr["coef"][j]).any():
            continue
        u = CL.bound_units(coef[i], tr["coef"][j], tol_rows[j]).max()
        if not np.isnan(tr["pred"][j]):
            u = max(u, float(CL.bound_units(pred[i:i + 1], tr["pred"][j:j + 1], tol_rows[j])[0]))
        out[j] = u
    return out


def sequence_of(fr: Dict, rows) -> np.ndarray:
    return np.searchsorted(fr["offs"], np.asarray(rows), side="right") - 1


def observations(fr: Dict, case: Dict) -> np.ndarray:
    """per row of the frame: the observations behind its answer (rolling: in the window; RLS: valid rows so far)"""
    offs, valid = fr["offs"], fr["valid"]
    n = int(offs[-1])
    v = np.ones(n, dtype=np.int64) if valid is None else valid.astype(np.int64)
    out = np.zeros(n, dtype=np.int64)
    for g in range(len(offs) - 1):
        s, e = int(offs[g]), int(offs[g + 1])
        c = np.cumsum(v[s:e])
        if case["entry"] == "rls":
            out[s:e] = c
        elif case["kw"]["null_policy"] == "drop":
            out[s:e] = np.minimum(c, case["kw"]["window_size"])
        else:
            w = case["kw"]["window_size"]
            lag = np.concatenate([np.zeros(min(w, e - s), dtype=np.int64), c[: max(0, e - s - w)]])
            out[s:e] = c - lag
    return out


def sequence_tol(fr: Dict, tr: Dict, rows: np.ndarray, dt: str) -> np.ndarray:
    """per sequence, for the every-row comparison with the oracle: TOL when every sampled window of the sequence with 2 kt observations has
    an exact ratio of at least STRICT_RATIO, else max(TOL, 1e3 eps x the largest cond among them)"""
    seq = sequence_of(fr, rows)
    out = np.full(len(fr["offs"]) - 1, TOL[dt])
    for g in range(len(out)):
        m = (seq == g) & (tr["nobs"] >= 2 * fr["kt"])
        if m.any() and tr["ratio"][m].min() < STRICT_RATIO:
            out[g] = max(TOL[dt], 1e3 * float(tr["cond"][m].max()) * EPS)
    return out


# ------------------------------------------------------------------------------------------------------------------ oracle and library
def oracle(fr: Dict, case: Dict):
    """(coef, pred) of the C oracle on the frame: f64 on the rounded inputs; predictions NaN on masked rows, un-scaled by 1 / sqrt(w)"""
    from oracle import orc

    cols = [np.ascontiguousarray(fr["X"][:, j]) for j in range(fr["kt"])]
    valid = None if fr["valid"] is None else fr["valid"].astype(bool)
    kw = dict(case["kw"])
    if case["entry"] == "rls":
        kw.pop("null_policy", None)
        ref = orc.batched_rls(fr["yv"], cols, fr["offs"], is_valid=valid, **kw)
    else:
        window = kw.pop("window_size")
        ref = orc.batched_rolling(fr["yv"], cols, fr["offs"], window, is_valid=valid, **kw)
    pred = ref["pred"]
    if valid is not None:
        pred = np.where(valid, pred, np.nan)
    if fr["w"] is not None:
        pred = pred / np.sqrt(fr["w"].astype(np.float64))
    return ref["coef"], pred


def oracle_on_batch_dtype_products(fr: Dict, case: Dict):
    """oracle() on the columns the prologue hands the kernels of a weighted batch: x sqrt(w), y sqrt(w) and sqrt(w) itself rounded to the
    BATCH dtype (dyn_prep.hip dyn_rewrite_kernel), then solved in f64"""
    sw = np.sqrt(fr["w"])                                                            # in the batch dtype
    cols = [c * sw for c in fr["cols"]] + ([sw] if fr["icpt"] else [])
    twin = dict(fr, X=np.column_stack(cols).astype(np.float64), yv=(fr["y"] * sw).astype(np.float64))
    return oracle(twin, case)


def run(eng, case: Dict, fr: Dict):
    """One case through the engine under the case's options (restored afterwards) -> (coef, pred) as f64 host arrays, last_kernel"""
    import torch

    put = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    fn = eng.rolling_least_squares if case["entry"] == "rolling" else eng.recursive_least_squares
    opts = case.get("opts", {})
    kw = dict(case["kw"])
    if case["entry"] == "rls":
        kw["null_policy"] = "drop"
    try:
        for key, v in opts.items():
            eng.set_option(key, v)
        out = fn(put(fr["y"]), [put(c) for c in fr["cols"]], fr["offs"], valid=put(fr["valid"]), weights=put(fr["w"]),
                 add_intercept=fr["icpt"], null_free=fr["valid"] is None, **kw)
        eng.synchronize()
        name = eng.last_kernel
    finally:
        for key in opts:
            eng.set_option(key, None)
    host = lambda t: t.cpu().numpy().astype(np.float64)  # noqa: E731
    return host(out["coef"]), host(out["pred"]), name


def family(name: str) -> str:
    """last_kernel without its dtype: k4_rolling_tiles_f64_gathered -> k4_rolling_tiles_gathered"""
    return name.replace("_f64", "").replace("_f32", "")


# ------------------------------------------------------------------------------------------------------------------ the cases
def _roll(reach, fam, kind, kt, rows, window, policy="drop", **more):
    kw = {"window_size": window, "null_policy": policy, "min_periods": more.pop("min_periods", kt)}
    for key in ("alpha", "use_woodbury"):
        if key in more:
            kw[key] = more.pop(key)
    return dict(entry="rolling", reach=reach, family=fam, kind=kind, kt=kt, rows=rows, kw=kw, **more)


def _rls(reach, fam, kind, kt, rows, half_life, p0, **more):
    kw = {"half_life": half_life, "initial_state_covariance": p0}
    if "mean" in more:
        kw["initial_state_mean"] = [more.pop("mean")] * kt
    return dict(entry="rls", reach=reach, family=fam, kind=kind, kt=kt, rows=rows, kw=kw, **more)


# RLS from p0 = 1e6 on ``level`` data: the reference's own P-form recursion misses the 0.1 of the bound the CPU test wants of it on the 1e-4
# rung, the lowest that is held to the plain bound -- 0.21 .. 2.5 on the first rows that rest on 2 kt observations, 0.23 / 0.18 further on
# at 33 / 130 columns.  Those sequences are held to the truth only ("Dynamic ladder").
P0_1E6_LEVEL = (1e-4,)
TILES, WALK, K4P = "k4_rolling_tiles", "k4_rolling_walk", "k4p_rolling_inverse_wave"
WIDE = (1.0, 1e-2, 1e-4, 1e-6)                       # 130 columns under 2 000 rows: four rungs, one seed each, 480 rows

# The smallest frames that reach each route (tests/dynamic_routes.py::CASES has the shapes and options): 14 sequences of `rows` rows --
# 300: whole sequences per tile / one chunk per sequence; 1 500: cut by the 1 024-row tiles and chunks.  Windows kt + 3, 4 kt or 252
# where the route admits them (the walk and the cut K4p cases need a window beyond the halo forms' 252 / 508 rows).
CASES = [
    # ---- rolling
    _roll("tiles-packed", TILES, "factor", 3, 300, 6),
    _roll("tiles-packed", TILES, "level", 4, 300, 16, weights=True),
    _roll("tiles-packed-min-periods-1", TILES, "factor", 3, 300, 12, min_periods=1, alpha=1e-5),   # (the penalty defines the rows with fewer than kt observations)
    _roll("tiles-packed-ridge", TILES, "factor", 4, 300, 16, alpha=1e-5),
    _roll("tiles-own-halo", TILES, "factor", 4, 1500, 252),
    _roll("tiles-own-halo", TILES, "level", 3, 1500, 12, opts={"ROLLING_ENGINE": "halo"}),
    _roll("tiles-halo-wave", TILES, "factor", 3, 1500, 12, opts={"ROLLING_ENGINE": "halowave"}),
    _roll("tiles-halo-wave", TILES, "level", 4, 1500, 252, opts={"ROLLING_ENGINE": "halowave"}),
    _roll("tiles-k10", TILES, "factor", 10, 1500, 40),
    _roll("tiles-k10", TILES, "level", 10, 1500, 252, weights=True),
    _roll("walk-k8", WALK, "factor", 8, 1500, 300),
    _roll("walk-k8", WALK, "level", 8, 1500, 300),
    _roll("k4p-single-chunk", K4P, "factor", 12, 300, 48),
    _roll("k4p-single-chunk", K4P, "level", 12, 300, 252),
    _roll("k4p-single-chunk-kp32", K4P, "factor", 20, 300, 80),
    _roll("k4p-cut", K4P, "factor", 12, 1500, 252),
    _roll("k4p-cut", K4P, "level", 9, 1500, 300),
    _roll("k4p-cut-kp32", K4P, "level", 20, 1500, 80),
    _roll("k4p-x4", K4P + "_x4", "factor", 12, 300, 48, opts={"K4P_LPS": "16"}),
    _roll("k4p-x4", K4P + "_x4", "level", 12, 1500, 252, opts={"K4P_LPS": "16"}),
    _roll("k4w", "k4w_rolling_walk", "factor", 12, 1500, 48, opts={"ROLLING_ENGINE": "chunk"}),
    _roll("k4w", "k4w_rolling_walk", "level", 12, 1500, 252, opts={"ROLLING_ENGINE": "chunk"}),
    _roll("k4x-k33", "k4x_rolling_inverse", "factor", 33, 400, 132),
    _roll("k4x-k33-no-woodbury", "k4x_rolling_inverse", "level", 33, 400, 132, use_woodbury=False),
    _roll("k4x-k48", "k4x_rolling_inverse", "level", 48, 400, 192),
    _roll("k4x-k48-no-woodbury", "k4x_rolling_inverse", "factor", 48, 400, 192, use_woodbury=False),
    _roll("k4y-k130", "k4y_rolling_inverse_hbm", "factor", 130, 480, 300, rungs=WIDE, seeds=1),
    _roll("k4y-k130", "k4y_rolling_inverse_hbm", "level", 130, 480, 300, rungs=WIDE, seeds=1),
    _roll("gathered", TILES + "_gathered", "factor", 4, 1500, 16, nulls=0.05),
    _roll("gathered", TILES + "_gathered", "level", 4, 1500, 252, nulls=0.05),
    _roll("masked-tiles", TILES + "_masked", "factor", 4, 1500, 252, policy="drop_window", nulls=0.05),
    _roll("masked-tiles", TILES + "_masked", "level", 4, 1500, 16, policy="drop_window", nulls=0.05),
    _roll("masked-k4p", K4P, "factor", 12, 1500, 48, policy="drop_window", nulls=0.05),
    _roll("masked-k4p", K4P, "level", 12, 1500, 252, policy="drop_window", nulls=0.05),
    _roll("scaled-tiles", TILES, "scaled", 4, 1500, 16, scale=1e-4),
    _roll("scaled-tiles", TILES, "scaled", 4, 1500, 252, scale=1e4),
    _roll("scaled-walk", WALK, "scaled", 8, 1500, 300, scale=1e-4),
    _roll("scaled-k4p", K4P, "scaled", 12, 1500, 48, scale=1e-4),
    _roll("scaled-k4p", K4P, "scaled", 12, 1500, 252, scale=1e4),
    _roll("scaled-k4x", "k4x_rolling_inverse", "scaled", 33, 400, 132, scale=1e-4),
    _roll("scaled-k4x", "k4x_rolling_inverse", "scaled", 33, 400, 132, scale=1e4),
    # ---- recursive (half-life 21 with p0 = 10, None with p0 = 1e6: a prior of 0.1 I that never decays would hold every rung at ~0.1 / rows)
    _rls("k3-seq", "k3_rls", "factor", 3, 300, 21.0, 1e6, opts={"RLS_ENGINE": "seq"}),
    _rls("k3-seq", "k3_rls", "level", 4, 300, None, 1e6, opts={"RLS_ENGINE": "seq"}, no_oracle=P0_1E6_LEVEL),
    _rls("k3s-rows", "k3s_rls_rows", "factor", 4, 300, 21.0, 1e6, weights=True),
    _rls("k3s-rows", "k3s_rls_rows", "level", 3, 1500, None, 1e6, no_oracle=P0_1E6_LEVEL),
    _rls("k3s-rows-prior-mean", "k3s_rls_rows_lookback", "level", 4, 1500, 21.0, 10.0, mean=0.25),
    _rls("k3s-rows-masked", "k3s_rls_rows", "factor", 3, 1500, 21.0, 10.0, nulls=0.05),
    _rls("k3s-lookback", "k3s_rls_rows_lookback", "factor", 3, 1500, 21.0, 10.0),
    _rls("k3s-lookback", "k3s_rls_rows_lookback", "level", 4, 1500, 21.0, 10.0, weights=True),
    _rls("k3s-lookback-no-spins", "k3s_rls_rows_lookback", "level", 3, 1500, 21.0, 1e6, opts={"RLS_SPINS": "0"}, no_oracle=P0_1E6_LEVEL),
    _rls("k3s-halo", "k3s_rls_rows_halo", "factor", 4, 1500, 21.0, 10.0, opts={"RLS_ENGINE": "halo"}),
    _rls("k3s-halo", "k3s_rls_rows_halo", "level", 8, 1500, 21.0, 10.0),
    _rls("k3s-scan-walk", "k3s_rls_scan_walk", "factor", 3, 300, 21.0, 1e6, opts={"RLS_ENGINE": "chunk"}),
    _rls("k3s-scan-walk", "k3s_rls_scan_walk", "level", 4, 1500, None, 1e6, opts={"RLS_ENGINE": "chunk"}, no_oracle=P0_1E6_LEVEL),
    _rls("k3p-kp16", "k3p_rls_inverse_wave", "factor", 12, 300, None, 1e6),
    _rls("k3p-kp16", "k3p_rls_inverse_wave", "level", 12, 1500, 21.0, 10.0),
    _rls("k3p-kp32", "k3p_rls_inverse_wave", "level", 20, 300, None, 1e6, no_oracle=P0_1E6_LEVEL),
    _rls("k3p-kp32", "k3p_rls_inverse_wave", "factor", 20, 1500, None, 1e6),
    _rls("k3sw", "k3sw_rls_scan_walk", "factor", 12, 1500, None, 1e6, opts={"RLS_ENGINE": "chunk"}),
    _rls("k3sw", "k3sw_rls_scan_walk", "level", 12, 300, 21.0, 1e6, opts={"RLS_ENGINE": "chunk"}, no_oracle=P0_1E6_LEVEL),
    _rls("k3x", "k3x_rls_inverse", "factor", 33, 400, None, 1e6),
    _rls("k3x", "k3x_rls_inverse", "level", 33, 400, None, 1e6, no_oracle=P0_1E6_LEVEL),
    _rls("k3y", "k3y_rls_inverse_hbm", "factor", 130, 480, None, 1e6, rungs=WIDE, seeds=1),
    _rls("k3y", "k3y_rls_inverse_hbm", "level", 130, 480, None, 1e6, rungs=WIDE, seeds=1, no_oracle=P0_1E6_LEVEL),
    _rls("scaled-k3s-rows", "k3s_rls_rows", "scaled", 4, 300, 21.0, 10.0, scale=1e-4),
    _rls("scaled-k3p", "k3p_rls_inverse_wave", "scaled", 12, 300, None, 1e6, scale=1e-4),
    _rls("scaled-k3s-rows", "k3s_rls_rows", "scaled", 4, 300, 21.0, 10.0, scale=1e4),
    _rls("scaled-k3p", "k3p_rls_inverse_wave", "scaled", 12, 300, None, 10.0, scale=1e4),
]
for _i, _c in enumerate(CASES):
    _c["seed"] = 2000 + _i
    _c["id"] = "-".join([_c["entry"][:4], _c["reach"], _c["kind"], f"k{_c['kt']}", f"n{_c['rows']}"] +
                        ([f"w{_c['kw']['window_size']}"] if _c["entry"] == "rolling" else [f"hl{_c['kw']['half_life']}", f"p{_c['kw']['initial_state_covariance']:g}"]) +
                        ([f"s{_c['scale']:g}"] if "scale" in _c else []))
assert len({c["id"] for c in CASES}) == len(CASES)

# the routes the issue names: every one must be the `reach` of a case that ran its recorded kernel family (test (e))
REACH = {"tiles-packed", "tiles-own-halo", "tiles-halo-wave", "tiles-k10", "walk-k8", "k4p-single-chunk", "k4p-cut", "k4p-x4", "k4w",
         "k4x-k33", "k4x-k33-no-woodbury", "k4x-k48", "k4x-k48-no-woodbury", "k4y-k130", "gathered", "masked-tiles", "masked-k4p",
         "tiles-packed-min-periods-1", "k3-seq", "k3s-rows", "k3s-lookback", "k3s-lookback-no-spins", "k3s-halo", "k3s-scan-walk",
         "k3p-kp16", "k3p-kp32", "k3sw", "k3x", "k3y", "k3s-rows-prior-mean"}
# OPEN (DESIGN.md "Dynamic ladder").  test_dyn_ladder_gpu.py holds these (case, dtype) to everything else and expects exactly their rows
# below OPEN_RATIO to fail.
# * f32 batches WITH WEIGHTS.  The prologue writes x sqrt(w) back in the batch dtype, as the reference's f32 frame arithmetic does; that
#   rounding of the inputs (6e-8 relative) is amplified by cond(X) and, below pivot ratios of 1e-4, exceeds the f32 bound on every route behind
#   it.  test_dyn_ladder_cpu.py shows that the ORACLE fed the same f32 products misses the bound on these cases.
# * K3 (k3_rls.hip, the wave-per-sequence P-form: RLS_ENGINE=seq, or columns the row-parallel kernel cannot take) from p0 = 1e6 on ``level``
#   data without forgetting, f64: 18.9 x the bound on the first row that rests on 2 kt observations of a 1e-4 sequence (exact ratio 3.5e-5),
#   where the reference's own P-form is at 0.21.
OPEN_F32_WEIGHTS = {("roll-tiles-packed-level-k4-n300-w16", "f32"), ("rls-k3s-rows-factor-k4-n300-hl21.0-p1e+06", "f32")}
OPEN = OPEN_F32_WEIGHTS | {("rls-k3-seq-level-k4-n300-hlNone-p1e+06", "f64")}
OPEN_RATIO = 1e-4                                       # the rows of an open case with an exact ratio of at least this are asserted like any other
PARAMS = [(c, dt) for c in CASES for dt in ("f64", "f32")]
PARAM_IDS = [f"{c['id']}-{dt}" for c, dt in PARAMS]

_CACHE: Dict = {}


def prepared(case: Dict, dt: str) -> Dict:
    """frame, sampled rows, truth and oracle of a (case, dtype), computed once per process and left unchanged"""
    key = (case["id"], dt)
    if key not in _CACHE:
        fr = ladder(case, dt)
        rows = sample_rows(fr, case)
        tr = truth(fr, case, rows)
        oc, op = oracle(fr, case)
        _CACHE[key] = {"fr": fr, "rows": rows, "truth": tr, "oracle_coef": oc, "oracle_pred": op}
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------ the comparison
def compare(case: Dict, dt: str, coef: np.ndarray, pred: np.ndarray) -> Dict:
    """What test_dyn_ladder_gpu.py asserts and scripts/dyn_ladder.py prints, of one run's (coef, pred):
    ``truth_units``    per sampled row, error / bound against the truth, the bound decided by the row's exact ratio (row_tol)
    ``oracle_units``   per frame row that rests on 2 kt observations, error / (2 x the bound of its sequence) against the oracle (0 elsewhere,
                       and on the sequences of a rung the case lists under ``no_oracle``).  The bound of a sequence comes from its sampled
                       rows, the first row with 2 kt observations among them
    ``nan_rows``       the rows with 2 kt observations (under a ridge penalty: all rows) whose NaN pattern (coefficients or prediction) differs from the oracle's"""
    p = prepared(case, dt)
    fr, rows, tr = p["fr"], p["rows"], p["truth"]
    kt = fr["kt"]
    truth_units = sample_units(coef, pred, rows, tr, row_tol(tr, dt))
    well = observations(fr, case) >= 2 * kt
    oc, op = p["oracle_coef"], p["oracle_pred"]
    pinned = well | bool(case["entry"] == "rolling" and case["kw"].get("alpha"))       # (a penalty defines every row, under-determined ones included)
    nan_rows = np.flatnonzero(pinned & ((np.isnan(coef) != np.isnan(oc)).any(axis=1) | (np.isnan(pred) != np.isnan(op))))
    tol_rows = 2.0 * np.repeat(sequence_tol(fr, tr, rows, dt), np.diff(fr["offs"]))
    judged = np.repeat(~np.isin(fr["target"], case.get("no_oracle", ())), np.diff(fr["offs"]))
    uc = CL.bound_units(coef, oc, 1.0)                                       # |got - ref| / (1 + |ref|): the tolerance divides below
    up = CL.bound_units(pred, op, 1.0)
    oracle_units = np.where(well & judged, np.maximum(uc.max(axis=1), up) / tol_rows, 0.0)
    return {"truth_units": truth_units, "oracle_units": oracle_units, "nan_rows": nan_rows}
