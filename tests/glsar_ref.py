"""numpy restatement of per-group AR(1) feasible GLS (pols_glsar, K18): the yardstick of tests/test_glsar_*.py.
Per group, f64, rows in frame order t = 1..n (time order), X = [x | 1], kt columns.  At a given rho the ROWS are transformed --
z*_t = z_t - rho z_{t-1} for t >= 2, Prais-Winsten adds z*_1 = sqrt(1 - rho^2) z_1 -- and b(rho) is the least-squares fit of the
transformed rows; the device forms the same normal equations from lag-one cross-moments, this file never does.
    rho^0 = 0 (b^0 is OLS);  e = y - X b^i on the ORIGINAL rows;  rho^{i+1} = sum_{t>=2} e_t e_{t-1} / sum_{t<=n-1} e_t^2;
    stop when |rho^{i+1} - rho^i| <= tol or after max_iter updates (NOT_CONVERGED); the reported b is b(rho*) at the last rho;
    u_t = e_t - rho* e_{t-1} (t >= 2), u_1 = sqrt(1 - rho*^2) e_1 (Prais-Winsten);  RSS* = sum u^2;  df = n* - kt;
    V = RSS* / df (X*'X*)^-1;  dw = sum (u_t - u_{t-1})^2 / sum u_t^2;  dw_ols the same of the OLS residuals.
Whether a group has a fit at all is the device's rule: X*'X* of every solve must have a Cholesky factorisation whose pivots clear
d^2 > 16 kt eps A_jj (``ratio``: the smallest d^2 / A_jj met).  A group is "decided" when a second implementation must reproduce its
status and n_iter: every ratio above 1e-8, |rho| < 0.99 at every iterate and no |d rho| within a relative 1e-3 of tol -- or no fit
for a reason that does not hang on rounding (no rows, no degrees of freedom, non-finite values).  The edge rules are those of
include/pols_mi355x.h."""
import numpy as np

from iv_ref import pivot_ratio
from ridge_cv_ref import EPS

OK, FALLBACK, EMPTY, NOT_CONVERGED, BAD_DOF = 0, 1, 2, 3, 4
METHODS = ("cochrane_orcutt", "prais_winsten")
DECIDED_RATIO, DECIDED_RHO, DECIDED_TOL = 1e-8, 0.99, 1e-3
F64_FIELDS = ("se", "t_values", "p_values", "cov", "sigma2", "rho", "dw", "dw_ols")


def transform(Z, rho, method):
    """the transformed rows of Z [n, c] at rho"""
    body = Z[1:] - rho * Z[:-1]
    if method == "prais_winsten":
        return np.vstack([np.sqrt(1.0 - rho * rho) * Z[:1], body])
    return body


def rho_of(e):
    """the regression of e_t on e_{t-1} over t = 2..n: (numerator, denominator)"""
    return float(e[1:] @ e[:-1]), float(e[:-1] @ e[:-1])


def _dw(u):
    d = np.diff(u)
    with np.errstate(all="ignore"):
        return float(d @ d) / float(u @ u)


def glsar_group(X, y, method="prais_winsten", max_iter=100, tol=1e-6):
    """One group's rows in time order: X [n, kt] (ones column last where there is one), y [n].  Returns a dict of coef, se, t_values,
    p_values [kt], cov [kt, kt], sigma2, rho, dw, dw_ols, n_iter, status, n, and the margins ratio, rho_max, tol_margin."""
    from scipy import stats

    assert method in METHODS
    n, kt = X.shape
    nstar = n if method == "prais_winsten" else n - 1
    nan = dict(coef=np.full(kt, np.nan), se=np.full(kt, np.nan), t_values=np.full(kt, np.nan), p_values=np.full(kt, np.nan),
               cov=np.full((kt, kt), np.nan), sigma2=np.nan, rho=np.nan, dw=np.nan, dw_ols=np.nan, n_iter=0, status=FALLBACK, n=n,
               ratio=np.inf, rho_max=0.0, tol_margin=np.inf, hard=True)
    if n == 0:
        return dict(nan, coef=np.zeros(kt), status=EMPTY)
    if nstar <= kt:
        return dict(nan, status=BAD_DOF)
    if not (np.isfinite(X).all() and np.isfinite(y).all()):
        return nan
    Z = np.column_stack([X, y])
    rho, n_iter, converged, b0 = 0.0, 0, False, None
    ratio, rho_max, margin = np.inf, 0.0, np.inf
    while True:
        Zs = transform(Z, rho, method)
        Xs, ys = Zs[:, :kt], Zs[:, kt]
        A = Xs.T @ Xs
        if not np.isfinite(A).all():
            return dict(nan, n_iter=n_iter)
        r = pivot_ratio(A)
        ratio = min(ratio, r)
        if not r > 16.0 * kt * EPS:
            # (hard: the rounding noise of an exact singularity, well below the floor)
            return dict(nan, n_iter=n_iter, ratio=ratio, rho_max=rho_max, tol_margin=margin, hard=bool(r < 4.0 * kt * EPS))
        b = np.linalg.lstsq(Xs, ys, rcond=None)[0]
        if not np.isfinite(b).all():
            return dict(nan, n_iter=n_iter, ratio=ratio, hard=False)
        if b0 is None:
            b0 = b
        if converged or n_iter == max_iter:
            break
        e = y - X @ b
        num, den = rho_of(e)
        n_iter += 1
        with np.errstate(all="ignore"):
            new = num / den if den > 0.0 else np.nan
        if not (den > 0.0 and np.isfinite(den)) or not abs(new) < 1.0:
            # (hard: nowhere near the edge of the rule)
            far = np.isfinite(new) and abs(new) > 1.0 / DECIDED_RHO
            return dict(nan, n_iter=n_iter, ratio=ratio, rho_max=max(rho_max, abs(new)) if np.isfinite(new) else np.inf,
                        tol_margin=margin, hard=bool(far))
        step = abs(new - rho)
        margin = min(margin, abs(step - tol) / tol)
        rho_max = max(rho_max, abs(new))
        rho = new
        converged = step <= tol
    e, e0 = y - X @ b, y - X @ b0
    u = transform(e[:, None], rho, method)[:, 0]
    rss = float(u @ u)
    df = nstar - kt
    sigma2 = rss / df
    V = sigma2 * np.linalg.inv(A)
    with np.errstate(all="ignore"):
        se = np.sqrt(np.diagonal(V))
        t = b / se
        p = 2.0 * stats.t.sf(np.abs(t), df)
    return dict(coef=b, se=se, t_values=t, p_values=p, cov=V, sigma2=sigma2, rho=rho, dw=_dw(u), dw_ols=_dw(e0), n_iter=n_iter,
                status=OK if converged else NOT_CONVERGED, n=n, ratio=ratio, rho_max=rho_max, tol_margin=margin, hard=False)


def fill(y, cols, null_policy):
    """the values the entry fits: as they are ("ignore") or with the nulls zero-filled ("zero")"""
    assert null_policy in ("ignore", "zero")
    y = np.asarray(y, dtype=np.float64)
    X = np.column_stack([np.asarray(c, dtype=np.float64) for c in cols]) if len(cols) else np.empty((len(y), 0))
    if null_policy == "zero":
        y, X = np.nan_to_num(y, nan=0.0), np.nan_to_num(X, nan=0.0)
    return y, X


def glsar_batch(y, cols, offsets, method="prais_winsten", max_iter=100, tol=1e-6, add_intercept=False, null_policy="ignore"):
    """Every group of a group-sorted batch.  Returns the fields of glsar_group stacked over the groups (n as ``n_obs``) and ``fit``."""
    offs = np.asarray(offsets, dtype=np.int64)
    G, N = len(offs) - 1, int(offs[-1])
    y, X = fill(y, cols, null_policy)
    if add_intercept:
        X = np.column_stack([X, np.ones(N)])
    kt = X.shape[1]
    out = dict(coef=np.empty((G, kt)), se=np.empty((G, kt)), t_values=np.empty((G, kt)), p_values=np.empty((G, kt)),
               cov=np.empty((G, kt, kt)), sigma2=np.empty(G), rho=np.empty(G), dw=np.empty(G), dw_ols=np.empty(G),
               n_iter=np.zeros(G, dtype=np.int32), status=np.zeros(G, dtype=np.int32), n_obs=np.zeros(G, dtype=np.int64),
               ratio=np.empty(G), rho_max=np.empty(G), tol_margin=np.empty(G), hard=np.zeros(G, dtype=bool), fit=np.ones(N, dtype=bool))
    for g in range(G):
        res = glsar_group(X[offs[g]:offs[g + 1]], y[offs[g]:offs[g + 1]], method, max_iter, tol)
        for key, v in res.items():
            out["n_obs" if key == "n" else key][g] = v
    return out


def decided(ref):
    """the groups whose status and n_iter a second implementation must reproduce"""
    return ref["hard"] | ((ref["ratio"] > DECIDED_RATIO) & (ref["rho_max"] < DECIDED_RHO) & (ref["tol_margin"] > DECIDED_TOL))


def outputs(coef, y, cols, offsets, add_intercept=False, null_policy="ignore"):
    """pred, resid [N] as pols_glsar returns them with the coefficients ``coef`` [G, kt]: x'b on the original scale, features
    zero-filled under "zero"; resid = y - pred with y as it is."""
    offs = np.asarray(offsets, dtype=np.int64)
    N = int(offs[-1])
    y = np.asarray(y, dtype=np.float64)
    X = fill(y, cols, null_policy)[1]
    if add_intercept:
        X = np.column_stack([X, np.ones(N)])
    with np.errstate(all="ignore"):
        pred = (X * np.repeat(coef, np.diff(offs), axis=0)).sum(axis=1)
    return pred, y - pred


def gen_panel_ar1(G, lo, hi, k, dtype, seed=5, sizes=None):
    """Ragged groups of n ~ U{lo..hi} rows (or the given ``sizes``), each a time series: phi ~ U(-0.8, 0.9) per group, errors
    u_t = phi u_{t-1} + N(0, 1) started from the stationary law, regressors x_t = 0.5 x_{t-1} + N(0, 1) (mildly persistent),
    y = x'b + 1 + u with b ~ N(0, 1) per group.  Everything is rounded to ``dtype``.  Returns y, cols, offsets, phi."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, size=G) if sizes is None else np.asarray(sizes, dtype=np.int64)
    G = len(sizes)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    phi = rng.uniform(-0.8, 0.9, size=G)
    beta = rng.normal(size=(G, k))
    X, u = np.empty((n, k)), np.empty(n)
    ex, eu = rng.normal(size=(n, k)), rng.normal(size=n)
    for g in range(G):
        a, b = offs[g], offs[g + 1]
        if b == a:
            continue
        X[a], u[a] = ex[a] / np.sqrt(0.75), eu[a] / np.sqrt(1.0 - phi[g] ** 2)
        for t in range(a + 1, b):
            X[t] = 0.5 * X[t - 1] + ex[t]
            u[t] = phi[g] * u[t - 1] + eu[t]
    gid = np.repeat(np.arange(G), sizes)
    y = (X * beta[gid]).sum(axis=1) + 1.0 + u
    X = X.astype(dtype)
    return y.astype(dtype), [np.ascontiguousarray(X[:, j]) for j in range(k)], offs, phi


def tile_edge_sizes():
    """group lengths that put a lag pair on every side of a tile boundary, odd fillers between so that the group starts meet every
    alignment of the 16-byte grid"""
    sizes = []
    for rep, filler in enumerate((5, 7, 9, 11)):
        for n in (2, 3, 255, 256, 257, 511, 512, 513, 769):
            sizes += [n, filler + 2 * (len(sizes) % 3) + rep]
    return np.array(sizes, dtype=np.int64)


# name: (groups, fewest rows, most rows, features, SEG_TARGET, seed) -- the frames of tests/test_glsar_gpu.py, all with an intercept
SHAPES = {
    "short_k1": (200, 8, 60, 1, None, 6),
    "short_k2": (200, 8, 60, 2, None, 11),
    "short_k3": (200, 8, 60, 3, None, 8),
    "tile_edges": (None, None, None, 3, None, 9),
    "segmented": (40, 600, 1500, 3, 256, 5),
    "long": (3, 5000, 9000, 3, 1024, 5),
    "at_cap": (12, 100, 300, 30, None, 5),
}


def frame(shape, dtype):
    G, lo, hi, k, _, seed = SHAPES[shape]
    return gen_panel_ar1(G, lo, hi, k, dtype, seed, sizes=tile_edge_sizes() if shape == "tile_edges" else None)


def edge_frame(dtype):
    """Ordinary groups with the edge groups between them, 2 features + intercept (kt = 3): group 1 is empty, 2 has one row, 4 has
    kt + 1 rows, 5 an exactly duplicated column, 6 an explosive series y_t ~ 1.05^t on noise regressors.  Returns y, cols, offsets."""
    kt = 3
    sizes = np.array([90, 0, 1, 70, kt + 1, 80, 64, 75, 60, 85])
    y, cols, offs, _ = gen_panel_ar1(len(sizes), 0, 0, 2, np.float64, 23, sizes=sizes)
    y4, cols4, _, _ = gen_panel_ar1(1, kt + 1, kt + 1, 2, np.float64, 0)   # (four rows whose Prais-Winsten iteration is decided)
    y[offs[4]:offs[5]] = y4
    for c, c4 in zip(cols, cols4):
        c[offs[4]:offs[5]] = c4
    cols[1][offs[5]:offs[6]] = cols[0][offs[5]:offs[6]]
    a, b = offs[6], offs[7]
    rng = np.random.default_rng(24)
    y[a:b] = 1.05 ** np.arange(1, b - a + 1) * (1.0 + 0.01 * rng.normal(size=b - a))
    return y.astype(dtype), [c.astype(dtype) for c in cols], offs


def null_frame():
    """8 f64 groups with NaNs in y (group 1), in a feature (3, 5) and in a group's first row (6).  Returns y, cols, offsets."""
    y, cols, offs, _ = gen_panel_ar1(8, 80, 140, 2, np.float64, 31)
    rng = np.random.default_rng(32)
    for g, a in ((1, y), (3, cols[0]), (5, cols[1])):
        a[offs[g] + rng.choice(offs[g + 1] - offs[g], size=3, replace=False)] = np.nan
    cols[1][offs[6]] = np.nan
    return y, cols, offs
