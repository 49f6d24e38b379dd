"""numpy restatement of per-group two-stage least squares with diagnostics (pols_iv2sls, K14): the yardstick of tests/test_iv_*.py.
Per group, f64, on the fitted rows F (ridge_cv_ref.fit_rows with the excluded instruments counted as features) scaled by sqrt(w):
X = [X1 | X2 | 1] (the last n_endog user columns endogenous), Z = [X1 | 1 | Z2].  Both stages run by np.linalg.lstsq on the rows --
X^ = Z lstsq(Z, X), b = lstsq(X^, y) -- and NOT through the cross-moments the device uses:
    e = y - X b (the actual regressors),  RSS = e'e,  M = X^'X^,
    V = sigma2 M^-1  |  M^-1 (X^' diag(e^2) X^) M^-1 (HC0)  |  that x n / df (HC1),   df = n - kt (small_sample) or n,
    first stage of x2j: RSS_r from lstsq on [X1 | 1], RSS_u from lstsq on Z, F = ((RSS_r - RSS_u) / m) / (RSS_u / (n - L)),
    partial R2 = 1 - RSS_u / RSS_r,   Sargan = n |Z lstsq(Z, e)|^2 / RSS with scipy's chi2(m - n_endog) tail.
Whether a group has a fit at all is the device's rule: Z'Z and M must have a Cholesky factorisation whose pivots clear the project's
floor d^2 > 16 dim eps A_jj (``pivot_ratio`` reports the smallest d^2 / A_jj met; a group is "decided" when it is above 1e-8 or the
group fails).  The edge rules -- empty groups, n <= L, non-finite values -- are those of include/pols_mi355x.h."""
import numpy as np

from ridge_cv_ref import EPS, fit_rows

OK, FALLBACK, EMPTY, BAD_DOF = 0, 1, 2, 4
COV_TYPES = ("nonrobust", "HC0", "HC1")
DECIDED_RATIO = 1e-8
F64_FIELDS = ("se", "t_values", "p_values", "cov", "sigma2", "first_stage_f", "partial_r2", "sargan", "sargan_p")


def pivot_ratio(A):
    """the smallest d_j^2 / A_jj of the Cholesky factorisation of A (0.0 where a pivot is not positive)"""
    A = np.array(A, dtype=np.float64)
    k = A.shape[0]
    diag = np.diagonal(A).copy()
    worst = np.inf
    for j in range(k):
        d = A[j, j]
        if not (d > 0.0 and diag[j] > 0.0):
            return 0.0
        worst = min(worst, d / diag[j])
        A[j:, j] /= np.sqrt(d)
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return float(worst)


def split(X, Z2, n_endog, icpt):
    """(Z1, Z): the included instruments [X1 | 1] and all of them [X1 | 1 | Z2] of the regressors X = [X1 | X2 | 1]"""
    kt = X.shape[1]
    k1 = kt - int(icpt) - n_endog
    Z1 = np.column_stack([X[:, :k1], X[:, kt - 1:]]) if icpt else X[:, :k1]
    return Z1, np.column_stack([Z1, Z2])


def _rss(A, y):
    if A.shape[1] == 0:
        return float(y @ y)
    r = y - A @ np.linalg.lstsq(A, y, rcond=None)[0]
    return float(r @ r)


def iv_group(X, Z2, y, n_endog, icpt, cov_type="nonrobust", small_sample=True):
    """One group's scaled fitted rows: X [n, kt] (ones column last when ``icpt``), Z2 [n, m], y [n].  Returns a dict of coef, se,
    t_values, p_values [kt], cov [kt, kt], sigma2, first_stage_f, partial_r2 [n_endog], sargan, sargan_p, status, n, ratio."""
    from scipy import stats

    n, kt = X.shape
    m = Z2.shape[1]
    L = kt - n_endog + m
    nan = dict(coef=np.full(kt, np.nan), se=np.full(kt, np.nan), t_values=np.full(kt, np.nan), p_values=np.full(kt, np.nan),
               cov=np.full((kt, kt), np.nan), sigma2=np.nan, first_stage_f=np.full(n_endog, np.nan), partial_r2=np.full(n_endog, np.nan),
               sargan=np.nan, sargan_p=np.nan, status=FALLBACK, n=n, ratio=0.0)
    if n == 0:
        return dict(nan, coef=np.zeros(kt), status=EMPTY)
    if n <= L:
        return dict(nan, status=BAD_DOF)
    if not (np.isfinite(X).all() and np.isfinite(Z2).all() and np.isfinite(y).all()):
        return nan
    Z1, Z = split(X, Z2, n_endog, icpt)
    ratio = pivot_ratio(Z.T @ Z)
    if not ratio > 16.0 * L * EPS:
        return dict(nan, ratio=ratio)
    Xh = Z @ np.linalg.lstsq(Z, X, rcond=None)[0]
    M = Xh.T @ Xh
    ratio = min(ratio, pivot_ratio(M))
    if not pivot_ratio(M) > 16.0 * kt * EPS:
        return dict(nan, ratio=ratio)
    b = np.linalg.lstsq(Xh, y, rcond=None)[0]
    e = y - X @ b
    rss = float(e @ e)
    df = n - kt if small_sample else n
    Mi = np.linalg.inv(M)
    if cov_type == "nonrobust":
        V = rss / df * Mi
    else:
        V = Mi @ ((Xh * (e * e)[:, None]).T @ Xh) @ Mi
        if cov_type == "HC1":
            V = V * (n / df)
    with np.errstate(all="ignore"):
        se = np.sqrt(np.diagonal(V))
        t = b / se
        p = 2.0 * stats.t.sf(np.abs(t), df) if small_sample else 2.0 * stats.norm.sf(np.abs(t))
    k1 = kt - int(icpt) - n_endog
    F, pr2 = np.empty(n_endog), np.empty(n_endog)
    for j in range(n_endog):
        x = X[:, k1 + j]
        rr, ru = _rss(Z1, x), _rss(Z, x)
        F[j] = ((rr - ru) / m) / (ru / (n - L))
        pr2[j] = (rr - ru) / rr
    sargan = sargan_p = np.nan
    if m > n_endog:
        eh = Z @ np.linalg.lstsq(Z, e, rcond=None)[0]
        sargan = n * float(eh @ eh) / rss
        sargan_p = float(stats.chi2.sf(sargan, m - n_endog))
    return dict(coef=b, se=se, t_values=t, p_values=p, cov=V, sigma2=rss / df, first_stage_f=F, partial_r2=pr2, sargan=sargan,
                sargan_p=sargan_p, status=OK, n=n, ratio=ratio)


def iv_batch(y, cols, z_cols, offsets, n_endog, cov_type="nonrobust", small_sample=True, weights=None, add_intercept=False,
             null_policy="ignore", valid=None):
    """Every group of a group-sorted batch; ``cols`` = exogenous then endogenous regressors, ``z_cols`` the excluded instruments.
    Returns the fields of iv_group stacked over the groups (n as ``n_obs``), and ``fit`` [N]."""
    offs = np.asarray(offsets, dtype=np.int64)
    G, N = len(offs) - 1, int(offs[-1])
    y = np.asarray(y, dtype=np.float64)
    ku, m = len(cols), len(z_cols)
    XZ = np.column_stack([np.asarray(c, dtype=np.float64) for c in list(cols) + list(z_cols)])
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    fit, y, XZ, w = fit_rows(y, XZ, w, null_policy, valid)     # a null instrument is a null feature
    sw = np.ones(N) if w is None else np.sqrt(w)
    X, Z2 = XZ[:, :ku], XZ[:, ku:]
    if add_intercept:
        X = np.column_stack([X, np.ones(N)])
    kt = X.shape[1]
    with np.errstate(all="ignore"):
        X, Z2, y = X * sw[:, None], Z2 * sw[:, None], y * sw
    out = dict(coef=np.empty((G, kt)), se=np.empty((G, kt)), t_values=np.empty((G, kt)), p_values=np.empty((G, kt)),
               cov=np.empty((G, kt, kt)), sigma2=np.empty(G), first_stage_f=np.empty((G, n_endog)), partial_r2=np.empty((G, n_endog)),
               sargan=np.empty(G), sargan_p=np.empty(G), status=np.zeros(G, dtype=np.int32), n_obs=np.zeros(G, dtype=np.int64),
               ratio=np.empty(G), fit=fit)
    for g in range(G):
        rows = np.arange(offs[g], offs[g + 1])[fit[offs[g]:offs[g + 1]]]
        res = iv_group(X[rows], Z2[rows], y[rows], n_endog, add_intercept, cov_type, small_sample)
        for key, v in res.items():
            out["n_obs" if key == "n" else key][g] = v
    return out


def decided(ref):
    """the groups whose status a second implementation must reproduce: every pivot ratio above 1e-8, or no fit at all"""
    return (ref["ratio"] > DECIDED_RATIO) | (ref["status"] != OK)


def outputs(coef, fit, y, cols, offsets, weights=None, add_intercept=False, null_policy="ignore"):
    """pred, resid [N] as pols_iv2sls returns them with the coefficients ``coef`` [G, kt]: x'b from the actual regressors, features
    zero-filled for every policy but "ignore", "drop" masks the rows outside the fit with NaN, a zero weight gives NaN (the
    prediction is (sqrt(w) x)'b / sqrt(w))."""
    offs = np.asarray(offsets, dtype=np.int64)
    N = int(offs[-1])
    y = np.asarray(y, dtype=np.float64)
    X = np.column_stack([np.asarray(c, dtype=np.float64) for c in cols])
    if null_policy != "ignore":
        X = np.nan_to_num(X, nan=0.0)
    if add_intercept:
        X = np.column_stack([X, np.ones(N)])
    with np.errstate(all="ignore"):
        pred = (X * np.repeat(coef, np.diff(offs), axis=0)).sum(axis=1)
        if weights is not None:
            sw = np.sqrt(np.where(np.isnan(weights), 1e-24, np.asarray(weights, dtype=np.float64)))
            pred = (pred * sw) * (1.0 / sw)
    if null_policy == "drop":
        pred = np.where(fit, pred, np.nan)
    return pred, y - pred


def gen_panel_iv(G, lo, hi, n_exog, n_endog, m, dtype, seed=5, strength=0.6):
    """Ragged groups of n ~ U{lo..hi} rows.  Per group: exogenous X1 ~ N(0, 1) [n_exog], instruments Z2 ~ N(0, 1) [m] independent of
    the structural error u; the endogenous regressors X2 = Z2 P + 0.3 X1 Q + v with v = 0.6 u + 0.8 N(0, 1) (the shared error makes
    them endogenous), P = strength N(0, 1) + a diagonal of 1; y = X1 b1 + X2 b2 + 1 + u.  Everything is rounded to ``dtype`` first.
    Returns y, cols (exogenous then endogenous), z_cols, offsets, weights U(0.5, 2)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, size=G)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    gid = np.repeat(np.arange(G), sizes)
    X1 = rng.normal(size=(n, n_exog))
    Z2 = rng.normal(size=(n, m))
    u = rng.normal(size=n)
    P = strength * rng.normal(size=(G, m, n_endog))
    P[:, np.arange(n_endog), np.arange(n_endog)] += 1.0
    Q = 0.3 * rng.normal(size=(G, n_exog, n_endog))
    v = 0.6 * u[:, None] + 0.8 * rng.normal(size=(n, n_endog))
    X2 = np.einsum("nm,nme->ne", Z2, P[gid]) + np.einsum("nk,nke->ne", X1, Q[gid]) + v
    b1, b2 = rng.normal(size=(G, n_exog)), rng.normal(size=(G, n_endog))
    y = (X1 * b1[gid]).sum(axis=1) + (X2 * b2[gid]).sum(axis=1) + 1.0 + u
    w = rng.uniform(0.5, 2.0, size=n).astype(dtype)
    X = np.column_stack([X1, X2]).astype(dtype)
    Z2 = Z2.astype(dtype)
    return (y.astype(dtype), [np.ascontiguousarray(X[:, j]) for j in range(n_exog + n_endog)],
            [np.ascontiguousarray(Z2[:, j]) for j in range(m)], offs, w)


# name: (groups, fewest rows, most rows, user exogenous, endogenous, instruments, intercept, SEG_TARGET) -- the frames of tests/test_iv_gpu.py
SHAPES = {
    "just_identified": (200, 8, 60, 0, 1, 1, False, None),
    "short": (200, 24, 120, 2, 1, 3, True, None),
    "several_tiles": (40, 300, 700, 3, 2, 4, True, None),          # (odd group lengths: groups start off the 16-byte grid)
    "many_endog": (40, 100, 300, 1, 6, 6, True, None),             # exactly identified: Sargan NaN
    "at_cap": (12, 100, 300, 9, 4, 17, True, None),                # T = 9 + 4 + 1 + 17 = 31
    "segmented": (40, 600, 1500, 3, 2, 4, True, 256),              # 3 - 6 segments a group
    "long": (3, 5000, 9000, 2, 1, 3, True, 1024),
    "two_entries_robust": (12, 100, 300, 21, 1, 2, True, None),    # kx = 23: 276 score-matrix entries, two slots of the spread
}
