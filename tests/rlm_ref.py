"""numpy restatement of the Huber / bisquare M-estimator per group (pols_rlm, K11): the yardstick of tests/test_rlm_*.py.  Per group,
f64, on the fitted rows F (ridge_cv_ref.fit_rows: the rows pols_least_squares fits) scaled by sqrt(w) with the ones column last:
    b0 = OLS on F;  r = y - X b;  s = median(|r|) / 0.6744897501960817;  omega = psi(u) / u at u = |r| / s
    (huber: 1 for u <= c, else c / u;  bisquare: (1 - (u / c)^2)^2 for u < c, else 0);  b <- (X' diag(omega) X)^-1 X' diag(omega) y
until max_j |b_new - b| <= tol max(max_j |b_new|, 1e-300) or ``max_iter`` updates.  Every solve is a Cholesky factorisation whose
pivots must clear the project's floor (ridge_cv_ref._cholesky_inverse: d^2 > 16 k eps A_jj).  The edge rules -- empty groups, n <= kt,
a start or an update that does not factor or is not finite, the collapse of the scale -- are those of include/pols_mi355x.h."""
import numpy as np

from ridge_cv_ref import EPS, _cholesky_inverse, fit_rows

OK, FALLBACK, EMPTY, NOT_CONVERGED = 0, 1, 2, 3
MAD = 0.6744897501960817
HUBER_C, BISQUARE_C = 1.345, 4.685
NORMS = ("huber", "bisquare")


def default_c(norm):
    return HUBER_C if norm == "huber" else BISQUARE_C


def omega(u, norm, c):
    """psi(u) / u"""
    with np.errstate(all="ignore"):
        if norm == "huber":
            return np.where(u <= c, 1.0, c / np.where(u <= c, 1.0, u))
        return np.where(u < c, (1.0 - (u / c) ** 2) ** 2, 0.0)


def wls(X, y, om):
    """the solution of (X' diag(om) X) b = X' diag(om) y by the project's Cholesky rule, or None"""
    with np.errstate(all="ignore"):
        Xo = X * om[:, None]
        A, g = Xo.T @ X, Xo.T @ y
        Li, ok = _cholesky_inverse(A[None])
        if not ok[0]:
            return None
        b = Li[0].T @ (Li[0] @ g)
    return b if np.isfinite(b).all() else None


def scale_of(X, y, b):
    """(s, |r|) at the coefficients b"""
    with np.errstate(all="ignore"):
        r = np.abs(y - X @ b)
        return np.median(r) / MAD, r


def rlm_group(X, y, norm="huber", c=None, max_iter=50, tol=1e-8):
    """One group's scaled fitted rows X [n, kt], y [n].  Returns dict(coef, scale, n_iter, status, weights [n], step): ``step`` is
    the last max_j |b_new - b| over its threshold tol max(max_j |b_new|, 1e-300) (NaN when no update was made)."""
    n, kt = X.shape
    c = default_c(norm) if c is None or c <= 0 else c
    nan = dict(coef=np.full(kt, np.nan), scale=np.nan, n_iter=0, status=FALLBACK, weights=np.full(n, np.nan), step=np.nan)
    if n == 0:
        return dict(nan, coef=np.zeros(kt), status=EMPTY)
    if n <= kt:
        return nan
    b = wls(X, y, np.ones(n))
    if b is None:
        return nan
    with np.errstate(all="ignore"):
        ymax = np.abs(y).max()
    om, it, step, status = np.ones(n), 0, np.nan, OK
    while True:
        s, r = scale_of(X, y, b)
        if not (s > 16.0 * EPS * ymax) or not np.isfinite(s):      # the scale collapsed: converged where it is
            break
        om_new = omega(r / s, norm, c)
        b_new = wls(X, y, om_new)
        if b_new is None:
            return dict(nan, n_iter=it)
        om = om_new
        it += 1
        d, thr = np.abs(b_new - b).max(), tol * max(np.abs(b_new).max(), 1e-300)
        b, step = b_new, d / thr
        if d <= thr:
            break
        if it >= max_iter:
            status = NOT_CONVERGED
            break
    return dict(coef=b, scale=s, n_iter=it, status=status, weights=om, step=step)


def rlm_batch(y, cols, offsets, norm="huber", c=None, max_iter=50, tol=1e-8, weights=None, add_intercept=False, null_policy="ignore",
              valid=None):
    """Every group of a group-sorted batch.  Returns coef [G, kt], scale, n_iter, status, step [G], weights [N] (NaN outside the
    fit), ``fit`` [N], n [G] and the scaled design ``Xs`` [N, kt], ``ys`` [N] the fit ran on."""
    offs = np.asarray(offsets, dtype=np.int64)
    G, N = len(offs) - 1, int(offs[-1])
    y = np.asarray(y, dtype=np.float64)
    X = np.column_stack([np.asarray(col, dtype=np.float64) for col in cols])
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    fit, y, X, w = fit_rows(y, X, w, null_policy, valid)
    if add_intercept:
        X = np.column_stack([X, np.ones(N)])
    kt = X.shape[1]
    sw = np.ones(N) if w is None else np.sqrt(w)
    Xs, ys = X * sw[:, None], y * sw
    out = dict(coef=np.empty((G, kt)), scale=np.empty(G), n_iter=np.zeros(G, dtype=np.int32), status=np.zeros(G, dtype=np.int32),
               step=np.empty(G), weights=np.full(N, np.nan), fit=fit, n=np.zeros(G, dtype=np.int64), Xs=Xs, ys=ys)
    for g in range(G):
        rows = np.arange(offs[g], offs[g + 1])[fit[offs[g]:offs[g + 1]]]
        res = rlm_group(Xs[rows], ys[rows], norm, c, max_iter, tol)
        out["coef"][g], out["scale"][g], out["n_iter"][g] = res["coef"], res["scale"], res["n_iter"]
        out["status"][g], out["step"][g], out["n"][g] = res["status"], res["step"], len(rows)
        out["weights"][rows] = res["weights"]
    return out


def outputs(coef, fit, y, cols, offsets, add_intercept=False, null_policy="ignore"):
    """pred [N], resid [N] as pols_least_squares returns them with the coefficients ``coef`` [G, kt]: features zero-filled for every
    policy but "ignore", "drop" masks the rows outside the fit with NaN."""
    offs = np.asarray(offsets, dtype=np.int64)
    N = int(offs[-1])
    y = np.asarray(y, dtype=np.float64)
    X = np.column_stack([np.asarray(col, dtype=np.float64) for col in cols])
    if null_policy != "ignore":
        X = np.nan_to_num(X, nan=0.0)
    if add_intercept:
        X = np.column_stack([X, np.ones(N)])
    with np.errstate(all="ignore"):
        pred = (X * np.repeat(coef, np.diff(offs), axis=0)).sum(axis=1)
    if null_policy == "drop":
        pred = np.where(fit, pred, np.nan)
    return pred, y - pred


def decided(ref, max_iter):
    """the groups whose status and n_iter a second implementation must reproduce: converged with at least two iterations to spare,
    or not converged with a last step above 10 x its threshold; groups that did not iterate (empty, no fit) count as decided"""
    st, it, step = ref["status"], ref["n_iter"], ref["step"]
    with np.errstate(all="ignore"):
        return np.where(st == OK, it <= max_iter - 2, np.where(st == NOT_CONVERGED, step > 10.0, True))


def gen_panel(G, lo, hi, kt, dtype, seed=5, shift=(3.0, 10.0), share=0.1):
    """Ragged groups of n ~ U{lo..hi} rows; the last of the kt columns is the intercept (kt - 1 feature columns come back, fit with
    add_intercept=True).  y = X beta + 0.3 N(0, 1), then ``share`` of the rows shifted by +-U(shift).  Returns y, cols, offsets,
    sample weights ~ U(0.2, 2) and the true beta [G, kt]."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, size=G)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    X = rng.normal(size=(n, kt))
    X[:, kt - 1] = 1.0
    beta = rng.normal(size=(G, kt))
    y = (X * np.repeat(beta, sizes, axis=0)).sum(axis=1) + 0.3 * rng.normal(size=n)
    out = rng.random(n) < share
    y = y + np.where(out, rng.choice([-1.0, 1.0], size=n) * rng.uniform(shift[0], shift[1], size=n), 0.0)
    w = rng.uniform(0.2, 2.0, size=n)
    return y.astype(dtype), [X[:, j].astype(dtype) for j in range(kt - 1)], offs, w.astype(dtype), beta
