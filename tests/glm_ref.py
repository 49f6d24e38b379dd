"""numpy restatement of the logistic / Poisson generalised linear model per group (pols_glm, K13): the yardstick of tests/test_glm_*.py.
Per group, f64, on the fitted rows F (ridge_cv_ref.fit_rows: the rows pols_least_squares fits; a null offset counts as a null
feature) with the ones column last, prior weights w and offsets o:
    mu0 = (y + 0.5) / 2 | y + 0.1;  eta0 = logit(mu0) | log(mu0);  D0 = D(mu0);
    W = w d(mu);  z = eta - o + (y - mu) / d(mu);  b <- (X' diag(W) X)^-1 X' diag(W) z;  eta = X b + o;  mu = g^-1(eta) clipped;
    D = 2 sum w u(y, mu)
until |D_new - D| <= tol (|D_new| + 0.1) or ``max_iter`` updates.  Every solve is a Cholesky factorisation whose pivots must clear the
project's floor (ridge_cv_ref._cholesky_inverse: d^2 > 16 k eps A_jj).  The edge rules -- empty groups, n <= kt, y outside the
family's domain, non-finite values, an update that does not factor or is not finite -- are those of include/pols_mi355x.h."""
import numpy as np

from ridge_cv_ref import EPS, _cholesky_inverse, fit_rows

OK, FALLBACK, EMPTY, NOT_CONVERGED = 0, 1, 2, 3
FAMILIES = ("binomial", "poisson")


def mean(eta, family):
    """(mu, d(mu)) at the linear predictor eta"""
    with np.errstate(all="ignore"):
        if family == "binomial":
            mu = np.clip(1.0 / (1.0 + np.exp(-eta)), EPS, 1.0 - EPS)
            return mu, mu * (1.0 - mu)
        mu = np.maximum(np.exp(eta), EPS)
        return mu, mu


def variance(mu, family):
    return mu * (1.0 - mu) if family == "binomial" else mu


def start(y, family):
    """(mu0, eta0)"""
    with np.errstate(all="ignore"):
        if family == "binomial":
            mu = (y + 0.5) / 2.0
            return mu, np.log(mu / (1.0 - mu))
        mu = y + 0.1
        return mu, np.log(mu)


def _xlogy(y, r):
    """y log(r) with 0 log 0 = 0"""
    with np.errstate(all="ignore"):
        return np.where(y > 0.0, y * np.log(np.where(y > 0.0, r, 1.0)), 0.0)


def deviance(y, mu, w, family):
    with np.errstate(all="ignore"):
        if family == "binomial":
            u = _xlogy(y, y / mu) + _xlogy(1.0 - y, (1.0 - y) / (1.0 - mu))
        else:
            u = _xlogy(y, y / mu) - (y - mu)
        return 2.0 * float((w * u).sum())


def in_domain(y, family):
    return (y >= 0.0) & (y <= 1.0) if family == "binomial" else y >= 0.0


def glm_group(X, y, w, o, family="binomial", max_iter=25, tol=1e-8):
    """One group's fitted rows X [n, kt], y, w, o [n].  Returns dict(coef, se, deviance, n_iter, status, ratios): ``ratios`` lists every
    step's |D_new - D| / (tol (|D_new| + 0.1)), the stop test's left side over its right side."""
    n, kt = X.shape
    nan = dict(coef=np.full(kt, np.nan), se=np.full(kt, np.nan), deviance=np.nan, n_iter=0, status=FALLBACK, ratios=[])
    if n == 0:
        return dict(nan, coef=np.zeros(kt), status=EMPTY)
    if n <= kt:
        return nan
    if not (np.isfinite(X).all() and np.isfinite(y).all() and np.isfinite(w).all() and np.isfinite(o).all()):
        return nan
    if not in_domain(y, family).all():
        return nan
    mu, eta = start(y, family)
    d = variance(mu, family)
    D = deviance(y, mu, w, family)
    if not np.isfinite(D):
        return nan
    it, status, ratios = 0, OK, []
    while True:
        with np.errstate(all="ignore"):
            W = w * d
            z = eta - o + (y - mu) / d
            XW = X * W[:, None]
            Li, ok = _cholesky_inverse((XW.T @ X)[None])
            if not ok[0]:
                return dict(nan, n_iter=it, ratios=ratios)
            b = Li[0].T @ (Li[0] @ (XW.T @ z))
            if not np.isfinite(b).all():
                return dict(nan, n_iter=it, ratios=ratios)
            se = np.sqrt((Li[0] * Li[0]).sum(axis=0))
            eta = X @ b + o
            mu, d = mean(eta, family)
            Dn = deviance(y, mu, w, family)
        it += 1
        if not np.isfinite(Dn):
            return dict(nan, n_iter=it, ratios=ratios)
        thr = tol * (abs(Dn) + 0.1)
        ratios.append(abs(Dn - D) / thr)
        conv = abs(Dn - D) <= thr
        D = Dn
        if conv:
            break
        if it >= max_iter:
            status = NOT_CONVERGED
            break
    return dict(coef=b, se=se, deviance=D, n_iter=it, status=status, ratios=ratios)


def glm_batch(y, cols, offsets, family="binomial", offset=None, max_iter=25, tol=1e-8, weights=None, add_intercept=False,
              null_policy="ignore", valid=None):
    """Every group of a group-sorted batch.  Returns coef, se [G, kt], deviance, n_iter, status, n [G], ``ratios`` (a list per group)
    and ``fit`` [N]."""
    offs = np.asarray(offsets, dtype=np.int64)
    G, N = len(offs) - 1, int(offs[-1])
    y = np.asarray(y, dtype=np.float64)
    X = np.column_stack([np.asarray(col, dtype=np.float64) for col in cols])
    ku = X.shape[1]
    if offset is not None:                                         # a null offset is a null feature
        X = np.column_stack([X, np.asarray(offset, dtype=np.float64)])
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    fit, y, X, w = fit_rows(y, X, w, null_policy, valid)
    o = X[:, ku] if offset is not None else np.zeros(N)
    X = X[:, :ku]
    if add_intercept:
        X = np.column_stack([X, np.ones(N)])
    kt = X.shape[1]
    w = np.ones(N) if w is None else w
    out = dict(coef=np.empty((G, kt)), se=np.empty((G, kt)), deviance=np.empty(G), n_iter=np.zeros(G, dtype=np.int32),
               status=np.zeros(G, dtype=np.int32), n=np.zeros(G, dtype=np.int64), ratios=[], fit=fit)
    for g in range(G):
        rows = np.arange(offs[g], offs[g + 1])[fit[offs[g]:offs[g + 1]]]
        res = glm_group(X[rows], y[rows], w[rows], o[rows], family, max_iter, tol)
        out["coef"][g], out["se"][g], out["deviance"][g] = res["coef"], res["se"], res["deviance"]
        out["n_iter"][g], out["status"][g], out["n"][g] = res["n_iter"], res["status"], len(rows)
        out["ratios"].append(res["ratios"])
    return out


def outputs(coef, fit, y, cols, offsets, family, offset=None, add_intercept=False, null_policy="ignore"):
    """linpred, pred, resid [N] as pols_glm returns them with the coefficients ``coef`` [G, kt]: features and offsets zero-filled for
    every policy but "ignore", "drop" masks the rows outside the fit with NaN."""
    offs = np.asarray(offsets, dtype=np.int64)
    N = int(offs[-1])
    y = np.asarray(y, dtype=np.float64)
    X = np.column_stack([np.asarray(col, dtype=np.float64) for col in cols])
    o = np.zeros(N) if offset is None else np.asarray(offset, dtype=np.float64)
    if null_policy != "ignore":
        X, o = np.nan_to_num(X, nan=0.0), np.nan_to_num(o, nan=0.0)
    if add_intercept:
        X = np.column_stack([X, np.ones(N)])
    with np.errstate(all="ignore"):
        eta = (X * np.repeat(coef, np.diff(offs), axis=0)).sum(axis=1) + o
    if null_policy == "drop":
        eta = np.where(fit, eta, np.nan)
    mu, _ = mean(eta, family)
    return eta, mu, y - mu


def decided(ref):
    """the groups whose status and n_iter a second implementation must reproduce: no step's stop ratio lies in [0.5, 2]"""
    return np.array([not any(0.5 <= r <= 2.0 for r in rs) for rs in ref["ratios"]], dtype=bool)


def gen_panel_glm(G, lo, hi, kt, dtype, family, seed=5):
    """Ragged groups of n ~ U{lo..hi} rows; the last of the kt columns is the intercept (kt - 1 feature columns come back, fit with
    add_intercept=True).  Features N(0, 1), true coefficients 0.5 N(0, 1) / sqrt(kt - 1) per group, intercept 0 (binomial) / 1
    (Poisson), offsets 0.3 N(0, 1), prior weights U(0.5, 2), everything rounded to ``dtype`` first; y drawn from the family at
    eta = x'beta + intercept + offset.  Returns y, cols, offsets, weights, offset."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, size=G)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    X = rng.normal(size=(n, kt - 1)).astype(dtype)
    beta = 0.5 * rng.normal(size=(G, kt - 1)) / np.sqrt(kt - 1)
    off = (0.3 * rng.normal(size=n)).astype(dtype)
    w = rng.uniform(0.5, 2.0, size=n).astype(dtype)
    eta = (X.astype(np.float64) * np.repeat(beta, sizes, axis=0)).sum(axis=1) + off.astype(np.float64) + (0.0 if family == "binomial" else 1.0)
    if family == "binomial":
        y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(dtype)
    else:
        y = rng.poisson(np.exp(eta)).astype(dtype)
    return y, [np.ascontiguousarray(X[:, j]) for j in range(kt - 1)], offs, w, off
