"""numpy restatement of the ridge regularisation path with leave-one-out selection (pols_ridge_cv, K10): the yardstick of
tests/test_ridge_cv_*.py.  Per group, f64, on the fitted rows F scaled by sqrt(w) with the ones column last and penalised like any
other: for every candidate a, A = X'X + a I over F, b = A^-1 X'y, h_i = x_i' A^-1 x_i and
    score = (1 / n) sum_F ((y_i - x_i'b) / (1 - h_i))^2.
A candidate is unusable (NaN score, NaN coefficients) when A has no Cholesky factorisation -- np.linalg.cholesky raises, or a pivot
d_j^2 is within 16 k eps of A_jj: rounding noise around the exact 0 of a singular matrix, the rule of the project's own f64 Cholesky
(fix_chol_solve) -- when a fitted row has 1 - h_i < 1e-10, or when the score is not finite.  The chosen candidate is the usable one
with the smallest score, the lowest index on a tie.  Groups of equal length are evaluated as stacks."""
import numpy as np

HIGH_LEVERAGE = 1e-10
EPS = np.finfo(np.float64).eps
OK, FALLBACK, EMPTY = 0, 1, 2
DROP_X = ("drop", "drop_zero", "drop_window")
DROP_Y = DROP_X + ("drop_y_zero_x",)


def fit_rows(y, X, w, null_policy="ignore", valid=None):
    """(fit mask [N], y, X, w as the policy leaves them): the rows pols_least_squares fits.  A null is a NaN; the drop family
    also drops the rows whose validity byte is 0; every policy but "ignore" turns the nulls that stay into 0; a null weight acts
    as 1e-24 under every policy."""
    N = len(y)
    fit = np.ones(N, dtype=bool)
    if null_policy in DROP_Y:
        if valid is not None:
            fit &= np.asarray(valid).astype(bool)
        fit &= ~np.isnan(y)
    if null_policy in DROP_X:
        fit &= ~np.isnan(X).any(axis=1)
    if null_policy != "ignore":
        y, X = np.nan_to_num(y, nan=0.0), np.nan_to_num(X, nan=0.0)
    if w is not None:
        w = np.where(np.isnan(w), 1e-24, w)
    return fit, y, X, w


def _cholesky_inverse(A):
    """(L^-1, ok) of a stack of matrices; ok False where the factorisation fails or a pivot is noise"""
    B, k, _ = A.shape
    Li, ok = np.zeros_like(A), np.zeros(B, dtype=bool)

    def one(M):
        if not np.isfinite(M).all():
            return None
        try:
            L = np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            return None
        d = np.diagonal(L, axis1=-2, axis2=-1)
        good = (d * d > 16.0 * k * EPS * np.diagonal(M, axis1=-2, axis2=-1)).all(axis=-1)
        return L, good

    r = one(A)
    if r is not None:
        L, good = r
        ok[:] = good
        Li[good] = np.linalg.inv(L[good])
        return Li, ok
    for i in range(B):
        r = one(A[i])
        if r is not None and r[1]:
            Li[i], ok[i] = np.linalg.inv(r[0]), True
    return Li, ok


def _stack(Xf, yf, m, alphas):
    """B groups of n rows, the rows outside the fit zeroed: Xf [B, n, k], yf [B, n], m [B, n] bool.  Returns cv_scores [B, na] and
    coef_path [B, na, k]."""
    B, n, k = Xf.shape
    nn = m.sum(axis=1).astype(np.float64)
    G = np.einsum("bni,bnj->bij", Xf, Xf)
    c = np.einsum("bni,bn->bi", Xf, yf)
    scores, path = np.full((B, len(alphas)), np.nan), np.full((B, len(alphas), k), np.nan)
    for j, a in enumerate(alphas):
        Li, ok = _cholesky_inverse(G + a * np.eye(k))
        b = np.einsum("bki,bkj,bj->bi", Li, Li, c)
        Z = np.einsum("bni,bki->bnk", Xf, Li)
        om = 1.0 - (Z * Z).sum(axis=2)
        e = yf - np.einsum("bni,bi->bn", Xf, b)
        sc = (np.where(m, e / np.where(m, om, 1.0), 0.0) ** 2).sum(axis=1) / np.where(nn > 0, nn, 1.0)
        usable = ok & (nn > 0) & ~(m & ~(om >= HIGH_LEVERAGE)).any(axis=1) & np.isfinite(sc)
        scores[usable, j] = sc[usable]
        path[usable, j] = b[usable]
    return scores, path


def choose(scores):
    """(alpha_index [G], score [G]) of a [G, na] table of scores: the smallest usable one, the lowest index on a tie; -1 / NaN
    where no candidate is usable"""
    G = scores.shape[0]
    idx, best = np.full(G, -1, dtype=np.int32), np.full(G, np.nan)
    for g in range(G):
        u = np.nonzero(~np.isnan(scores[g]))[0]
        if len(u):
            idx[g] = u[np.argmin(scores[g, u])]                # (argmin: the first of equal minima)
            best[g] = scores[g, idx[g]]
    return idx, best


def ridge_cv_batch(y, cols, offsets, alphas, weights=None, add_intercept=False, null_policy="ignore", valid=None):
    """Every group of a group-sorted batch.  Returns cv_scores [G, na], coef_path [G, na, kt], alpha_index, alpha, score, status,
    n (fitted rows) per group, and ``fit`` [N]."""
    offs = np.asarray(offsets, dtype=np.int64)
    G, N = len(offs) - 1, int(offs[-1])
    alphas = np.asarray(alphas, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    X = np.column_stack([np.asarray(c, dtype=np.float64) for c in cols])
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    fit, y, X, w = fit_rows(y, X, w, null_policy, valid)
    if add_intercept:
        X = np.column_stack([X, np.ones(N)])
    kt = X.shape[1]
    sw = np.ones(N) if w is None else np.sqrt(w)
    Xs, ys = X * sw[:, None], y * sw
    Xf, yf = np.where(fit[:, None], Xs, 0.0), np.where(fit, ys, 0.0)
    scores, path = np.full((G, len(alphas)), np.nan), np.full((G, len(alphas), kt), np.nan)
    sizes = np.diff(offs)
    with np.errstate(all="ignore"):
        for n in np.unique(sizes):
            if n == 0:
                continue
            ids = np.nonzero(sizes == n)[0]
            step = max(1, int(2e7 // (n * kt)))
            for lo in range(0, len(ids), step):
                part = ids[lo:lo + step]
                idx = offs[part][:, None] + np.arange(n)[None, :]
                scores[part], path[part] = _stack(Xf[idx], yf[idx], fit[idx], alphas)
    cs = np.concatenate([[0], np.cumsum(fit)])
    nfit = cs[offs[1:]] - cs[offs[:-1]]
    index, best = choose(scores)
    status = np.where(index >= 0, OK, np.where(nfit > 0, FALLBACK, EMPTY)).astype(np.int32)
    alpha = np.where(index >= 0, alphas[np.maximum(index, 0)], np.nan)
    return dict(cv_scores=scores, coef_path=path, alpha_index=index, alpha=alpha, score=best, status=status, n=nfit, fit=fit)


def chosen_outputs(ref, index, y, cols, offsets, weights=None, add_intercept=False, null_policy="ignore"):
    """coef [G, kt], pred [N], resid [N] of the candidate ``index[g]`` of every group (the DEVICE's choice in the tests), as
    pols_least_squares(alpha = that candidate) returns them: features zero-filled for every policy but "ignore", "drop" masks the
    rows outside the fit with NaN, a group without a usable candidate is NaN and an empty one has zero coefficients."""
    offs = np.asarray(offsets, dtype=np.int64)
    G, N = len(offs) - 1, int(offs[-1])
    kt = ref["coef_path"].shape[2]
    index = np.asarray(index)
    coef = np.where((index >= 0)[:, None], ref["coef_path"][np.arange(G), np.maximum(index, 0)], np.nan)
    coef[(index < 0) & (ref["n"] == 0)] = 0.0
    y = np.asarray(y, dtype=np.float64)
    X = np.column_stack([np.asarray(c, dtype=np.float64) for c in cols])
    if null_policy != "ignore":
        X = np.nan_to_num(X, nan=0.0)
    if add_intercept:
        X = np.column_stack([X, np.ones(N)])
    assert X.shape[1] == kt
    with np.errstate(all="ignore"):
        pred = (X * np.repeat(coef, np.diff(offs), axis=0)).sum(axis=1)
    if null_policy == "drop":
        pred = np.where(ref["fit"], pred, np.nan)
    return coef, pred, y - pred


def loo_brute_force(ys, Xs, alpha):
    """the definition itself on ONE group's scaled fitted rows: delete row i, re-solve the ridge, predict row i"""
    n, k = Xs.shape
    err = np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        A = Xs[keep].T @ Xs[keep] + alpha * np.eye(k)
        b = np.linalg.solve(A, Xs[keep].T @ ys[keep])
        err[i] = ys[i] - Xs[i] @ b
    return float((err * err).mean())
