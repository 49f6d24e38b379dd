"""numpy restatement of the elastic-net / lasso regularisation path with K-fold selection of alpha (pols_elastic_net_cv, K12): the
yardstick of tests/test_enet_cv_*.py; the definitions are the header's.  Per group, f64, on the fitted rows F scaled by sqrt(w) with
the ones column last: the fitted rows are cut in row order into n_folds contiguous folds (KFold(shuffle=False)), every fold's Gram
matrix is a direct sum over its rows, the training matrix of fold f is the sum of the others.  Every fit is the reference's cyclic
coordinate descent in Gram form with alpha times the rows OF THAT FIT, candidates visited in descending order (equal values in index
order) with warm starts; the validation error of fold f is max(0, yy_f - 2 b'c_f + b'G_f b) / n_f, the score the mean over the
folds, the winner the smallest finite score with the lowest index.  All problems of a batch are swept together."""
import numpy as np

from ridge_cv_ref import chosen_outputs, fit_rows  # noqa: F401  (chosen_outputs: coef / pred / resid at the device's choice)

OK, FALLBACK, EMPTY, NOT_CONVERGED = 0, 1, 2, 3


def fold_ids(n, n_folds):
    """fold of every rank 0 .. n - 1: the first n % n_folds folds hold n // n_folds + 1 rows, the rest n // n_folds"""
    sizes = np.full(n_folds, n // n_folds, dtype=np.int64)
    sizes[:n % n_folds] += 1
    return np.repeat(np.arange(n_folds), sizes)


def auto_grid(c_full, n, l1_ratio, n_alphas, eps):
    """(alpha_max, grid): alpha_max = max|X'y| / (n l1_ratio), a_j = alpha_max eps^(j / (n_alphas - 1))"""
    with np.errstate(all="ignore"):
        amax = np.abs(c_full).max() / (n * l1_ratio)
        return amax, amax * eps ** (np.arange(n_alphas) / (n_alphas - 1))


def cd_path(Gm, c, m, alphas, order, go, l1_ratio, max_iter, tol, positive):
    """P problems at once.  Gm [P, k, k], c [P, k], m [P] rows of each fit, alphas [P, A], order: the candidates' visiting order,
    go [P]: the problems that are fitted at all.  Returns path [P, A, k] (NaN where not go), sweeps [P, A], stopped [P, A]."""
    P, k = c.shape
    A = alphas.shape[1]
    w = np.zeros((P, k))
    path = np.full((P, A, k), np.nan)
    sweeps, stopped = np.zeros((P, A), dtype=np.int32), np.zeros((P, A), dtype=bool)
    diag = np.einsum("pii->pi", Gm)
    with np.errstate(all="ignore"):
        for j in order:
            an = alphas[:, j] * m
            thr, den = an * l1_ratio, diag + (an * (1.0 - l1_ratio))[:, None]
            idx = np.nonzero(go)[0]
            for it in range(max_iter):
                if idx.size == 0:
                    break
                Gs, ws = Gm[idx], w[idx]
                w_old = ws.copy()
                for q in range(k):
                    ws[:, q] = 0.0
                    dot = c[idx, q] - np.einsum("pi,pi->p", Gs[:, q, :], ws)
                    s = np.copysign(np.maximum(np.abs(dot) - thr[idx], 0.0), dot)
                    if positive:
                        s = np.maximum(s, 0.0)
                    ws[:, q] = s / den[idx, q]
                w[idx] = ws
                sweeps[idx, j] = it + 1
                conv = np.sqrt(((ws - w_old) ** 2).sum(axis=1)) < tol
                if it + 1 == max_iter:
                    stopped[idx[~conv], j] = True
                idx = idx[~conv]
            path[go, j] = w[go]
    return path, sweeps, stopped


def choose(scores):
    """(alpha_index [G], score [G]): the smallest finite score, the lowest index on a tie; -1 / NaN where there is none"""
    G = scores.shape[0]
    idx, best = np.full(G, -1, dtype=np.int32), np.full(G, np.nan)
    for g in range(G):
        u = np.nonzero(np.isfinite(scores[g]))[0]
        if len(u):
            idx[g] = u[np.argmin(scores[g, u])]
            best[g] = scores[g, idx[g]]
    return idx, best


def enet_cv_batch(y, cols, offsets, alphas=None, *, n_alphas=100, eps=1e-3, l1_ratio=0.5, n_folds=5, max_iter=1000, tol=1e-5,
                  positive=False, weights=None, add_intercept=False, null_policy="ignore", valid=None):
    """Every group of a group-sorted batch.  Returns cv_scores, alphas_used, n_iter [G, A], coef_path [G, A, kt], alpha_index, alpha,
    score, status, n (fitted rows) per group, ``fit`` [N] and fold_scores [G, n_folds, A]."""
    offs = np.asarray(offsets, dtype=np.int64)
    G, N = len(offs) - 1, int(offs[-1])
    F = n_folds
    y = np.asarray(y, dtype=np.float64)
    X = np.column_stack([np.asarray(c, dtype=np.float64) for c in cols])
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    fit, y, X, w = fit_rows(y, X, w, null_policy, valid)
    if add_intercept:
        X = np.column_stack([X, np.ones(N)])
    kt = X.shape[1]
    sw = np.ones(N) if w is None else np.sqrt(w)
    Xs, ys = X * sw[:, None], y * sw
    automatic = alphas is None
    A = n_alphas if automatic else len(alphas)
    order = np.arange(A) if automatic else np.argsort(-np.asarray(alphas, dtype=np.float64), kind="stable")
    # per-fold Gram matrices by direct row sums
    Gf, cf, yyf, nf = np.zeros((G, F, kt, kt)), np.zeros((G, F, kt)), np.zeros((G, F)), np.zeros((G, F))
    nfit = np.zeros(G, dtype=np.int64)
    with np.errstate(all="ignore"):
        for g in range(G):
            rows = np.arange(offs[g], offs[g + 1])[fit[offs[g]:offs[g + 1]]]
            nfit[g] = len(rows)
            if len(rows) < F:
                continue
            fid = fold_ids(len(rows), F)
            for f in range(F):
                r = rows[fid == f]
                Gf[g, f], cf[g, f], yyf[g, f], nf[g, f] = Xs[r].T @ Xs[r], Xs[r].T @ ys[r], ys[r] @ ys[r], len(r)
        Gall, call = Gf.sum(axis=1), cf.sum(axis=1)
        grid = np.empty((G, A))
        go = nfit >= F
        if automatic:
            for g in range(G):
                amax, grid[g] = auto_grid(call[g], float(nfit[g]), l1_ratio, A, eps) if go[g] else (np.nan, np.nan)
                if not (amax > 0 and np.isfinite(amax)):
                    go[g], grid[g] = False, np.nan
        else:
            grid[:] = np.asarray(alphas, dtype=np.float64)[None, :]
        # the problems: (g, f) trains on the other folds, (g, F) on everything
        # (the training matrix is the sum of the OTHER folds, not a difference: no cancellation)
        others = [[h for h in range(F) if h != f] for f in range(F)]
        Gm = np.stack([Gf[:, o].sum(axis=1) for o in others] + [Gall], axis=1).reshape(G * (F + 1), kt, kt)
        cm = np.stack([cf[:, o].sum(axis=1) for o in others] + [call], axis=1).reshape(G * (F + 1), kt)
        m = np.concatenate([nfit[:, None] - nf, nfit[:, None].astype(np.float64)], axis=1).reshape(-1)
        path, sweeps, stopped = cd_path(Gm, cm, m, np.repeat(grid, F + 1, axis=0), order, np.repeat(go, F + 1), l1_ratio, max_iter, tol, positive)
        path = path.reshape(G, F + 1, A, kt)
        sweeps, stopped = sweeps.reshape(G, F + 1, A), stopped.reshape(G, F + 1, A)
        b = path[:, :F]                                            # [G, F, A, kt]
        val = yyf[:, :, None] - 2.0 * np.einsum("gfak,gfk->gfa", b, cf) + np.einsum("gfak,gfkl,gfal->gfa", b, Gf, b)
        fold_scores = np.maximum(val, 0.0) / np.where(nf > 0, nf, 1.0)[:, :, None]
        scores = fold_scores.sum(axis=1) / F
    scores[~go] = np.nan
    index, best = choose(scores)
    has = index >= 0
    rows = np.arange(G)
    status = np.where(has, np.where(stopped[rows, :, np.maximum(index, 0)].any(axis=1), NOT_CONVERGED, OK),
                      np.where(nfit > 0, FALLBACK, EMPTY)).astype(np.int32)
    alpha = np.where(has, grid[rows, np.maximum(index, 0)], np.nan)
    return dict(cv_scores=scores, alphas_used=grid, coef_path=path[:, F], alpha_index=index, alpha=alpha, score=best, status=status,
                n_iter=sweeps.max(axis=1).astype(np.int32), n=nfit, fit=fit, fold_scores=fold_scores)
