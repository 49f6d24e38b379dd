"""numpy restatements of the absorbed-effect regression (pols_least_squares_absorb, K16): the yardstick of tests/test_absorb_*.py.
Two independent routes on f64 (or any numpy float type) values:

``within_group``   the header's definitions: category means first, the demeaned rows x~ = sqrt(w) (x - xbar_c), A = X~'X~ factored by
                   Cholesky with the pivot rule d_j <= 16 k eps T_jj (T_jj = sum w x_j^2), b, e~ from the rows, a_c = ybar_c - xbar_c'b,
                   c0 = sum W_c a_c / sum W_c, df = n - k - C, V = sigma2 A^-1 or q A^-1 (sum_c s_c s_c') A^-1 with
                   q = C / (C - 1) (n - 1) / (n - k - 1).
``lsdv_group``     explicit dummies through np.linalg.lstsq; cluster standard errors from cluster_ref.cluster_group on the dummy design
                   without its correction, times q (each dummy's score sums to zero inside its own cluster, so the Frisch-Waugh-Lovell
                   identity holds for the sandwich too)."""
import numpy as np

from cluster_ref import cluster_group
from robust_ref import two_sided_p

OK, FALLBACK, EMPTY, BAD_DOF = 0, 1, 2, 4


def _chol(A, T, k):
    """lower factor of A by the pivot rule of the header (None when a pivot fails), in A's dtype"""
    ft = A.dtype.type
    eps = ft(np.finfo(np.float64).eps)
    L = np.zeros_like(A)
    for j in range(k):
        d = A[j, j] - (L[j, :j] ** 2).sum()
        if not d > ft(16 * k) * eps * T[j]:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, k):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def _chol_inverse(L):
    k = L.shape[0]
    Li = np.zeros_like(L)
    for c in range(k):                                         # column c of L^-1 by forward substitution
        for j in range(c, k):
            s = (L.dtype.type(1) if j == c else L.dtype.type(0)) - (L[j, c:j] * Li[c:j, c]).sum()
            Li[j, c] = s / L[j, j]
    return Li.T @ Li


def _by_category(inv, C, v):
    """sums of the rows of v (one or two dimensions) per category"""
    out = np.zeros((C,) + v.shape[1:], dtype=v.dtype)
    np.add.at(out, inv, v)
    return out


def within_group(y, X, ids, w=None, add_intercept=False, cov_type="nonrobust", fit=None, ft=np.float64):
    """One group.  y [n], X [n, k] (user columns only), ids [n], w [n] or None; ``fit``: the rows of the fit (None: all), the others
    are predicted from their category's effect (NaN when it has no fitted row).  Returns a dict: coef [k (+ 1)], se / t_values /
    p_values (same length, NaN for the intercept), sigma2, r2_within, r2, n_obs, n_categories, status, pred / resid / fe [n]."""
    y, X = np.asarray(y, dtype=ft), np.asarray(X, dtype=ft)
    ids = np.asarray(ids, dtype=np.int64)
    N, k = X.shape
    kc = k + (1 if add_intercept else 0)
    fit = np.ones(N, dtype=bool) if fit is None else np.asarray(fit, dtype=bool)
    wv = np.ones(N, dtype=ft) if w is None else np.asarray(w, dtype=ft)
    nanv = np.full(kc, np.nan)
    out = {"coef": nanv.copy(), "se": nanv.copy(), "t_values": nanv.copy(), "p_values": nanv.copy(), "sigma2": np.nan,
           "r2_within": np.nan, "r2": np.nan, "pred": np.full(N, np.nan), "resid": np.full(N, np.nan), "fe": np.full(N, np.nan)}
    yf, Xf, idf, wf = y[fit], X[fit], ids[fit], wv[fit]
    n = int(fit.sum())
    uniq, inv = np.unique(idf, return_inverse=True)
    C = len(uniq)
    out["n_obs"], out["n_categories"] = n, C
    if n == 0:
        out["coef"] = np.zeros(kc)
        out["status"] = EMPTY
        return out
    df = n - k - C
    if df <= 0:
        out["status"] = BAD_DOF
        return out
    Wc = _by_category(inv, C, wf)                              # the means first
    ybar = _by_category(inv, C, wf * yf) / Wc
    xbar = _by_category(inv, C, wf[:, None] * Xf) / Wc[:, None]
    sw = np.sqrt(wf)
    Xt, yt = sw[:, None] * (Xf - xbar[inv]), sw * (yf - ybar[inv])
    A, T = Xt.T @ Xt, (wf[:, None] * Xf * Xf).sum(axis=0)
    L = _chol(A, T, k) if np.isfinite(np.asarray(A, dtype=np.float64)).all() else None
    if L is None:
        out["status"] = FALLBACK
        return out
    Ainv = _chol_inverse(L)
    b = Ainv @ (Xt.T @ yt)
    et = yt - Xt @ b
    rss = (et ** 2).sum()
    a = ybar - xbar @ b
    c0 = (Wc * a).sum() / Wc.sum() if add_intercept else ft(0)
    sigma2 = rss / df
    if cov_type == "nonrobust":
        V, dfp = sigma2 * np.diag(Ainv), float(df)
    else:
        Z = _by_category(inv, C, et[:, None] * Xt) @ Ainv         # row c: (A^-1 s_c)'
        dfp = C - 1.0
        V = (C / (C - 1.0) * (n - 1.0) / (n - k - 1.0) * (Z ** 2).sum(axis=0)) if (C >= 2 and n - k - 1 > 0) else np.full(k, np.nan)
    V = np.asarray(V, dtype=np.float64)
    b64 = np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.where(V >= 0, np.sqrt(np.abs(V)), np.nan)
        t = b64 / se
    p = np.array([two_sided_p(float(tj), dfp) if np.isfinite(tj) else np.nan for tj in t])
    out["coef"][:k], out["se"][:k], out["t_values"][:k], out["p_values"][:k] = b, se, t, p
    if add_intercept:
        out["coef"][k] = c0
    ybw = (wf * yf).sum() / wf.sum()
    out["sigma2"], out["r2_within"], out["r2"] = float(sigma2), float(1 - rss / (yt ** 2).sum()), float(1 - rss / (wf * (yf - ybw) ** 2).sum())
    eff = dict(zip(uniq.tolist(), np.asarray(a, dtype=np.float64)))
    arow = np.array([eff.get(int(i), np.nan) for i in ids])
    out["pred"] = np.asarray(X, dtype=np.float64) @ b64 + arow
    out["resid"] = np.asarray(y, dtype=np.float64) - out["pred"]
    out["fe"] = arow - float(c0)
    out["status"] = OK
    return out


def lsdv_group(y, X, ids, w=None, cov_type="nonrobust"):
    """One group through explicit dummies: coef [k] by lstsq on [X | D], se [k]."""
    y, X = np.asarray(y, dtype=np.float64), np.asarray(X, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64)
    n, k = X.shape
    uniq, inv = np.unique(ids, return_inverse=True)
    C = len(uniq)
    D = (inv[:, None] == np.arange(C)[None, :]).astype(np.float64)
    Z = np.column_stack([X, D])
    sw = np.ones(n) if w is None else np.sqrt(np.asarray(w, dtype=np.float64))
    Zs, ys = Z * sw[:, None], y * sw
    beta = np.linalg.lstsq(Zs, ys, rcond=None)[0]
    if cov_type == "nonrobust":
        e = ys - Zs @ beta
        se = np.sqrt((e ** 2).sum() / (n - k - C) * np.diag(np.linalg.inv(Zs.T @ Zs)))[:k]
    else:
        q = C / (C - 1.0) * (n - 1.0) / (n - k - 1.0)
        se = cluster_group(y, Z, ids, None, w, 0.0, use_correction=False)[0][:k] * np.sqrt(q)
    return beta[:k], se


def fitted_rows(y, cols, policy):
    """the rows a null policy fits (NaN = null) and the features as the fit and the prediction see them"""
    y = np.asarray(y, dtype=np.float64)
    cols = [np.asarray(c, dtype=np.float64) for c in cols]
    if policy == "ignore":
        return np.ones(len(y), dtype=bool), cols
    keep = ~np.isnan(y)
    if policy == "drop":
        for c in cols:
            keep &= ~np.isnan(c)
        return keep, cols
    if policy == "drop_y_zero_x":
        return keep, [np.where(np.isnan(c), 0.0, c) for c in cols]
    raise ValueError(policy)


GROUP_FIELDS = ("se", "t_values", "p_values", "sigma2", "r2_within", "r2")


def within_batch(y, cols, offsets, ids, weights=None, add_intercept=False, cov_type="nonrobust", policy="ignore"):
    """Every group of a group-sorted batch: dict coef / se / t_values / p_values [G, kc], sigma2 / r2_within / r2 / n_obs /
    n_categories / status [G], pred / resid / fe [N].  Under "drop" a row with a null is masked (NaN)."""
    offs = np.asarray(offsets)
    y = np.asarray(y, dtype=np.float64)
    keep, cols = fitted_rows(y, cols, policy)
    res = {key: [] for key in ("coef",) + GROUP_FIELDS + ("n_obs", "n_categories", "status")}
    rows = {key: np.full(len(y), np.nan) for key in ("pred", "resid", "fe")}
    for g in range(len(offs) - 1):
        s, e = int(offs[g]), int(offs[g + 1])
        X = np.column_stack([c[s:e] for c in cols]) if e > s else np.zeros((0, len(cols)))
        Xp = np.where(np.isnan(X), 0.0, X) if policy == "drop" else X
        r = within_group(np.where(keep[s:e], y[s:e], 0.0), Xp, ids[s:e], None if weights is None else np.asarray(weights, dtype=np.float64)[s:e],
                         add_intercept, cov_type, fit=keep[s:e])
        for key in res:
            res[key].append(r[key])
        rows["pred"][s:e], rows["fe"][s:e] = r["pred"], r["fe"]
        rows["resid"][s:e] = y[s:e] - r["pred"]
        if policy == "drop":
            for key in rows:
                rows[key][s:e][~keep[s:e]] = np.nan
    out = {key: np.array(v) for key, v in res.items()}
    out.update(rows)
    return out
