"""numpy restatements of the random-effects panel regression (pols_random_effects, K19): the yardstick of tests/test_random_effects_*.py.
Two independent routes on f64 values:

``re_group``         the header's definitions: the within fit (absorb_ref's Cholesky with the pivot rule against the raw second moments),
                     the between regression over the table of category means (pivots against the table's second moments), Swamy-Arora
                     variance components, M = embed(A_w) + sum_c q_c zbar_c zbar_c' and v likewise, b = M^-1 v (pivots against the raw
                     second moments, n for the intercept), RSS = the row term + the table term, V = RSS / (n - kc) M^-1, the Hausman
                     statistic from D = sigma2_e (A_w^-1 - (M^-1)_1..k,1..k), u_c and theta_c.
``gls_dense_group``  the dense solve with Omega = sigma2_e I + sigma2_u [same id]: b = (Z'Omega^-1 Z)^-1 Z'Omega^-1 y and the matrix
                     (Z'Omega^-1 Z)^-1 / sigma2_e, which equals M^-1; sigma2_e and sigma2_u are taken from ``re_group``."""
import numpy as np
from scipy import special

from absorb_ref import BAD_DOF, EMPTY, FALLBACK, OK, _by_category, _chol, _chol_inverse
from robust_ref import two_sided_p

GROUP_FIELDS = ("se", "t_values", "p_values", "coef_between", "coef_within", "sigma2_e", "sigma2_u", "rho", "hausman", "hausman_p")
ROW_FIELDS = ("pred", "resid", "effects", "theta")
COUNTS = ("n_obs", "n_categories", "status")


def _solve(M, v, T, kc):
    """(b, M^-1) by Cholesky with pivots held against T, or None when a pivot fails or M is not finite"""
    if not (np.isfinite(M).all() and np.isfinite(v).all()):
        return None
    L = _chol(M, T, kc)
    if L is None:
        return None
    Mi = _chol_inverse(L)
    b = Mi @ v
    return (b, Mi) if np.isfinite(b).all() else None


def re_group(y, X, ids, add_intercept=False, fit=None):
    """One group.  y [N], X [N, k] (user columns only), ids [N]; ``fit``: the rows of the fit (None: all).  Returns a dict: coef / se /
    t_values / p_values / coef_between [kc], coef_within [k], sigma2_e, sigma2_u, rho, hausman, hausman_p, n_obs, n_categories, status,
    pred / resid / effects / theta [N], and Minv [kc, kc] for the dense route."""
    y, X = np.asarray(y, dtype=np.float64), np.asarray(X, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64)
    N, k = X.shape
    kc = k + (1 if add_intercept else 0)
    fit = np.ones(N, dtype=bool) if fit is None else np.asarray(fit, dtype=bool)
    nanc = np.full(kc, np.nan)
    out = {"coef": nanc.copy(), "se": nanc.copy(), "t_values": nanc.copy(), "p_values": nanc.copy(), "coef_between": nanc.copy(),
           "coef_within": np.full(k, np.nan), "sigma2_e": np.nan, "sigma2_u": np.nan, "rho": np.nan, "hausman": np.nan, "hausman_p": np.nan,
           "pred": np.full(N, np.nan), "resid": np.full(N, np.nan), "effects": np.full(N, np.nan), "theta": np.full(N, np.nan), "Minv": None}
    yf, Xf, idf = y[fit], X[fit], ids[fit]
    n = int(fit.sum())
    uniq, inv = np.unique(idf, return_inverse=True)
    C = len(uniq)
    out["n_obs"], out["n_categories"] = n, C
    if n == 0:
        out["coef"] = np.zeros(kc)
        out["status"] = EMPTY
        return out
    df_w, df_b = n - k - C, C - kc
    if df_w <= 0 or df_b <= 0:
        out["status"] = BAD_DOF
        return out
    out["status"] = FALLBACK
    # 1. within
    Tc = _by_category(inv, C, np.ones(n))
    ybar = _by_category(inv, C, yf) / Tc
    xbar = _by_category(inv, C, Xf) / Tc[:, None]
    Xt, yt = Xf - xbar[inv], yf - ybar[inv]
    A_w, g_w, T_raw = Xt.T @ Xt, Xt.T @ yt, (Xf * Xf).sum(axis=0)
    within = _solve(A_w, g_w, T_raw, k)
    if within is None:
        return out
    b_w, A_wi = within
    s2e = ((yt - Xt @ b_w) ** 2).sum() / df_w
    # 2. between
    Z = np.column_stack([xbar, np.ones(C)]) if add_intercept else xbar
    B = Z.T @ Z
    between = _solve(B, Z.T @ ybar, np.diag(B).copy(), kc)
    if between is None:
        return out
    b_b = between[0]
    rss_b = ((ybar - Z @ b_b) ** 2).sum()
    # 3. variance components
    tbar = C / (1.0 / Tc).sum()
    raw = rss_b / df_b - s2e / tbar
    if not np.isfinite(raw):
        return out
    s2u = max(0.0, raw)
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = 1.0 - np.sqrt(s2e / (s2e + Tc * s2u))
    # 4. GLS
    qc = Tc * (1.0 - theta) ** 2
    M, v = (Z * qc[:, None]).T @ Z, (Z * qc[:, None]).T @ ybar
    M[:k, :k] += A_w
    v[:k] += g_w
    gls = _solve(M, v, np.concatenate([T_raw, [float(n)]])[:kc], kc)
    if gls is None:
        return out
    b, Mi = gls
    # 5. / 6. residual sum, inference
    r_c = ybar - Z @ b
    rss_t = (qc * r_c ** 2).sum()
    if not np.isfinite(rss_t):
        return out
    rss = ((yt - Xt @ b[:k]) ** 2).sum() + rss_t
    df = n - kc
    V = rss / df * np.diag(Mi)
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.where(V >= 0, np.sqrt(np.abs(V)), np.nan)
        t = b / se
    p = np.array([two_sided_p(float(tj), float(df)) if np.isfinite(tj) else np.nan for tj in t])
    # 7. Hausman
    D = s2e * (A_wi - Mi[:k, :k])
    L = _chol(D, np.zeros(k), k) if np.isfinite(D).all() else None
    if L is not None:
        z = np.linalg.solve(L, b_w - b[:k])
        out["hausman"] = float(z @ z)
        out["hausman_p"] = float(special.gammaincc(0.5 * k, 0.5 * out["hausman"]))
    # 8. / 9. effects, rows
    u_c = Tc * s2u / (Tc * s2u + s2e) * r_c
    Zrow = np.column_stack([X, np.ones(N)]) if add_intercept else X
    pos = {int(i): j for j, i in enumerate(uniq.tolist())}
    row_c = np.array([pos.get(int(i), -1) for i in ids], dtype=np.int64)
    has = row_c >= 0
    out["pred"] = Zrow @ b
    out["resid"] = y - out["pred"]
    out["effects"][has], out["theta"][has] = u_c[row_c[has]], theta[row_c[has]]
    out.update(coef=b, se=se, t_values=t, p_values=p, coef_between=b_b, coef_within=b_w, sigma2_e=float(s2e), sigma2_u=float(s2u),
               rho=float(s2u / (s2u + s2e)), status=OK, Minv=Mi)
    return out


def gls_dense_group(y, X, ids, sigma2_e, sigma2_u, add_intercept=False):
    """One group by the dense solve: (b [kc], (Z'Omega^-1 Z)^-1 / sigma2_e [kc, kc])."""
    y, X = np.asarray(y, dtype=np.float64), np.asarray(X, dtype=np.float64)
    ids = np.asarray(ids)
    n = len(y)
    Z = np.column_stack([X, np.ones(n)]) if add_intercept else X
    Om = sigma2_e * np.eye(n) + sigma2_u * (ids[:, None] == ids[None, :])
    OiZ = np.linalg.solve(Om, Z)
    P = Z.T @ OiZ
    b = np.linalg.solve(P, OiZ.T @ y)
    return b, np.linalg.inv(P) / sigma2_e


DROP_FAMILY = ("drop", "drop_zero", "drop_y_zero_x", "drop_window")


def fitted_rows(y, cols, policy, valid=None):
    """the rows a null policy fits (NaN = null; ``valid``: the mask of the drop family), and y and the features as the fit and the
    prediction see them: as they are under "ignore", zero-filled under every other policy"""
    y = np.asarray(y, dtype=np.float64)
    cols = [np.asarray(c, dtype=np.float64) for c in cols]
    keep = np.ones(len(y), dtype=bool)
    if policy == "ignore":
        return keep, y, cols
    if policy in DROP_FAMILY:
        keep = ~np.isnan(y)
        if valid is not None:
            keep &= np.asarray(valid).astype(bool)
        if policy != "drop_y_zero_x":
            for c in cols:
                keep &= ~np.isnan(c)
    elif policy != "zero":
        raise ValueError(policy)
    return keep, np.where(np.isnan(y), 0.0, y), [np.where(np.isnan(c), 0.0, c) for c in cols]


def re_batch(y, cols, offsets, ids, add_intercept=False, policy="ignore", valid=None):
    """Every group of a group-sorted batch: dict coef / GROUP_FIELDS [G, ..], COUNTS [G], ROW_FIELDS [N].  pred = z'b on the filled
    features for every row, under "drop" NaN for a row outside the fit; resid = y - pred on the raw y; effects and theta follow the
    row's id."""
    offs = np.asarray(offsets)
    y = np.asarray(y, dtype=np.float64)
    keep, yf, cols = fitted_rows(y, cols, policy, valid)
    res = {key: [] for key in ("coef",) + GROUP_FIELDS + COUNTS}
    rows = {key: np.full(len(y), np.nan) for key in ROW_FIELDS}
    for g in range(len(offs) - 1):
        s, e = int(offs[g]), int(offs[g + 1])
        X = np.column_stack([c[s:e] for c in cols]) if e > s else np.zeros((0, len(cols)))
        r = re_group(yf[s:e], X, ids[s:e], add_intercept, fit=keep[s:e])
        for key in res:
            res[key].append(r[key])
        for key in ("pred", "effects", "theta"):
            rows[key][s:e] = r[key]
        if policy == "drop":
            rows["pred"][s:e][~keep[s:e]] = np.nan
        rows["resid"][s:e] = y[s:e] - rows["pred"][s:e]
    out = {key: np.array(v) for key, v in res.items()}
    out.update(rows)
    return out
