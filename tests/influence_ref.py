"""numpy restatement of the per-row influence diagnostics and prediction intervals (pols_least_squares_influence, K7i): the
yardstick of tests/test_influence_*.py.  Per group, f64, on the fitted rows F scaled by sqrt(w) with the ones column last:
A = X'X + alpha I over F, b = A^-1 X'y, df = n - p (n - trace A^-1 when alpha > 0), sigma2 = sum_F e^2 / df, h_i = x_i' A^-1 x_i,
r_i = e_i / sqrt(sigma2 (1 - h_i)), t_i = r_i sqrt((df - 1) / (df - r_i^2)), Cook's D = r_i^2 h_i / (p (1 - h_i)),
DFFITS = t_i sqrt(h_i / (1 - h_i)), se_mean = sqrt(sigma2 h_i / w_i), se_obs = sqrt(sigma2 (1 + h_i) / w_i), intervals
x_i'b -+ t_crit se.  Rows outside F are new observations: leverage / se / intervals from their features and weight, NaN influence.
Groups of equal length are evaluated as one stack, so half a million small groups take seconds."""
import numpy as np

from robust_ref import betai

ROW_FIELDS = ("leverage", "student_internal", "student_external", "cooks_d", "dffits", "se_mean", "se_obs",
              "mean_lo", "mean_hi", "obs_lo", "obs_hi")
INFLUENCE_FIELDS = ROW_FIELDS[1:5]
GROUP_FIELDS = ("sigma2", "df", "t_crit")
HIGH_LEVERAGE = 1e-10


def t_tail(t, df):
    """P(|T| > t) for Student-t with df degrees of freedom"""
    return betai(0.5 * df, 0.5, df / (df + t * t))


def t_crit(df, level):
    """the (1 - (1 - level) / 2) quantile of Student-t(df): bracket, then bisect the two-sided tail (df may be fractional)"""
    if not df > 0:
        return float("nan")
    a = 1.0 - level
    lo, hi = 0.0, 1.0
    while t_tail(hi, df) > a:
        lo, hi = hi, hi * 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            break
        if t_tail(mid, df) > a:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _stack(y, X, w, alpha, fit):
    """B groups of n rows: y [B, n], X [B, n, k], w [B, n] or None, fit [B, n] bool or None (None: every row is fitted)."""
    B, n, k = X.shape
    m = np.ones((B, n), dtype=bool) if fit is None else fit
    wv = np.ones((B, n)) if w is None else np.where(m & np.isnan(w), 1e-24, w)       # a fitted row's null weight acts as 1e-24
    sw = np.sqrt(wv)
    Xs, ys = X * sw[..., None], y * sw
    Xf, yf = np.where(m[..., None], Xs, 0.0), np.where(m, ys, 0.0)
    nn = m.sum(axis=1).astype(np.float64)
    A = np.einsum("bni,bnj->bij", Xf, Xf) + alpha * np.eye(k)
    c = np.einsum("bni,bn->bi", Xf, yf)
    Ainv = np.full((B, k, k), np.nan)
    ok = np.zeros(B, dtype=bool)
    try:                                                       # the whole stack at once; group by group when one of them fails
        if not np.isfinite(A).all():
            raise np.linalg.LinAlgError
        Li = np.linalg.inv(np.linalg.cholesky(A))
        Ainv, ok[:] = np.einsum("bki,bkj->bij", Li, Li), True
    except np.linalg.LinAlgError:
        for i in range(B):
            try:
                if np.isfinite(A[i]).all():
                    Li = np.linalg.inv(np.linalg.cholesky(A[i]))
                    Ainv[i], ok[i] = Li.T @ Li, True
            except np.linalg.LinAlgError:
                pass
    b = np.einsum("bij,bj->bi", Ainv, c)
    df = nn - np.trace(Ainv, axis1=1, axis2=2) if alpha > 0 else nn - float(k)
    good = ok & (df > 0)
    e = ys - np.einsum("bnk,bk->bn", Xs, b)
    sigma2 = np.where(good, (np.where(m, e, 0.0) ** 2).sum(axis=1) / np.where(good, df, 1.0), np.nan)
    h = np.einsum("bni,bij,bnj->bn", Xs, Ainv, Xs)
    pm = np.einsum("bnk,bk->bn", X, b)
    om = 1.0 - h
    s2, dfc = sigma2[:, None], df[:, None]
    r = e / np.sqrt(s2 * om)
    den = dfc - r * r
    t = np.where((dfc - 1.0 > 0) & (den > 0), r * np.sqrt((dfc - 1.0) / np.where(den > 0, den, 1.0)), np.nan)
    cd = r * r * h / (k * om)
    dff = t * np.sqrt(h / om)
    undefined = ~m | ~(om >= HIGH_LEVERAGE)
    se_mean, se_obs = np.sqrt(s2 * h / wv), np.sqrt(s2 * (1.0 + h) / wv)
    out = {"leverage": h, "student_internal": r, "student_external": t, "cooks_d": cd, "dffits": dff, "se_mean": se_mean, "se_obs": se_obs,
           "pred": pm}
    for f in INFLUENCE_FIELDS:
        out[f] = np.where(undefined, np.nan, out[f])
    for f in out:
        out[f] = np.where(good[:, None], out[f], np.nan)
    return out, sigma2, df, good


def influence_batch(y, cols, offsets, weights=None, add_intercept=False, alpha=0.0, level=0.95, fit=None):
    """Every group of a group-sorted batch.  ``fit`` [n_rows] bool marks the rows a null policy keeps (None: all of them); the inputs are
    what the policy leaves (its zero fills applied by the caller).  Returns the per-row arrays [n_rows], sigma2 / df / t_crit [G] and
    "pred" (x_i'b, un-scaled)."""
    offs = np.asarray(offsets, dtype=np.int64)
    G, N = len(offs) - 1, int(offs[-1])
    y = np.asarray(y, dtype=np.float64)
    X = np.column_stack([np.asarray(c, dtype=np.float64) for c in cols] + ([np.ones(N)] if add_intercept else []))
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    rows = {f: np.full(N, np.nan) for f in ROW_FIELDS + ("pred",)}
    sigma2, df = np.full(G, np.nan), np.full(G, np.nan)
    sizes = np.diff(offs)
    with np.errstate(all="ignore"):
        for n in np.unique(sizes):
            ids = np.nonzero(sizes == n)[0]
            if n == 0:
                df[ids] = -float(X.shape[1])
                continue
            idx = offs[ids][:, None] + np.arange(n)[None, :]
            out, s2, d, _ = _stack(y[idx], X[idx], None if w is None else w[idx], alpha, None if fit is None else np.asarray(fit, dtype=bool)[idx])
            for f, v in out.items():
                rows[f][idx] = v
            sigma2[ids], df[ids] = s2, d
        tc = np.full(G, np.nan)
        cache = {}
        for g in range(G):
            if sigma2[g] == sigma2[g]:
                key = float(df[g])
                if key not in cache:
                    cache[key] = t_crit(key, level)
                tc[g] = cache[key]
        tcr = np.repeat(tc, sizes)
        rows["mean_lo"], rows["mean_hi"] = rows["pred"] - tcr * rows["se_mean"], rows["pred"] + tcr * rows["se_mean"]
        rows["obs_lo"], rows["obs_hi"] = rows["pred"] - tcr * rows["se_obs"], rows["pred"] + tcr * rows["se_obs"]
    rows.update(sigma2=sigma2, df=df, t_crit=tc)
    return rows


def conditioning(ref, offsets, rows=None):
    """(min over rows of 1 - h_i, max over rows of r_i^2 / df): what the comparison frames keep away from 0 and 1; ``rows`` [n_rows]
    bool restricts it to the rows whose influence measures are compared (the fitted rows of healthy groups)"""
    sizes = np.diff(np.asarray(offsets))
    df = np.repeat(ref["df"], sizes)
    h, r = ref["leverage"], ref["student_internal"]
    if rows is not None:
        df, h, r = df[rows], h[rows], r[rows]
    return float(np.nanmin(1.0 - h)), float(np.nanmax(r * r / df))
