"""numpy restatement of the robust standard errors of mode="statistics" (cov_type HC0 .. HC3, HAC): the yardstick of
tests/test_robust_stats_*.py.  Per group, f64, on the sqrt(w)-scaled rows with the ones column last:
A = X'X + alpha I, b = A^-1 X'y, e = y - X b, h_i = x_i' A^-1 x_i, u_i = c_i e_i x_i, S = sum u_i u_i' (+ Bartlett-weighted lag
cross products for HAC), V = A^-1 S A^-1 (x n / df for HC1), se = sqrt(diag V), t = b / se, p two-sided Student-t with df."""
import math

import numpy as np

COV_TYPES = ("HC0", "HC1", "HC2", "HC3", "HAC")


def _betacf(a, b, x):
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) >= tiny else tiny)
    h = d
    for m in range(1, 501):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = d if abs(d) >= tiny else tiny
        c = 1.0 + aa / c
        c = c if abs(c) >= tiny else tiny
        d = 1.0 / d
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = d if abs(d) >= tiny else tiny
        c = 1.0 + aa / c
        c = c if abs(c) >= tiny else tiny
        d = 1.0 / d
        de = d * c
        h *= de
        if abs(de - 1.0) < 1e-16:
            break
    return h


def betai(a, b, x):
    """regularised incomplete beta I_x(a, b)"""
    if not x > 0.0:
        return x if x != x else 0.0
    if x >= 1.0:
        return 1.0
    bt = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x))
    if x < (a + 1.0) / (a + b + 2.0):
        return bt * _betacf(a, b, x) / a
    return 1.0 - bt * _betacf(b, a, 1.0 - x) / b


def two_sided_p(t, df):
    """2 (1 - cdf_t(|t|; df)) == I_{df / (df + t^2)}(df / 2, 1 / 2)"""
    if t != t:
        return float("nan")
    return betai(0.5 * df, 0.5, df / (df + t * t))


def hac_meat(U, maxlags):
    """sum_i u_i u_i' + sum_{l=1..L} (1 - l / (L + 1)) sum_i (u_i u_{i-l}' + u_{i-l} u_i'), L = min(maxlags, n - 1)"""
    n = U.shape[0]
    S = U.T @ U
    L = min(maxlags, n - 1)
    for lag in range(1, L + 1):
        G = U[lag:].T @ U[:-lag]
        S += (1.0 - lag / (L + 1)) * (G + G.T)
    return S


def hac_meat_bruteforce(U, maxlags):
    """the same sum as a double loop over row pairs |i - j| <= L"""
    n, k = U.shape
    L = min(maxlags, n - 1)
    S = np.zeros((k, k))
    for i in range(n):
        for j in range(max(0, i - L), min(n, i + L + 1)):
            wt = 1.0 - abs(i - j) / (L + 1)
            S += wt * np.outer(U[i], U[j])
    return S


def robust_group(y, X, w=None, alpha=0.0, cov_type="HC0", maxlags=0):
    """One group: y [n], X [n, k] (the ones column, if any, already appended last), w [n] or None.  Returns se, t, p [k]."""
    y = np.asarray(y, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    n, k = X.shape
    nan = np.full(k, np.nan)
    if w is not None:
        sw = np.sqrt(np.asarray(w, dtype=np.float64))
        X, y = X * sw[:, None], y * sw
    A = X.T @ X + alpha * np.eye(k)
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return nan, nan.copy(), nan.copy()
    Li = np.linalg.inv(Lc)
    Ainv = Li.T @ Li
    b = Ainv @ (X.T @ y)
    df = n - np.trace(Ainv) if alpha > 0 else float(n - k)
    if not df > 0:
        return nan, nan.copy(), nan.copy()
    e = y - X @ b
    c = np.ones(n)
    if cov_type in ("HC2", "HC3"):
        h = np.einsum("ij,jk,ik->i", X, Ainv, X)
        om = 1.0 - h
        if not np.all(om >= 1e-10):
            return nan, nan.copy(), nan.copy()
        c = om ** -0.5 if cov_type == "HC2" else 1.0 / om
    U = (c * e)[:, None] * X
    S = hac_meat(U, maxlags) if cov_type == "HAC" else U.T @ U
    V = Ainv @ S @ Ainv
    if cov_type == "HC1":
        V = V * (n / df)
    se = np.sqrt(np.diag(V))
    t = b / se
    p = np.array([two_sided_p(float(tj), df) for tj in t])
    return se, t, p


def robust_batch(y, cols, offsets, weights=None, add_intercept=False, alpha=0.0, cov_type="HC0", maxlags=0):
    """Every group of a group-sorted batch: dict std_err / t_values / p_values [G, k]."""
    offs = np.asarray(offsets)
    out = {"std_err": [], "t_values": [], "p_values": []}
    for g in range(len(offs) - 1):
        s, e = int(offs[g]), int(offs[g + 1])
        X = np.column_stack([np.asarray(c[s:e], dtype=np.float64) for c in cols]) if cols else np.zeros((e - s, 0))
        if add_intercept:
            X = np.column_stack([X, np.ones(e - s)])
        se, t, p = robust_group(y[s:e], X, None if weights is None else weights[s:e], alpha, cov_type, maxlags)
        out["std_err"].append(se)
        out["t_values"].append(t)
        out["p_values"].append(p)
    return {k: np.array(v) for k, v in out.items()}
