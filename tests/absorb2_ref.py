"""numpy restatements of the two-way absorbed regression (pols_least_squares_absorb2, K17): the yardsticks of tests/test_absorb2_*.py,
and the panels those tests share.

``map_group``     the header's definitions literally: alternating projections per column from v0 with the stop rule
                  max |m| <= tol sqrt(sum w v0^2 / sum w), the accumulated means, A = X~'X~ by Cholesky with K16's pivot rule, e~ from the
                  rows, df = n - k - (C1 + C2 - M) with M from label propagation, the effects from the accumulated means.
``lsdv2_group``   explicit dummies for both ids through np.linalg.lstsq; the rank of the dummy block by matrix_rank, M by union-find; the
                  cluster covariance as the X-rows of pinv(Z) applied to the block-diagonal e e' (by Frisch-Waugh-Lovell these rows equal
                  A^-1 X~' whatever the weighting in the middle), times q."""
import numpy as np

from absorb_ref import _chol, _chol_inverse, fitted_rows
from robust_ref import two_sided_p

OK, FALLBACK, EMPTY, NOT_CONVERGED, BAD_DOF = 0, 1, 2, 3, 4
GROUP_FIELDS = ("se", "t_values", "p_values", "sigma2", "r2_within", "r2")
COUNTS = ("n_obs", "n_categories", "n_categories2", "n_components", "n_iter", "status")
ROWS = ("pred", "resid", "fe1", "fe2")


def _sum_by(inv, C, v):
    if v.dtype == np.float64:
        return np.bincount(inv, weights=v, minlength=C)
    out = np.zeros(C, dtype=v.dtype)
    np.add.at(out, inv, v)
    return out


def components(c1, c2, C1, C2):
    """union-find over the C1 + C2 categories joined by the rows (c1[i], c2[i]): the number of components, a root per category"""
    parent = np.arange(C1 + C2)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in set(zip(c1.tolist(), (c2 + C1).tolist())):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(a) for a in range(C1 + C2)])
    return len(np.unique(roots)), roots


def _propagate(c1, c2, C1, C2):
    """labels by min-propagation over the two families of categories (the kernel's way): root id-1 category per category"""
    lab = c1.copy()
    while True:
        m1 = np.full(C1, np.iinfo(np.int64).max)
        np.minimum.at(m1, c1, lab)
        new = m1[c1]
        m2 = np.full(C2, np.iinfo(np.int64).max)
        np.minimum.at(m2, c2, new)
        new = m2[c2]
        if (new == lab).all():
            return m1, m2
        lab = new


def demean(v0, c1, c2, C1, C2, w, max_iter, tol):
    """one column: (v final, a1 [C1], a2 [C2], sweeps, stop rule fired)"""
    ft = v0.dtype.type
    W1, W2 = _sum_by(c1, C1, w), _sum_by(c2, C2, w)
    thr = ft(tol) * np.sqrt((w * v0 * v0).sum() / w.sum())
    v, a1, a2 = v0.copy(), np.zeros(C1, dtype=v0.dtype), np.zeros(C2, dtype=v0.dtype)
    for it in range(1, max_iter + 1):
        m1 = _sum_by(c1, C1, w * v) / W1
        v = v - m1[c1]
        m2 = _sum_by(c2, C2, w * v) / W2
        v = v - m2[c2]
        a1 += m1
        a2 += m2
        mx = max(np.abs(m1).max(), np.abs(m2).max())
        if mx <= thr or not np.isfinite(mx):
            return v, a1, a2, it, True
    return v, a1, a2, max_iter, False


def map_group(y, X, ids1, ids2, w=None, add_intercept=False, cov_type="nonrobust", fit=None, max_iter=10_000, tol=1e-10, ft=np.float64):
    """One group.  y [n], X [n, k] (user columns only), ids1 / ids2 [n], w [n] or None; ``fit``: the rows of the fit (None: all).
    Returns a dict: coef [k (+ 1)], se / t_values / p_values (NaN for the intercept), sigma2, r2_within, r2, the counts, status,
    pred / resid / fe1 / fe2 [n] and ``Xt`` (the demeaned, sqrt(w)-scaled regressors of the fitted rows)."""
    y, X = np.asarray(y, dtype=ft), np.asarray(X, dtype=ft)
    ids1, ids2 = np.asarray(ids1, dtype=np.int64), np.asarray(ids2, dtype=np.int64)
    N, k = X.shape
    kc = k + (1 if add_intercept else 0)
    fit = np.ones(N, dtype=bool) if fit is None else np.asarray(fit, dtype=bool)
    wv = np.ones(N, dtype=ft) if w is None else np.asarray(w, dtype=ft)
    nanv = np.full(kc, np.nan)
    out = {"coef": nanv.copy(), "se": nanv.copy(), "t_values": nanv.copy(), "p_values": nanv.copy(), "sigma2": np.nan, "r2_within": np.nan,
           "r2": np.nan, "Xt": None}
    for key in ROWS:
        out[key] = np.full(N, np.nan)
    yf, Xf, wf = y[fit], X[fit], wv[fit]
    n = int(fit.sum())
    u1, c1 = np.unique(ids1[fit], return_inverse=True)
    u2, c2 = np.unique(ids2[fit], return_inverse=True)
    C1, C2 = len(u1), len(u2)
    out.update(n_obs=n, n_categories=C1, n_categories2=C2, n_components=0, n_iter=0)
    if n == 0:
        out["coef"] = np.zeros(kc)
        out["status"] = EMPTY
        return out
    lab1, lab2 = _propagate(c1, c2, C1, C2)
    M = len(np.unique(lab1))
    out["n_components"] = M
    cols = [demean(np.ascontiguousarray(Xf[:, j]), c1, c2, C1, C2, wf, max_iter, tol) for j in range(k)]
    cols.append(demean(yf.copy(), c1, c2, C1, C2, wf, max_iter, tol))
    out["n_iter"] = max(c[3] for c in cols)
    df = n - k - (C1 + C2 - M)
    if df <= 0:
        out["status"] = BAD_DOF
        return out
    sw = np.sqrt(wf)
    Xt, yt = sw[:, None] * np.column_stack([c[0] for c in cols[:k]]), sw * cols[k][0]
    out["Xt"] = Xt
    A, T = Xt.T @ Xt, (wf[:, None] * Xf * Xf).sum(axis=0)
    L = _chol(A, T, k) if np.isfinite(np.asarray(A, dtype=np.float64)).all() and np.isfinite(np.asarray(yt, dtype=np.float64)).all() else None
    if L is None:
        out["status"] = FALLBACK
        return out
    Ainv = _chol_inverse(L)
    b = Ainv @ (Xt.T @ yt)
    et = yt - Xt @ b
    rss = (et ** 2).sum()
    a1 = cols[k][1] - np.column_stack([c[1] for c in cols[:k]]) @ b
    a2 = cols[k][2] - np.column_stack([c[2] for c in cols[:k]]) @ b
    m1 = (wf * a1[c1]).sum() / wf.sum() if add_intercept else ft(0)
    m2 = (wf * a2[c2]).sum() / wf.sum() if add_intercept else ft(0)
    sigma2 = rss / df
    if cov_type == "nonrobust":
        V, dfp = sigma2 * np.diag(Ainv), float(df)
    else:
        S = np.zeros((C1, k), dtype=Xt.dtype)
        np.add.at(S, c1, et[:, None] * Xt)
        Z = S @ Ainv
        dfp, d1 = C1 - 1.0, n - k - 1.0 - (C2 - M)
        V = (C1 / (C1 - 1.0) * (n - 1.0) / d1 * (Z ** 2).sum(axis=0)) if (C1 >= 2 and d1 > 0) else np.full(k, np.nan)
    V, b64 = np.asarray(V, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.where(V >= 0, np.sqrt(np.abs(V)), np.nan)
        t = b64 / se
    p = np.array([two_sided_p(float(tj), dfp) if np.isfinite(tj) else np.nan for tj in t])
    out["coef"][:k], out["se"][:k], out["t_values"][:k], out["p_values"][:k] = b64, se, t, p
    if add_intercept:
        out["coef"][k] = float(m1 + m2)
    ybw = (wf * yf).sum() / wf.sum()
    out["sigma2"], out["r2_within"], out["r2"] = float(sigma2), float(1 - rss / (yt ** 2).sum()), float(1 - rss / (wf * (yf - ybw) ** 2).sum())
    # every row of the group: the effects of its two categories when they lie in one component
    e1 = {int(i): (float(a), int(l)) for i, a, l in zip(u1, np.asarray(a1, dtype=np.float64), lab1)}
    e2 = {int(i): (float(a), int(l)) for i, a, l in zip(u2, np.asarray(a2, dtype=np.float64), lab2)}
    r1 = np.array([e1.get(int(i), (np.nan, -1)) for i in ids1]).reshape(N, 2)
    r2 = np.array([e2.get(int(i), (np.nan, -2)) for i in ids2]).reshape(N, 2)
    same = r1[:, 1] == r2[:, 1]
    f1, f2 = np.where(same, r1[:, 0], np.nan), np.where(same, r2[:, 0], np.nan)
    out["pred"] = np.asarray(X, dtype=np.float64) @ b64 + (f1 + f2)
    out["resid"] = np.asarray(y, dtype=np.float64) - out["pred"]
    out["fe1"], out["fe2"] = f1 - float(m1), f2 - float(m2)
    out["status"] = OK if all(c[4] for c in cols) else NOT_CONVERGED
    return out


def lsdv2_group(y, X, ids1, ids2, w=None, cov_type="nonrobust"):
    """One group through explicit dummies for both ids: dict coef [k], se [k], rank (of the dummy block), n_components, df, sigma2."""
    y, X = np.asarray(y, dtype=np.float64), np.asarray(X, dtype=np.float64)
    n, k = X.shape
    u1, c1 = np.unique(np.asarray(ids1), return_inverse=True)
    u2, c2 = np.unique(np.asarray(ids2), return_inverse=True)
    C1, C2 = len(u1), len(u2)
    D = np.column_stack([(c1[:, None] == np.arange(C1)[None, :]), (c2[:, None] == np.arange(C2)[None, :])]).astype(np.float64)
    rank = int(np.linalg.matrix_rank(D))
    M, _ = components(c1, c2, C1, C2)
    sw = np.ones(n) if w is None else np.sqrt(np.asarray(w, dtype=np.float64))
    Zs, ys = np.column_stack([X, D]) * sw[:, None], y * sw
    beta = np.linalg.lstsq(Zs, ys, rcond=None)[0]
    e = ys - Zs @ beta
    df = n - k - rank
    sigma2 = (e ** 2).sum() / df if df > 0 else np.nan
    P = np.linalg.pinv(Zs)[:k]                                      # row j: what maps y~ to b_j
    if cov_type == "nonrobust":
        V = sigma2 * (P ** 2).sum(axis=1)
    else:
        S = np.zeros((C1, k))
        np.add.at(S, c1, (P * e[None, :]).T)                        # P_c e_c per id-1 cluster
        d1 = n - k - 1.0 - (C2 - M)
        V = C1 / (C1 - 1.0) * (n - 1.0) / d1 * (S ** 2).sum(axis=0) if (C1 >= 2 and d1 > 0) else np.full(k, np.nan)
    return {"coef": beta[:k], "se": np.sqrt(V), "rank": rank, "n_components": M, "df": df, "sigma2": sigma2}


def map_batch(y, cols, offsets, ids1, ids2, weights=None, add_intercept=False, cov_type="nonrobust", policy="ignore", max_iter=10_000, tol=1e-10):
    """Every group of a group-sorted batch through map_group: coef / se / t_values / p_values [G, kc], the group fields and counts [G],
    pred / resid / fe1 / fe2 [N]."""
    offs = np.asarray(offsets)
    y = np.asarray(y, dtype=np.float64)
    keep, cols = fitted_rows(y, cols, policy)
    res = {key: [] for key in ("coef",) + GROUP_FIELDS + COUNTS}
    rows = {key: np.full(len(y), np.nan) for key in ROWS}
    for g in range(len(offs) - 1):
        s, e = int(offs[g]), int(offs[g + 1])
        X = np.column_stack([c[s:e] for c in cols]) if e > s else np.zeros((0, len(cols)))
        Xp = np.where(np.isnan(X), 0.0, X) if policy != "ignore" else X
        r = map_group(np.where(keep[s:e], y[s:e], 0.0), Xp, ids1[s:e], ids2[s:e], None if weights is None else np.asarray(weights, dtype=np.float64)[s:e],
                      add_intercept, cov_type, fit=keep[s:e], max_iter=max_iter, tol=tol)
        for key in res:
            res[key].append(r[key])
        for key in ("pred", "fe1", "fe2"):
            rows[key][s:e] = r[key]
        rows["resid"][s:e] = y[s:e] - r["pred"]
    out = {key: np.array(v) for key, v in res.items()}
    out.update(rows)
    return out


# ------------------------------------------------------------------------------------------------------------------ the shared panels
def _encode(code, mult=1_000_003, shift=-7_000_000_000):
    return (code * mult + shift).astype(np.int64)


def ragged(seed=11, dtype=np.float64, G=23, k=6, lo=50, hi=1000, n1=15, n2=8):
    """ragged groups, ids drawn per row, a shock per id of either kind; returns y, cols, offs, w, ids1, ids2"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, size=G)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    a, b = rng.integers(0, n1, size=n), rng.integers(0, n2, size=n)
    cols = [rng.normal(size=n) + 0.5 * rng.normal(size=n1)[a] + 0.5 * rng.normal(size=n2)[b] for _ in range(k)]
    y = sum((j + 1) * 0.3 * c for j, c in enumerate(cols)) + 0.5 + 2.0 * rng.normal(size=n1)[a] + rng.normal(size=n2)[b] \
        + rng.normal(size=n) * (0.5 + np.abs(cols[0]))
    w = rng.uniform(0.2, 2.0, size=n)
    return y.astype(dtype), [c.astype(dtype) for c in cols], offs, w.astype(dtype), _encode(a), _encode(b, 977, -5_000_000_000)


def sort_within_groups(offs, ids, *cols):
    order = np.concatenate([s + np.argsort(ids[s:e], kind="stable") for s, e in zip(offs[:-1], offs[1:])])
    return [a[order] for a in (ids,) + cols]


def balanced(seed=3, n1=12, n2=8, k=3):
    """a complete panel, one row per cell, rows shuffled: y, X, ids1, ids2"""
    rng = np.random.default_rng(seed)
    a, b = [v.ravel() for v in np.meshgrid(np.arange(n1), np.arange(n2), indexing="ij")]
    perm = rng.permutation(n1 * n2)
    a, b = a[perm], b[perm]
    X = rng.normal(size=(n1 * n2, k)) + rng.normal(size=(n1, k))[a] + rng.normal(size=(n2, k))[b]
    y = X @ np.arange(1.0, k + 1) + rng.normal(size=n1)[a] + rng.normal(size=n2)[b] + rng.normal(size=n1 * n2)
    return y, X, _encode(a), _encode(b, 977, 0)


def two_blocks(seed=4, n1=16, n2=10, k=3, reps=2):
    """16 x 10 cells with the off-diagonal blocks removed (firms 0-7 meet periods 0-4 only, firms 8-15 periods 5-9), reps rows per
    cell, then four rows with a null target: two straddle the blocks, two lie inside one.  y, X, ids1, ids2, the four rows' indices"""
    rng = np.random.default_rng(seed)
    a, b = [v.ravel() for v in np.meshgrid(np.arange(n1), np.arange(n2), indexing="ij")]
    keep = (a < n1 // 2) == (b < n2 // 2)
    a, b = np.repeat(a[keep], reps), np.repeat(b[keep], reps)
    a, b = np.concatenate([a, [0, 9, 3, 12]]), np.concatenate([b, [7, 1, 2, 8]])
    n = len(a)
    X = rng.normal(size=(n, k)) + rng.normal(size=(n1, k))[a]
    y = X @ np.arange(1.0, k + 1) + rng.normal(size=n1)[a] + rng.normal(size=n2)[b] + rng.normal(size=n)
    y[-4:] = np.nan
    return y, X, _encode(a), _encode(b, 977, 0), np.arange(n - 4, n)


def chain(links=12, reps=3, k=2, seed=6):
    """firm i observed in periods i and i + 1, reps rows per cell: the slowest panel for alternating projections"""
    rng = np.random.default_rng(seed)
    a = np.repeat(np.arange(links), 2 * reps)
    b = a + np.tile(np.repeat([0, 1], reps), links)
    n = len(a)
    X = rng.normal(size=(n, k)) + 0.5 * np.arange(links)[a][:, None] * np.array([1.0, -1.0])[:k]
    y = X @ np.arange(1.0, k + 1) + rng.normal(size=links)[a] + rng.normal(size=links + 1)[b] + rng.normal(size=n)
    return y, X, _encode(a), _encode(b, 977, 0)


def shifted(seed=5, n=900, n1=30, n2=12, k=5, shift=1e4):
    """effects 1e4 x the within spread: y, X, ids1, ids2, w"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n1, size=n), rng.integers(0, n2, size=n)
    X = rng.normal(size=(n, k)) + shift * rng.normal(size=(n1, k))[a] + shift * rng.normal(size=(n2, k))[b]
    y = X @ (0.3 * np.arange(1, k + 1)) + shift * rng.normal(size=n1)[a] + shift * rng.normal(size=n2)[b] + rng.normal(size=n)
    return y, X, _encode(a), _encode(b, 977, 0), rng.uniform(0.2, 2.0, size=n)


def long_group(seed=8, n=40_000, k=3, n1=200, n2=50):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n1, size=n), rng.integers(0, n2, size=n)
    cols = [rng.normal(size=n) + rng.normal(size=n1)[a] + rng.normal(size=n2)[b] for _ in range(k)]
    y = sum((j + 1) * 0.2 * c for j, c in enumerate(cols)) + rng.normal(size=n1)[a] + rng.normal(size=n2)[b] + rng.normal(size=n)
    return y, cols, np.array([0, n], dtype=np.int64), rng.uniform(0.5, 2.0, size=n), _encode(a), _encode(b, 977, 0)
