"""numpy restatement of the cluster-robust standard errors of mode="statistics" (cov_type "cluster", one- and two-way): the yardstick
of tests/test_cluster_stats_*.py.  Per group, f64, on the sqrt(w)-scaled rows with the ones column last:
A = X'X + alpha I, b = A^-1 X'y, e = y - X b, u_i = e_i x_i;  per clustering: s_c = sum_{i in c} u_i, z_c = A^-1 s_c,
S = sum_c z_c^2 (elementwise), q = G / (G - 1) (N - 1) / df (use_correction) or 1;  one-way V = q S, two-way
V = q_A S_A + q_B S_B - q_AB S_AB;  se = sqrt(V), t = b / se, p two-sided Student-t with G - 1 (two-way min(G_A, G_B) - 1) df.
NaN when G < 2 (two-way min(G_A, G_B) < 2), df <= 0 with the correction, or A is not positive definite; two-way, V_jj < 0 is NaN
for that coefficient alone."""
import numpy as np

from robust_ref import two_sided_p


def _sums(Z_rows, ids):
    """sum over the clusters of ids (np.unique, ascending) of (A^-1 s_c)^2, and G; Z_rows = u_i A^-1 (A^-1 is symmetric)."""
    uniq, inv = np.unique(ids, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    G = len(uniq)
    Zc = np.zeros((G, Z_rows.shape[1]))
    for c in range(G):                                         # s_c then A^-1 s_c, cluster by cluster (the definition)
        Zc[c] = Z_rows[inv == c].sum(axis=0)
    return (Zc ** 2).sum(axis=0), G


def cluster_group(y, X, ids_a, ids_b=None, w=None, alpha=0.0, use_correction=True):
    """One group: y [n], X [n, k] (the ones column, if any, already appended last), ids_a [n] (and ids_b [n] for two-way), w [n] or
    None.  Returns se, t, p [k] and the cluster counts (G,) or (G_A, G_B)."""
    y = np.asarray(y, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    n, k = X.shape
    nan = np.full(k, np.nan)
    ids_a = np.asarray(ids_a, dtype=np.int64)
    two = ids_b is not None
    Ga = len(np.unique(ids_a))
    Gb = len(np.unique(np.asarray(ids_b, dtype=np.int64))) if two else None
    counts = (Ga, Gb) if two else (Ga,)
    if w is not None:
        sw = np.sqrt(np.asarray(w, dtype=np.float64))
        X, y = X * sw[:, None], y * sw
    A = X.T @ X + alpha * np.eye(k)
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return nan, nan.copy(), nan.copy(), counts
    Li = np.linalg.inv(Lc)
    Ainv = Li.T @ Li
    b = Ainv @ (X.T @ y)
    df = n - np.trace(Ainv) if alpha > 0 else float(n - k)
    gmin = min(Ga, Gb) if two else Ga
    if gmin < 2 or (use_correction and not df > 0):
        return nan, nan.copy(), nan.copy(), counts
    e = y - X @ b
    Z = (e[:, None] * X) @ Ainv                                # row i: (A^-1 u_i)'

    def q(G):
        return G / (G - 1.0) * (n - 1.0) / df if use_correction else 1.0

    Sa, _ = _sums(Z, ids_a)
    V = q(Ga) * Sa
    if two:
        ids_b = np.asarray(ids_b, dtype=np.int64)
        Sb, _ = _sums(Z, ids_b)
        Sab, Gab = _sums(Z, np.column_stack([ids_a, ids_b]))
        V = V + q(Gb) * Sb - q(Gab) * Sab
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.where(V >= 0, np.sqrt(np.abs(V)), np.nan)
        t = b / se
    dfp = gmin - 1.0
    p = np.array([two_sided_p(float(tj), dfp) for tj in t])
    return se, t, p, counts


def cluster_batch(y, cols, offsets, ids_a, ids_b=None, weights=None, add_intercept=False, alpha=0.0, use_correction=True):
    """Every group of a group-sorted batch: dict std_err / t_values / p_values [G, k], n_clusters [G] or [G, 2]."""
    offs = np.asarray(offsets)
    out = {"std_err": [], "t_values": [], "p_values": [], "n_clusters": []}
    for g in range(len(offs) - 1):
        s, e = int(offs[g]), int(offs[g + 1])
        X = np.column_stack([np.asarray(c[s:e], dtype=np.float64) for c in cols]) if cols else np.zeros((e - s, 0))
        if add_intercept:
            X = np.column_stack([X, np.ones(e - s)])
        se, t, p, cnt = cluster_group(y[s:e], X, ids_a[s:e], None if ids_b is None else ids_b[s:e],
                                      None if weights is None else weights[s:e], alpha, use_correction)
        out["std_err"].append(se)
        out["t_values"].append(t)
        out["p_values"].append(p)
        out["n_clusters"].append(cnt if ids_b is not None else cnt[0])
    return {k: np.array(v) for k, v in out.items()}


def kept_rows(y, cols, policy):
    """Rows a null policy keeps (NaN = null): "drop" every row with a NaN target or feature, "drop_y_zero_x" every row with a NaN
    target (its NaN features become 0).  Returns the mask and the features as the policy leaves them."""
    y = np.asarray(y, dtype=np.float64)
    cols = [np.asarray(c, dtype=np.float64) for c in cols]
    keep = ~np.isnan(y)
    if policy == "drop":
        for c in cols:
            keep &= ~np.isnan(c)
    elif policy == "drop_y_zero_x":
        cols = [np.where(np.isnan(c), 0.0, c) for c in cols]
    else:
        raise ValueError(policy)
    return keep, cols
