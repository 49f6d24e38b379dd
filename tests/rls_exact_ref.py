"""A high-precision restatement of recursive least squares (least_squares.rs:494-598) in its information form, for the tests
of frames on which a regressor falls silent.

By Sherman-Morrison the reference's covariance update P' = P / ff - k k' r is the decayed sum
    A_t = ff A_{t-1} + x_t x_t',   b_t = ff b_{t-1} + x_t y_t,   beta_t = A_t^-1 b_t,
started at every sequence's first row from A_0 = I / p0, b_0 = mean0 / p0.  Here every sum is carried in `decimal` at a precision
chosen for the frame, so nothing underflows (decimal's exponent range is far beyond f64's) and a column that is zero for s rows keeps
its decayed information ff^s exactly; the state is solved only at the rows asked for, by Gaussian elimination with partial pivoting.
Predictions are x_t . beta_t with the same row's coefficients (orc_predict_dynamic).  The inputs are taken as the f64 values they hold
and ff is the f64 value the kernels use, exp(log(0.5) / half_life): what is exact is the recursion, not the data."""
from __future__ import annotations

import math
from decimal import Decimal, localcontext

import numpy as np


def forgetting_factor(half_life):
    return 1.0 if half_life is None else math.exp(math.log(0.5) / half_life)


def precision_for(half_life, longest_silence_rows: int) -> int:
    """Digits that keep a column silent for `longest_silence_rows` rows exact through the solve: 40 + ceil(rows log10(2) / half_life)."""
    if half_life is None:
        return 40
    return 40 + int(math.ceil(longest_silence_rows * math.log10(2.0) / half_life))


def _solve(A, b, k):
    """Gaussian elimination with partial pivoting on the k x k system (A given as full rows of Decimals; consumed)."""
    M = [A[i][:] + [b[i]] for i in range(k)]
    for c in range(k):
        p = max(range(c, k), key=lambda r: abs(M[r][c]))
        if M[p][c] == 0:
            return None
        if p != c:
            M[c], M[p] = M[p], M[c]
        piv = M[c][c]
        for r in range(c + 1, k):
            f = M[r][c] / piv
            if f:
                Mr, Mc = M[r], M[c]
                for j in range(c, k + 1):
                    Mr[j] -= f * Mc[j]
    beta = [Decimal(0)] * k
    for c in range(k - 1, -1, -1):
        s = M[c][k]
        for j in range(c + 1, k):
            s -= M[c][j] * beta[j]
        beta[c] = s / M[c][c]
    return beta


def exact_rls(y, x_cols, group_offsets, rows, half_life=None, initial_state_covariance=10.0, initial_state_mean=None,
              digits: int = 60):
    """Coefficients (len(rows) x k) and predictions (len(rows)) of every sequence's RLS at the frame rows `rows`, as f64 values of
    the exact answer.  A singular state (no information at all, not possible with a positive p0) gives NaN."""
    y = np.asarray(y, dtype=np.float64)
    X = np.stack([np.asarray(c, dtype=np.float64) for c in x_cols], axis=1)
    N, k = X.shape
    offs = np.asarray(group_offsets, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    want = np.zeros(N, dtype=bool)
    want[rows] = True
    coef = {}
    tri = [(p, q) for p in range(k) for q in range(p, k)]
    with localcontext() as ctx:
        ctx.prec = digits
        ff = Decimal(forgetting_factor(half_life))
        ip0 = Decimal(1) / Decimal(float(initial_state_covariance))
        m0 = [Decimal(float(v)) for v in initial_state_mean] if initial_state_mean is not None else [Decimal(0)] * k
        zero = Decimal(0)
        for g in range(len(offs) - 1):
            s, e = int(offs[g]), int(offs[g + 1])
            if s >= e or not want[s:e].any():
                continue
            last = s + int(np.nonzero(want[s:e])[0][-1])
            A = [ip0 if p == q else zero for (p, q) in tri]
            b = [m * ip0 for m in m0]
            for t in range(s, last + 1):
                xr = [Decimal(float(v)) for v in X[t]]
                yr = Decimal(float(y[t]))
                for i, (p, q) in enumerate(tri):
                    A[i] = ff * A[i] + xr[p] * xr[q]
                for p in range(k):
                    b[p] = ff * b[p] + xr[p] * yr
                if want[t]:
                    full = [[zero] * k for _ in range(k)]
                    for i, (p, q) in enumerate(tri):
                        full[p][q] = full[q][p] = A[i]
                    beta = _solve(full, b, k)
                    coef[t] = beta
        out_c = np.full((len(rows), k), np.nan)
        out_p = np.full(len(rows), np.nan)
        for i, t in enumerate(rows):
            beta = coef.get(int(t))
            if beta is None:
                continue
            out_c[i] = [float(v) for v in beta]
            pr = sum((Decimal(float(X[t, j])) * beta[j] for j in range(k)), zero)
            out_p[i] = float(pr)
    return {"coef": out_c, "pred": out_p}
