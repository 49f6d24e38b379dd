"""CPU checks of the ridge regularisation path (pols_ridge_cv, K10): the numpy restatement in ridge_cv_ref.py against brute-force
leave-one-out refits and scikit-learn's RidgeCV; the library's defaults, header and code objects; the front end's validation."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

from ridge_cv_ref import EMPTY, FALLBACK, OK, chosen_outputs, fit_rows, loo_brute_force, ridge_cv_batch

ROOT = Path(__file__).resolve().parent.parent
ALPHAS = np.logspace(-2, 4, 13)


def _frame(seed, sizes, k, nan_share=0.0):
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    X = rng.normal(size=(n, k))
    y = X @ (0.5 * rng.normal(size=k)) + 0.3 + rng.normal(size=n)
    w = rng.uniform(0.2, 2.0, size=n)
    if nan_share:
        y[rng.random(n) < nan_share] = np.nan
        X[rng.random((n, k)) < nan_share / k] = np.nan
    return y, [X[:, j].copy() for j in range(k)], offs, w


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("policy", ["ignore", "drop"])
def test_scores_are_brute_force_leave_one_out_refits(weighted, intercept, policy):
    y, cols, offs, w = _frame(3, [9, 17, 30, 12, 25], 4, nan_share=0.1 if policy == "drop" else 0.0)
    w = w if weighted else None
    alphas = [0.0, 0.05, 1.0, 30.0]
    ref = ridge_cv_batch(y, cols, offs, alphas, w, add_intercept=intercept, null_policy=policy)
    fit, yy, X, ww = fit_rows(y, np.column_stack(cols), w, policy)
    if intercept:
        X = np.column_stack([X, np.ones(len(y))])
    sw = np.ones(len(y)) if ww is None else np.sqrt(ww)
    worst = 0.0
    for g in range(len(offs) - 1):
        rows = np.arange(offs[g], offs[g + 1])[fit[offs[g]:offs[g + 1]]]
        assert ref["n"][g] == len(rows) > X.shape[1]
        for j, a in enumerate(alphas):
            bf = loo_brute_force(yy[rows] * sw[rows], X[rows] * sw[rows, None], a)
            worst = max(worst, abs(ref["cv_scores"][g, j] - bf) / bf)
    print(f"max rel err against refits: {worst:.3e}")
    assert worst < 1e-9
    assert (ref["status"] == OK).all() and (ref["alpha_index"] >= 0).all()
    if policy == "drop":
        assert not fit.all()


@pytest.mark.parametrize("k", [3, 8])
def test_unweighted_scores_and_choice_are_sklearns(k):
    from sklearn.linear_model import RidgeCV

    y, cols, offs, _ = _frame(4, [40, 75, 120, 64], k)
    ref = ridge_cv_batch(y, cols, offs, ALPHAS)
    X = np.column_stack(cols)
    for g in range(len(offs) - 1):
        s, e = offs[g], offs[g + 1]
        m = RidgeCV(alphas=ALPHAS, fit_intercept=False, store_cv_results=True).fit(X[s:e], y[s:e])
        np.testing.assert_allclose(ref["cv_scores"][g], m.cv_results_.mean(axis=0), rtol=1e-10)
        assert ref["alpha"][g] == m.alpha_
        np.testing.assert_allclose(ref["coef_path"][g, ref["alpha_index"][g]], m.coef_, rtol=1e-8)


def test_unusable_candidates_ties_and_statuses():
    y, cols, offs, _ = _frame(5, [30, 3, 0, 30, 30], 4)
    cols[3][offs[3]:offs[4]] = cols[2][offs[3]:offs[4]]        # group 3: an exactly duplicated column
    ref = ridge_cv_batch(y, cols, offs, [0.0, 1.0, 1.0, 0.5])
    sc = ref["cv_scores"]
    assert np.isfinite(sc[0]).all()
    assert np.isnan(sc[1, 0]) and np.isfinite(sc[1, 1:]).all()          # n <= kt: alpha = 0 is an exact fit
    assert np.isnan(sc[2]).all() and ref["status"][2] == EMPTY and ref["alpha_index"][2] == -1
    assert np.isnan(sc[3, 0]) and np.isfinite(sc[3, 1:]).all()          # singular X'X
    assert sc[0, 1] == sc[0, 2] and ref["alpha_index"][0] != 2          # a repeated value: the lower index
    only0 = ridge_cv_batch(y, cols, offs, [0.0])
    assert list(only0["status"]) == [OK, FALLBACK, EMPTY, FALLBACK, OK]
    assert list(only0["alpha_index"]) == [0, -1, -1, -1, 0]
    coef, pred, _ = chosen_outputs(only0, only0["alpha_index"], y, cols, offs)
    assert np.isnan(coef[1]).all() and np.isnan(pred[offs[1]:offs[2]]).all() and np.isfinite(pred[offs[4]:]).all()


# ---------------------------------------------------------------- library and front end
@pytest.fixture(scope="module")
def L():
    from polars_ols_amd import _lib

    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


def test_params_default(L):
    from polars_ols_amd import _lib

    q = _lib.RidgeCvParams(alphas=(C.c_double * 2)(1.0, 2.0), n_alphas=2)
    L.pols_ridge_cv_params_default(C.byref(q))
    assert not q.alphas and q.n_alphas == 0
    L.pols_ridge_cv_params_default(None)
    assert {"pols_ridge_cv", "pols_ridge_cv_params_default"} <= set(_lib.EXPORTS)
    assert [f for f, _ in _lib.RidgeCvOut._fields_] == ["alpha", "alpha_index", "score", "cv_scores", "coef_path"]


def test_header_compiles_as_c99_with_the_new_structs(tmp_path, L):
    import shutil
    import subprocess

    from polars_ols_amd import _lib

    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    src = tmp_path / "consumer.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "pols_mi355x.h"\n'
        "int main(void) {\n"
        "    double grid[2] = {0.1, 1.0};\n"
        "    pols_ridge_cv_params q; pols_ridge_cv_out o = {0};\n"
        "    q.alphas = grid; q.n_alphas = 2;\n"
        "    pols_ridge_cv_params_default(&q);\n"
        "    if (q.alphas != NULL || q.n_alphas != 0 || o.coef_path != NULL) return 1;\n"
        "    if (pols_ridge_cv(NULL, NULL, NULL, &q, NULL, &o) != POLS_ERR_INVALID) return 2;\n"
        '    printf("%d %d\\n", (int)sizeof(pols_ridge_cv_params), (int)(sizeof(pols_ridge_cv_out) / sizeof(void *)));\n'
        "    return 0;\n}\n")
    exe = tmp_path / "consumer"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                    f"-L{_lib.LIB_PATH.parent}", "-lpols_mi355x", f"-Wl,-rpath,{_lib.LIB_PATH.parent}"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(C.sizeof(_lib.RidgeCvParams)), "5"], out


def test_k10_kernels_use_no_scratch_and_no_agprs(L):
    from polars_ols_amd import _lib

    sys.path.insert(0, str(ROOT / "scripts"))
    from check_scratch import LLVM, kernel_scratch

    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("ROCm LLVM tools not present")
    ks = {k: v for k, v in kernel_scratch(_lib.LIB_PATH).items() if "k10_" in k}
    # gram (2 dtypes), eig, pick, rows: 2 dtypes x (16 unrolled widths + the run-time build), predict (2 dtypes)
    assert len(ks) == 2 + 1 + 1 + 2 * 17 + 2, sorted(ks)
    for name, (scratch, vgpr, agpr) in ks.items():
        assert scratch == 0 and agpr == 0 and vgpr > 0, (name, scratch, vgpr, agpr)


def test_namespace_builds_expressions_and_rejects_bad_requests():
    import polars_ols_amd as P

    e = P.col("y").least_squares.ridge_cv(P.col("a"), "b", alphas=[0.1, 1.0], add_intercept=True, mode="cv")
    assert isinstance(e, P.Expr) and isinstance(e.over("k"), P.Expr)
    assert isinstance(P.compute_ridge_cv("y", "a", alphas=np.array([1.0]), mode="coefficients"), P.Expr)
    assert issubclass(P.RidgeCV, dict)
    for bad in ([], [-1.0, 1.0], [float("nan")], [float("inf")], np.zeros((0,))):
        with pytest.raises(ValueError):
            P.col("y").least_squares.ridge_cv("a", alphas=bad)
        with pytest.raises(ValueError):
            P.compute_ridge_cv("y", "a", alphas=bad)
    with pytest.raises(ValueError):
        P.col("y").least_squares.ridge_cv("a", alphas=[1.0], mode="statistics")
    with pytest.raises(ValueError):
        P.col("y").least_squares.ridge_cv("a", alphas=[1.0], null_policy="skip")
    with pytest.raises(TypeError):
        P.col("y").least_squares.ridge_cv("a")                                   # alphas is required
    # ridge(alpha=float) is what it was
    assert isinstance(P.col("y").least_squares.ridge("a", alpha=0.5), P.Expr)


def test_engine_rejects_bad_requests_before_any_device_call():
    """Engine.ridge_cv validates the grid and the field names first: no context is needed to be told"""
    from polars_ols_amd.engine import Engine

    eng = Engine.__new__(Engine)                                                 # no device behind it
    y, cols, offs, _ = _frame(6, [10, 10], 2)
    for bad in ([], [-0.5], [1.0, float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            eng.ridge_cv(y, cols, offs, bad)
    with pytest.raises(ValueError):
        eng.ridge_cv(y, cols, offs, [1.0], want=("coef", "leverage"))
