"""The numpy restatement of the elastic-net path with K-fold selection (enet_cv_ref.py, the yardstick of test_enet_cv_gpu.py) pinned
without a device: against scikit-learn's LassoCV / ElasticNetCV, its fold rule against KFold.split, "drop" against filter-then-fit,
equivariance under a rescaled target, every status rule, the front end's ValueErrors, and the library's defaults, header and code
objects."""
import numpy as np
import pytest

from enet_cv_ref import EMPTY, FALLBACK, NOT_CONVERGED, OK, enet_cv_batch, fold_ids


def gen(G, lo, hi, k, dtype=np.float64, seed=11, sigma=1.0, nonneg=False):
    """n ~ U{lo..hi} per group, X ~ N(0, 1) with columns 0 / 1 correlated, half the true coefficients zero (nonneg: the others
    positive, so that a `positive` fit is not a run of all-zero candidates with exactly tied scores)"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, size=G)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    X = rng.normal(size=(n, k))
    if k > 1:
        X[:, 1] = X[:, 0] + 0.3 * X[:, 1]
    beta = rng.normal(size=(G, k))
    beta[:, 1::2] = 0.0
    if nonneg:
        beta = np.abs(beta)
    y = (X * np.repeat(beta, sizes, axis=0)).sum(axis=1) + sigma * rng.normal(size=n)
    w = rng.uniform(0.2, 2.0, size=n)
    return y.astype(dtype), [X[:, j].astype(dtype) for j in range(k)], offs, w.astype(dtype)


@pytest.mark.parametrize("l1_ratio,positive,F", [(1.0, False, 5), (0.5, False, 5), (0.9, False, 3), (1.0, True, 4)])
def test_against_scikit_learn(l1_ratio, positive, F):
    sklearn = pytest.importorskip("sklearn")
    from sklearn.linear_model import ElasticNetCV, LassoCV
    from sklearn.model_selection import KFold

    rng = np.random.default_rng(3)
    sizes = rng.integers(30, 401, size=4)
    ks = rng.integers(6, 13, size=4)
    n_exempt = 0
    for n, k in zip(sizes, ks):
        y, cols, offs, _ = gen(1, n, n, int(k), seed=int(n), sigma=3.0, nonneg=positive)
        X = np.column_stack(cols)
        A = 30
        ref = enet_cv_batch(y, cols, offs, None, n_alphas=A, eps=1e-3, l1_ratio=l1_ratio, n_folds=F, max_iter=100000, tol=1e-10,
                            positive=positive)
        kw = dict(alphas=A, eps=1e-3, fit_intercept=False, cv=KFold(F), tol=1e-12, max_iter=1000000, positive=positive)
        try:
            m = (LassoCV(**kw) if l1_ratio == 1.0 else ElasticNetCV(l1_ratio=l1_ratio, **kw)).fit(X, y)
        except (TypeError, ValueError):                            # (older releases spell the grid size `n_alphas`)
            kw["n_alphas"] = kw.pop("alphas")
            m = (LassoCV(**kw) if l1_ratio == 1.0 else ElasticNetCV(l1_ratio=l1_ratio, **kw)).fit(X, y)
        assert ref["status"][0] == OK
        np.testing.assert_allclose(ref["alphas_used"][0], m.alphas_, rtol=1e-12)
        mse = m.mse_path_.mean(axis=1)
        print(f"n {n} k {k}: mse max rel {np.max(np.abs(ref['cv_scores'][0] - mse) / mse):.2e}")
        np.testing.assert_allclose(ref["cv_scores"][0], mse, rtol=1e-7)
        srt = np.sort(mse)
        if srt[1] > srt[0] * (1.0 + 1e-5):
            assert ref["alpha_index"][0] == int(np.argmin(mse)) and ref["alpha"][0] == pytest.approx(m.alpha_, rel=1e-12)
            np.testing.assert_allclose(ref["coef_path"][0, ref["alpha_index"][0]], m.coef_, rtol=1e-6, atol=1e-9)
        else:
            n_exempt += 1
    print(f"undecided winners: {n_exempt} of {len(sizes)}")
    assert n_exempt <= 1
    del sklearn


@pytest.mark.parametrize("F", [2, 3, 5, 16])
def test_fold_rule_is_kfold(F):
    pytest.importorskip("sklearn")
    from sklearn.model_selection import KFold

    for n in range(F, 3 * F + 2):
        fid = fold_ids(n, F)
        assert len(fid) == n
        for f, (_, test) in enumerate(KFold(F).split(np.zeros(n))):
            np.testing.assert_array_equal(np.nonzero(fid == f)[0], test)


def test_fold_rule_by_hand():
    np.testing.assert_array_equal(fold_ids(7, 3), [0, 0, 0, 1, 1, 2, 2])
    np.testing.assert_array_equal(fold_ids(6, 3), [0, 0, 1, 1, 2, 2])
    np.testing.assert_array_equal(fold_ids(3, 3), [0, 1, 2])


KEYS = ("cv_scores", "alphas_used", "coef_path", "alpha_index", "alpha", "score", "status", "n_iter")


@pytest.mark.parametrize("policy", ["drop", "drop_zero", "drop_y_zero_x"])
def test_drop_equals_filter_then_fit(policy):
    y, cols, offs, w = gen(5, 40, 90, 6, seed=2)
    rng = np.random.default_rng(9)
    N = len(y)
    y = y.copy()
    y[rng.random(N) < 0.1] = np.nan
    if policy != "drop_y_zero_x":
        for c in cols:
            c[rng.random(N) < 0.03] = np.nan
    valid = (rng.random(N) < 0.9).astype(np.uint8)
    kw = dict(n_alphas=12, l1_ratio=0.7, n_folds=4, tol=1e-9, max_iter=10000, add_intercept=True)
    got = enet_cv_batch(y, cols, offs, None, weights=w, null_policy=policy, valid=valid, **kw)
    keep = got["fit"]
    ids = np.repeat(np.arange(5), np.diff(offs))[keep]
    offs2 = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=5))])
    cols2 = [np.nan_to_num(c[keep], nan=0.0) for c in cols]
    ref = enet_cv_batch(y[keep], cols2, offs2, None, weights=w[keep], **kw)
    assert keep.sum() < N and (ref["n"] == got["n"]).all()
    for key in KEYS:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)


def test_equivariance_under_a_rescaled_target():
    y, cols, offs, w = gen(4, 40, 120, 7, seed=4)
    base = enet_cv_batch(y, cols, offs, None, n_alphas=10, l1_ratio=1.0, tol=1e-12, max_iter=100000, weights=w)
    c = 7.5                                                        # (the lasso: with an L2 term the penalty does not scale with y)
    for g in range(4):
        sl = slice(offs[g], offs[g + 1])
        a = enet_cv_batch(y[sl], [x[sl] for x in cols], [0, offs[g + 1] - offs[g]], base["alphas_used"][g], l1_ratio=1.0, tol=1e-12,
                          max_iter=100000, weights=w[sl])
        b = enet_cv_batch(c * y[sl], [x[sl] for x in cols], [0, offs[g + 1] - offs[g]], c * base["alphas_used"][g], l1_ratio=1.0,
                          tol=1e-12 * c, max_iter=100000, weights=w[sl])
        np.testing.assert_allclose(a["cv_scores"], base["cv_scores"][g:g + 1], rtol=1e-9)
        np.testing.assert_allclose(b["coef_path"], c * a["coef_path"], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(b["cv_scores"], c * c * a["cv_scores"], rtol=1e-8)
        assert b["alpha_index"][0] == a["alpha_index"][0]


def test_gram_form_validation_error_is_the_residual_form():
    y, cols, offs, _ = gen(1, 103, 103, 6, seed=6)
    F = 5
    ref = enet_cv_batch(y, cols, offs, None, n_alphas=8, n_folds=F, tol=1e-10, max_iter=100000)
    X = np.column_stack(cols)
    fid = fold_ids(103, F)
    # refit fold 2 at candidate 5 from the path's own definition: cold start at a tight tolerance, then residuals
    from enet_cv_ref import cd_path
    tr, te = fid != 2, fid == 2
    alphas = ref["alphas_used"][:, :6]
    path, _, _ = cd_path((X[tr].T @ X[tr])[None], (X[tr].T @ y[tr])[None], np.array([tr.sum()], dtype=np.float64), alphas, np.arange(6),
                         np.array([True]), 0.5, 100000, 1e-13, False)
    direct = np.mean((y[te] - X[te] @ path[0, 5]) ** 2)
    assert ref["fold_scores"][0, 2, 5] == pytest.approx(direct, rel=1e-8)


def test_every_status_rule():
    y, cols, offs, _ = gen(1, 200, 200, 4, seed=8)
    sizes = np.array([0, 3, 5, 6, 60, 40, 50])                     # empty, n < folds, n == folds, folds < n <= kt ...
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    y, cols = y[:n].copy(), [c[:n] for c in cols]
    y[offs[5]:offs[6]] = 0.0                                       # a constant-zero target: alpha_max = 0, no automatic grid
    kw = dict(n_alphas=6, n_folds=5, add_intercept=True, tol=1e-9, max_iter=10000)
    ref = enet_cv_batch(y, cols, offs, None, **kw)
    np.testing.assert_array_equal(ref["status"], [EMPTY, FALLBACK, OK, OK, OK, FALLBACK, OK])
    np.testing.assert_array_equal(ref["alpha_index"] >= 0, [False, False, True, True, True, False, True])
    for g in (0, 1, 5):
        assert np.isnan(ref["cv_scores"][g]).all() and np.isnan(ref["alphas_used"][g]).all() and np.isnan(ref["coef_path"][g]).all()
        assert (ref["n_iter"][g] == 0).all() and np.isnan(ref["alpha"][g]) and np.isnan(ref["score"][g])
    # an explicit grid: the zero target is fitted (all-zero path), the candidates come back as passed
    grid = np.array([0.1, 1.0, 0.01])
    ex = enet_cv_batch(y, cols, offs, grid, n_folds=5, add_intercept=True)
    np.testing.assert_array_equal(ex["status"], [EMPTY, FALLBACK, OK, OK, OK, OK, OK])
    np.testing.assert_array_equal(ex["alphas_used"], np.tile(grid, (7, 1)))
    assert ex["alpha_index"][5] == 0 and (ex["coef_path"][5] == 0.0).all()
    # max_iter = 1: the stop rule cannot fire on a moving path
    one = enet_cv_batch(y, cols, offs, None, n_alphas=6, n_folds=5, add_intercept=True, max_iter=1)
    assert one["status"][4] == NOT_CONVERGED and one["alpha_index"][4] >= 0 and (one["n_iter"][4] == 1).all()
    assert np.isfinite(one["coef_path"][4]).all()


def test_duplicates_and_unsorted_grids_follow_descending_order():
    y, cols, offs, _ = gen(3, 50, 80, 5, seed=12)
    srt = np.array([1.0, 0.3, 0.3, 0.1, 0.03, 0.01])
    perm = np.array([3, 1, 5, 0, 2, 4])
    a = enet_cv_batch(y, cols, offs, srt, tol=1e-12, max_iter=100000)
    b = enet_cv_batch(y, cols, offs, srt[perm], tol=1e-12, max_iter=100000)
    np.testing.assert_allclose(b["cv_scores"], a["cv_scores"][:, perm], rtol=1e-9)
    # the repeat is warm-started from its twin's solution: one more sweep confirms it
    assert (a["n_iter"][:, 2] == 1).all() and (a["n_iter"][:, 1] > 1).all()
    np.testing.assert_allclose(a["cv_scores"][:, 2], a["cv_scores"][:, 1], rtol=1e-10)


def test_front_end_refuses_bad_arguments_without_a_device():
    from polars_ols_amd import compute_elastic_net_cv
    from polars_ols_amd.engine import _enet_cv_params

    bad = [dict(l1_ratio=-0.1), dict(l1_ratio=1.5), dict(l1_ratio=float("nan")), dict(alphas=[1.0, -1.0]), dict(alphas=[float("inf")]),
           dict(alphas=[]), dict(n_alphas=1), dict(eps=0.0), dict(eps=1.0), dict(l1_ratio=0.0), dict(n_folds=1), dict(n_folds=17),
           dict(max_iter=0), dict(tol=0.0), dict(tol=float("inf")), dict(alphas=np.ones(129)), dict(n_alphas=129),
           dict(mode="statistics"), dict(null_policy="nope")]
    for kw in bad:
        with pytest.raises(ValueError):
            compute_elastic_net_cv("y", "x", **kw)
    q, grid = _enet_cv_params(None, [0.5, 2.0], 100, 1e-3, 0.0, 5, 1000, 1e-5, True)   # (l1_ratio 0 is legal with an explicit grid)
    assert q.n_alphas == 2 and q.positive == 1 and grid.tolist() == [0.5, 2.0]
    q, grid = _enet_cv_params(None, None, 100, 1e-3, 0.5, 5, 1000, 1e-5, False)
    assert grid is None and not q.alphas and (q.n_alphas, q.n_folds, q.max_iter) == (100, 5, 1000)


# ---------------------------------------------------------------- the library without a device
@pytest.fixture(scope="module")
def L():
    from polars_ols_amd import _lib

    return _lib.lib()


def test_defaults_exports_and_struct_order(L):
    import ctypes as C

    from polars_ols_amd import _lib

    q = _lib.EnetCvParams(alphas=(C.c_double * 2)(1.0, 2.0), n_alphas=2)
    L.pols_enet_cv_params_default(C.byref(q))
    assert not q.alphas
    assert (q.n_alphas, q.eps, q.l1_ratio, q.n_folds, q.max_iter, q.tol, q.positive) == (100, 1e-3, 0.5, 5, 1000, 1e-5, 0)
    L.pols_enet_cv_params_default(None)
    assert {"pols_elastic_net_cv", "pols_enet_cv_params_default"} <= set(_lib.EXPORTS)
    assert [f for f, _ in _lib.EnetCvOut._fields_] == ["alpha", "alpha_index", "score", "cv_scores", "alphas_used", "coef_path", "n_iter"]


def test_header_compiles_as_c99_with_the_new_structs(tmp_path, L):
    import ctypes as C
    import shutil
    import subprocess
    from pathlib import Path

    from polars_ols_amd import _lib

    root = Path(__file__).resolve().parent.parent
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    src = tmp_path / "consumer.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "pols_mi355x.h"\n'
        "int main(void) {\n"
        "    pols_enet_cv_params q; pols_enet_cv_out o = {0};\n"
        "    pols_enet_cv_params_default(&q);\n"
        "    if (q.alphas != NULL || q.n_alphas != 100 || q.n_folds != 5 || q.l1_ratio != 0.5 || o.n_iter != NULL) return 1;\n"
        "    if (pols_elastic_net_cv(NULL, NULL, NULL, &q, NULL, &o) != POLS_ERR_INVALID) return 2;\n"
        '    printf("%d %d\\n", (int)sizeof(pols_enet_cv_params), (int)(sizeof(pols_enet_cv_out) / sizeof(void *)));\n'
        "    return 0;\n}\n")
    exe = tmp_path / "consumer"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{root / 'include'}", str(src), "-o", str(exe),
                    f"-L{_lib.LIB_PATH.parent}", "-lpols_mi355x", f"-Wl,-rpath,{_lib.LIB_PATH.parent}"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(C.sizeof(_lib.EnetCvParams)), "7"], out


def test_k12_kernels_use_no_scratch_and_no_agprs(L):
    import sys
    from pathlib import Path

    from polars_ols_amd import _lib

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "scripts"))
    from check_scratch import LLVM, kernel_scratch

    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("ROCm LLVM tools not present")
    ks = {k: v for k, v in kernel_scratch(_lib.LIB_PATH).items() if "k12_" in k}
    assert len(ks) == 2 + 2 + 1 + 2 + 1, sorted(ks)             # count and fold_gram (2 dtypes each), reduce, path (16 / 32 lanes), pick
    for name, (scratch, vgpr, agpr) in ks.items():
        assert scratch == 0 and agpr == 0 and vgpr > 0, (name, scratch, vgpr, agpr)


def test_engine_rejects_unknown_fields_before_any_device_call():
    from polars_ols_amd.engine import Engine

    eng = Engine.__new__(Engine)                                # no device behind it
    eng._lib = None
    y, cols, offs, _ = gen(2, 10, 10, 2)
    with pytest.raises(ValueError):
        eng.elastic_net_cv(y, cols, offs, want=("coef", "leverage"))
    with pytest.raises(ValueError):
        eng.elastic_net_cv(y, cols, offs, [1.0, -2.0])
