"""The numpy restatement of per-group AR(1) feasible GLS (tests/glsar_ref.py, the yardstick of tests/test_glsar_gpu.py) against the
textbook identities of the estimator, the lag-moment route the device takes, its edge rules, the decidedness of every frame the GPU
tests use, the Python argument checks of the glsar entry and the resources of the K18 code objects.  No GPU here."""
from pathlib import Path

import numpy as np
import pytest

from glsar_ref import (BAD_DOF, EMPTY, FALLBACK, METHODS, NOT_CONVERGED, OK, SHAPES, decided, edge_frame, frame, gen_panel_ar1, glsar_batch,
                       glsar_group, null_frame, rho_of, transform)

ROOT = Path(__file__).resolve().parent.parent


def _one_group(n=300, k=3, seed=3):
    y, cols, offs, phi = gen_panel_ar1(1, n, n, k, np.float64, seed)
    return np.column_stack(cols + [np.ones(n)]), y, float(phi[0])


def _moments(Z):
    """what the device keeps of a group: S, the lag-one cross-moments C, the first and the last row"""
    return Z.T @ Z, Z[1:].T @ Z[:-1], Z[0], Z[-1]


def _a_of_rho(S, Cm, z1, zn, rho, method):
    A = (S - np.outer(z1, z1)) - rho * (Cm + Cm.T) + rho * rho * (S - np.outer(zn, zn))
    if method == "prais_winsten":
        A = A + (1.0 - rho * rho) * np.outer(z1, z1)
    return A


def _rho_from_moments(S, Cm, zn, b):
    v = np.append(-b, 1.0)
    return (v @ Cm @ v) / (v @ (S - np.outer(zn, zn)) @ v)


@pytest.mark.parametrize("rho", [-0.7, 0.0, 0.35, 0.9])
def test_prais_winsten_at_a_fixed_rho_is_dense_gls(rho):
    X, y, _ = _one_group(n=120)
    n = len(y)
    idx = np.arange(n)
    omega = rho ** np.abs(idx[:, None] - idx[None, :]) / (1.0 - rho * rho)
    Oi = np.linalg.inv(omega)
    b_gls = np.linalg.solve(X.T @ Oi @ X, X.T @ Oi @ y)
    Zs = transform(np.column_stack([X, y]), rho, "prais_winsten")
    b = np.linalg.lstsq(Zs[:, :-1], Zs[:, -1], rcond=None)[0]
    print("max |b - dense GLS|", np.abs(b - b_gls).max())
    np.testing.assert_allclose(b, b_gls, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(Zs[:, :-1].T @ Zs[:, :-1], X.T @ Oi @ X, rtol=1e-10, atol=1e-10)   # P'P = Omega^-1


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_moment_form_equals_the_row_form_on_every_test_frame(shape):
    y, cols, offs, _ = frame(shape, np.float64)
    X = np.column_stack(cols + [np.ones(len(y))])
    worst_a = worst_r = 0.0
    for g in range(len(offs) - 1):
        Z = np.column_stack([X, y])[offs[g]:offs[g + 1]]
        if len(Z) <= X.shape[1] + 1:
            continue
        S, Cm, z1, zn = _moments(Z)
        scale = np.sqrt(np.outer(np.diagonal(S), np.diagonal(S)))
        for method in METHODS:
            for rho in (0.0, -0.6, 0.45, 0.93):
                Zs = transform(Z, rho, method)
                worst_a = max(worst_a, (np.abs(_a_of_rho(S, Cm, z1, zn, rho, method) - Zs.T @ Zs) / scale).max())
                b = np.linalg.lstsq(Zs[:, :-1], Zs[:, -1], rcond=None)[0]
                num, den = rho_of(Z[:, -1] - Z[:, :-1] @ b)
                worst_r = max(worst_r, abs(_rho_from_moments(S, Cm, zn, b) - num / den))
    print(f"{shape}: A(rho) moments against rows {worst_a:.3e} (relative to sqrt(S_ii S_jj)), rho update {worst_r:.3e}")
    assert worst_a < 1e-10 and worst_r < 1e-10


@pytest.mark.parametrize("method", METHODS)
def test_max_iter_one_is_the_two_step_estimator(method):
    X, y, _ = _one_group()
    res = glsar_group(X, y, method, max_iter=1)
    assert res["status"] == NOT_CONVERGED and res["n_iter"] == 1
    Z0 = transform(np.column_stack([X, y]), 0.0, method)             # rho = 0: OLS (Cochrane-Orcutt: of the rows t >= 2, its n* rows)
    b0 = np.linalg.solve(Z0[:, :-1].T @ Z0[:, :-1], Z0[:, :-1].T @ Z0[:, -1])
    if method == "prais_winsten":
        np.testing.assert_allclose(b0, np.linalg.solve(X.T @ X, X.T @ y), rtol=1e-12)
    e = y - X @ b0
    rho = (e[1:] @ e[:-1]) / (e[:-1] @ e[:-1])
    Zs = transform(np.column_stack([X, y]), rho, method)
    b1 = np.linalg.solve(Zs[:, :-1].T @ Zs[:, :-1], Zs[:, :-1].T @ Zs[:, -1])
    np.testing.assert_allclose(res["rho"], rho, rtol=1e-12)
    np.testing.assert_allclose(res["coef"], b1, rtol=1e-9, atol=1e-12)
    u = Zs[:, -1] - Zs[:, :-1] @ b1
    df = len(u) - X.shape[1]
    np.testing.assert_allclose(res["sigma2"], u @ u / df, rtol=1e-9)
    np.testing.assert_allclose(res["se"], np.sqrt(u @ u / df * np.diagonal(np.linalg.inv(Zs[:, :-1].T @ Zs[:, :-1]))), rtol=1e-9)
    np.testing.assert_allclose(res["dw_ols"], (np.diff(e) @ np.diff(e)) / (e @ e), rtol=1e-12)
    np.testing.assert_allclose(res["dw"], (np.diff(u) @ np.diff(u)) / (u @ u), rtol=1e-9)


def test_rho_follows_the_generating_phi_and_dw_moves_towards_two():
    y, cols, offs, phi = frame("segmented", np.float64)
    ref = glsar_batch(y, cols, offs, "prais_winsten", add_intercept=True)
    assert (ref["status"] == OK).all()
    r = np.corrcoef(ref["rho"], phi)[0, 1]
    print("corr(rho*, phi)", r, "max |rho* - phi|", np.abs(ref["rho"] - phi).max())
    assert r > 0.99 and np.abs(ref["rho"] - phi).max() < 0.1
    np.testing.assert_allclose(ref["dw_ols"], 2.0 * (1.0 - ref["rho"]), atol=0.05)
    assert np.abs(ref["dw"] - 2.0).max() < 0.2


def _assert_decided(ref, what):
    d = decided(ref)
    soft = ~ref["hard"]
    print(f"{what}: status counts {np.bincount(ref['status'], minlength=5).tolist()}, smallest ratio {ref['ratio'][soft].min():.2e}, "
          f"largest |rho| {ref['rho_max'][soft].max():.4f}, smallest tol margin {ref['tol_margin'][soft].min():.2e}, most updates {ref['n_iter'].max()}")
    assert d.all(), (what, np.flatnonzero(~d))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_group_of_every_gpu_frame_is_decided(shape, dtype, method):
    y, cols, offs, _ = frame(shape, dtype)
    _assert_decided(glsar_batch(y, cols, offs, method, add_intercept=True), f"{shape} {np.dtype(dtype).name} {method}")


@pytest.mark.parametrize("method", METHODS)
def test_the_other_gpu_frames_are_decided_too(method):
    for dtype in (np.float64, np.float32):
        y, cols, offs = edge_frame(dtype)
        _assert_decided(glsar_batch(y, cols, offs, method, add_intercept=True), f"edges {np.dtype(dtype).name} {method}")
    y, cols, offs, _ = frame("short_k2", np.float64)
    for max_iter in (1, 2):
        _assert_decided(glsar_batch(y, cols, offs, method, max_iter=max_iter, add_intercept=True), f"short_k2 max_iter={max_iter} {method}")
    y, cols, offs = null_frame()
    for policy in ("ignore", "zero"):
        _assert_decided(glsar_batch(y, cols, offs, method, add_intercept=True, null_policy=policy), f"nulls {policy} {method}")


@pytest.mark.parametrize("method", METHODS)
def test_status_of_the_edge_groups(method):
    y, cols, offs = edge_frame(np.float64)
    ref = glsar_batch(y, cols, offs, method, add_intercept=True)
    pw = method == "prais_winsten"
    st = list(ref["status"])
    assert st[:4] == [OK, EMPTY, BAD_DOF, OK] and st[5:] == [FALLBACK, FALLBACK, OK, OK, OK]
    assert st[4] in (OK, NOT_CONVERGED) if pw else st[4] == BAD_DOF
    assert (ref["coef"][1] == 0).all() and ref["n_iter"][1] == 0 and np.isnan(ref["rho"][1])
    assert ref["rho_max"][6] >= 1.0 and ref["n_iter"][6] >= 1           # the explosive series: an update reached |rho| >= 1
    assert ref["ratio"][5] < 1e-14                                      # the duplicated column: no pivot
    for g in (2, 5, 6):
        assert np.isnan(ref["coef"][g]).all() and np.isnan(ref["se"][g]).all() and np.isnan(ref["dw"][g])
    np.testing.assert_array_equal(ref["n_obs"], np.diff(offs))
    y, cols, offs = null_frame()
    assert list(glsar_batch(y, cols, offs, method, add_intercept=True)["status"]) == [OK, FALLBACK, OK, FALLBACK, OK, FALLBACK, FALLBACK, OK]
    assert (glsar_batch(y, cols, offs, method, add_intercept=True, null_policy="zero")["status"] == OK).all()


def test_argument_checks_need_no_device():
    from polars_ols_amd import _lib as L
    from polars_ols_amd.engine import _glsar_params
    from polars_ols_amd.least_squares import compute_glsar

    q = _glsar_params(None, "cochrane_orcutt", 7, 1e-4)
    assert (q.method, q.max_iter, q.tol) == (0, 7, 1e-4)
    assert L.GLSAR_METHODS == {"cochrane_orcutt": 0, "prais_winsten": 1} and "pols_glsar" in L.EXPORTS
    for bad in (dict(method="yule_walker"), dict(max_iter=0), dict(max_iter=2.5), dict(max_iter=True), dict(tol=0.0), dict(tol=float("nan")),
                dict(tol=float("inf")), dict(mode="glsar"), dict(null_policy="drop")):
        with pytest.raises(ValueError):
            compute_glsar("y", "x", **bad)


def test_the_lag_gram_kernel_keeps_its_arrays_in_registers():
    """The code objects' own metadata (no GPU, no recompilation): the hot launch of pols_glsar holds nothing in scratch memory."""
    import sys

    from polars_ols_amd import _lib

    sys.path.insert(0, str(ROOT / "scripts"))
    from check_scratch import LLVM, kernel_scratch

    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("ROCm LLVM tools not present")
    if not _lib.LIB_PATH.exists():
        _lib.build()
    ks = {k: v for k, v in kernel_scratch(_lib.LIB_PATH).items() if "pols::k18_lag_gram_kernel<" in k}
    print(ks)
    assert len(ks) == 2, sorted(ks)                                  # float and double
    assert all(v[0] == 0 for v in ks.values()), ks
