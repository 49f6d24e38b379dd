"""pols_least_squares_absorb (K16) on guarded buffers: nothing outside a column's extent is used, every output is written in full
and no guard is touched; a poisoned group leaves its neighbours' bits alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from absorb_ref import within_batch  # noqa: E402
from arena import Frame, arena_engine, input_arena  # noqa: E402
from arena_cases import (assert_same_bits, close, every_other, guarded, odd_total, poisoned, static_data, tol_of)  # noqa: E402

DTYPES = [np.float32, np.float64]
NARROW_SIZES, WIDE_SIZES = odd_total([61, 203, 517, 1001, 333]), odd_total([205, 517, 1001, 333, 411])
WIDTHS = [(6, NARROW_SIZES), (20, WIDE_SIZES)]                      # features; with the intercept 7 and 21 coefficients


@pytest.fixture(scope="module")
def eng():
    e = arena_engine(0)
    yield e
    e.close()


def _all():
    from polars_ols_amd import _lib as L

    return ("coef", "pred", "resid", "status") + L.ABSORB_FIELDS


def _ids(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 15, size=n) * 1_000_003 - 7_000_000_000).astype(np.int64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,sizes", WIDTHS)
@pytest.mark.parametrize("cov_type", ["nonrobust", "cluster"])
def test_guards(eng, dtype, k, sizes, cov_type):
    d = static_data(61 + k, dtype, k, True, "ignore", sizes=sizes)
    ida = _ids(len(d["y"]), 9)
    fr = Frame(d["y"], d["cols"], d["offs"], w=d["w"])
    ids = input_arena(ida, -1, device=True)
    call = lambda: eng.absorb(fr.y, fr.cols, ids.body, fr.offs, cov_type=cov_type, weights=fr.w, add_intercept=True, want=_all())  # noqa: E731
    fr.guards(np.nan)
    a, name = guarded(eng, f"absorb k={k} [NaN guards]", call, fresh=True)
    fr.guards(7.0)
    ids.fill_guards(int(ida[0]))                                     # (an id that exists: a read past the end would join its category)
    b, name_b = guarded(eng, f"absorb k={k} [7.0 guards]", call, fresh=False)
    assert name == name_b == "k16_absorb_ordered"
    assert_same_bits(a, b, f"absorb k={k} [{name}]: NaN against 7.0 in the input guards")
    f = lambda v: np.asarray(v, dtype=np.float64)  # noqa: E731
    exp = within_batch(f(d["y"]), [f(c) for c in d["cols"]], d["offs"], ida, f(d["w"]), True, cov_type)
    tol = tol_of(dtype)
    for key in ("coef", "pred", "resid", "fe", "se", "t_values", "p_values", "sigma2", "r2_within", "r2"):
        close(a[key], exp[key], tol, f"absorb k={k} {key}")
    for key in ("status", "n_obs", "n_categories"):
        assert np.array_equal(a[key], exp[key]), key


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["nan", "huge"])
def test_isolation(eng, dtype, kind):
    k = 6
    d = static_data(71, dtype, k, True, "ignore", sizes=NARROW_SIZES)
    offs = d["offs"]
    ida = _ids(len(d["y"]), 10)
    fr = Frame(d["y"], d["cols"], offs, w=d["w"])
    ids = input_arena(ida, -1, device=True)
    call = lambda: eng.absorb(fr.y, fr.cols, ids.body, fr.offs, cov_type="cluster", weights=fr.w, add_intercept=True, want=_all())  # noqa: E731
    first, name = guarded(eng, "absorb [clean]", call, fresh=True)
    again, _ = guarded(eng, "absorb [clean, again]", call, fresh=False)
    assert_same_bits(first, again, "absorb: two runs of the clean frame")
    bad, clean, rows = every_other(offs)
    p = poisoned([d["y"]] + list(d["cols"]) + [d["w"]], offs, bad, kind)
    fr.load(p[0], p[1:1 + k], p[1 + k])
    got, name_p = guarded(eng, f"absorb [{kind} next door]", call, fresh=False)
    assert name_p == name
    n = len(d["y"])
    sel = {key: (rows if v.shape[0] == n else clean) for key, v in first.items()}
    assert_same_bits(first, got, f"absorb: {kind} in every other group", rows=sel)
    assert (got["status"][bad] != 0).all() and (got["status"][clean] == 0).all()
