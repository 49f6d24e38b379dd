"""pols_random_effects (K19) on guarded buffers: nothing outside a column's extent is used, every output is written in full and no
guard is touched, on both routes of the table kernel and for subsets of the outputs; a poisoned group leaves its neighbours' bits
alone; a device output off the 16-byte grid is refused."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from arena import Frame, arena_engine, input_arena  # noqa: E402
from arena_cases import (assert_same_bits, close, every_other, guarded, odd_total, poisoned, static_data, tol_of)  # noqa: E402
from random_effects_ref import COUNTS, GROUP_FIELDS, ROW_FIELDS, re_batch  # noqa: E402

DTYPES = [np.float32, np.float64]
NARROW_SIZES, WIDE_SIZES = odd_total([61, 203, 517, 1001, 333]), odd_total([205, 517, 1001, 333, 411])
WIDTHS = [(6, NARROW_SIZES, 15), (20, WIDE_SIZES, 40)]               # features, sizes, ids per group (C > kc = 7 and 21)
RESIDENT, GLOBAL = "k19_random_effects_resident", "k19_random_effects_global"


@pytest.fixture(scope="module")
def eng():
    e = arena_engine(0)
    yield e
    e.close()


def _all():
    from polars_ols_amd import _lib as L

    return ("coef", "pred", "resid", "status") + L.RANDOM_EFFECTS_FIELDS


def _panel(seed, dtype, k, sizes, n_ids):
    """static_data's frame with a shock per id added to the target"""
    d = static_data(seed, dtype, k, False, "ignore", sizes=sizes)
    rng = np.random.default_rng(seed + 1)
    code = rng.integers(0, n_ids, size=len(d["y"]))
    d["y"] = (d["y"].astype(np.float64) + rng.normal(size=n_ids)[code]).astype(dtype)
    for j in range(k):
        d["cols"][j] = (d["cols"][j].astype(np.float64) + 0.5 * rng.normal(size=n_ids)[code]).astype(dtype)
    return d, (code * 1_000_003 - 7_000_000_000).astype(np.int64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,sizes,n_ids", WIDTHS)
@pytest.mark.parametrize("route", [None, "global"])
def test_guards(eng, dtype, k, sizes, n_ids, route):
    d, ida = _panel(61 + k, dtype, k, sizes, n_ids)
    fr = Frame(d["y"], d["cols"], d["offs"])
    ids = input_arena(ida, -1, device=True)
    call = lambda: eng.random_effects(fr.y, fr.cols, ids.body, fr.offs, add_intercept=True, want=_all())  # noqa: E731
    try:
        eng.set_option("RANDOM_EFFECTS_ROUTE", route)
        fr.guards(np.nan)
        a, name = guarded(eng, f"random_effects k={k} [NaN guards]", call, fresh=True)
        fr.guards(7.0)
        ids.fill_guards(int(ida[0]))                                 # (an id that exists: a read past the end would join its category)
        b, name_b = guarded(eng, f"random_effects k={k} [7.0 guards]", call, fresh=False)
    finally:
        eng.set_option("RANDOM_EFFECTS_ROUTE", None)
    assert name == name_b == (GLOBAL if route else RESIDENT)
    assert_same_bits(a, b, f"random_effects k={k} [{name}]: NaN against 7.0 in the input guards")
    f = lambda v: np.asarray(v, dtype=np.float64)  # noqa: E731
    exp = re_batch(f(d["y"]), [f(c) for c in d["cols"]], d["offs"], ida, True)
    assert (exp["status"] == 0).all() and np.isfinite(exp["se"]).all()
    tol = tol_of(dtype)
    for key in ("coef",) + GROUP_FIELDS + ROW_FIELDS:
        close(a[key], exp[key], tol, f"random_effects k={k} {key}")
    for key in COUNTS:
        assert np.array_equal(a[key], exp[key]), key


@pytest.mark.parametrize("want", [("coef",), ("hausman", "hausman_p", "theta"), ("se", "effects", "n_obs")])
def test_guards_of_output_subsets(eng, want):
    d, ida = _panel(67, np.float32, 6, NARROW_SIZES, 15)
    fr = Frame(d["y"], d["cols"], d["offs"])
    ids = input_arena(ida, -1, device=True)
    fr.guards(np.nan)
    full, _ = guarded(eng, "random_effects [every field]", lambda: eng.random_effects(fr.y, fr.cols, ids.body, fr.offs, add_intercept=True, want=_all()))
    part, _ = guarded(eng, f"random_effects {want}", lambda: eng.random_effects(fr.y, fr.cols, ids.body, fr.offs, add_intercept=True, want=want),
                      fresh=True)
    assert set(part) == set(want)
    assert_same_bits({key: full[key] for key in want}, part, f"random_effects: {want} alone")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["nan", "huge"])
def test_isolation(eng, dtype, kind):
    k = 6
    d, ida = _panel(71, dtype, k, NARROW_SIZES, 15)
    offs = d["offs"]
    fr = Frame(d["y"], d["cols"], offs)
    ids = input_arena(ida, -1, device=True)
    call = lambda: eng.random_effects(fr.y, fr.cols, ids.body, fr.offs, add_intercept=True, want=_all())  # noqa: E731
    first, name = guarded(eng, "random_effects [clean]", call, fresh=True)
    again, _ = guarded(eng, "random_effects [clean, again]", call, fresh=False)
    assert_same_bits(first, again, "random_effects: two runs of the clean frame")
    bad, clean, rows = every_other(offs)
    p = poisoned([d["y"]] + list(d["cols"]), offs, bad, kind)
    fr.load(p[0], p[1:1 + k])
    got, name_p = guarded(eng, f"random_effects [{kind} next door]", call, fresh=False)
    assert name_p == name
    n = len(d["y"])
    sel = {key: (rows if v.shape[0] == n else clean) for key, v in first.items()}
    assert_same_bits(first, got, f"random_effects: {kind} in every other group", rows=sel)
    assert (got["status"][bad] != 0).all() and (got["status"][clean] == 0).all()


def test_unaligned_device_outputs_are_refused(eng):
    import torch
    from polars_ols_amd import _lib as L

    d, ida = _panel(73, np.float64, 3, [101, 203], 9)
    n = len(d["y"])
    t = torch.from_numpy
    y, cols, ids = t(d["y"]).cuda(), [t(c).cuda() for c in d["cols"]], t(ida).cuda()
    room = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
    for key in ("pred", "resid"):
        with pytest.raises(L.PolsError) as ei:
            eng.random_effects(y, cols, ids, d["offs"], want=("coef", key), out={key: room[1:n + 1]})
        assert ei.value.code == -1
    got = eng.random_effects(y, cols, ids, d["offs"], want=("coef", "pred"), out={"pred": room[2:n + 2]})
    eng.synchronize()
    assert torch.isfinite(got["pred"]).all() and float(room[0]) == 0.0 and float(room[1]) == 0.0
