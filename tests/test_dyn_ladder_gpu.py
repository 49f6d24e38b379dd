"""Every route of rolling_least_squares and recursive_least_squares on the conditioning ladders of dyn_ladder.py: sequences whose windows
have an exact Cholesky pivot ratio from 1 down to 1e-6 (levels fitted with an intercept, returns that share a factor), and r = 1 panels
at a common feature scale of 1e-4 / 1e4.  test_dyn_ladder_cpu.py holds what this file rests on: the truths, the rungs, and the oracle's
own error (a tenth of the bound).

Per (case, dtype), one library call:
(a) on the sampled rows, coefficients and predictions within tol + tol |truth| of the per-row TRUTH (1e-6 f64, 1e-4 f32) wherever the
    exact ratio of the row's system is at least 1e-4 / sqrt(10); below, the bound is max(tol, 1e3 cond eps).  The exact ratio alone
    decides which bound applies;
(b) EVERY row that rests on 2 kt observations within twice the bound of its sequence of the ORACLE (kernel and oracle are each within one
    bound of the truth) -- except on the rungs a case lists under ``no_oracle``, where the reference is no truth (RLS from p0 = 1e6 on
    ``level`` data, the 1e-4 rung: those sequences are held to (a) and (c));
(c) the NaN pattern of every row that rests on 2 kt observations (under a ridge penalty: every row) is the oracle's: no rung makes a
    route give up;
(d) ``scaled``, rolling: coefficients equal 1 / s x the s = 1 run's, predictions equal the s = 1 run's, the kernel is the same -- every
    row with kt observations, at the tolerance from 2 kt observations on and at max(tol, 1e3 cond eps) of the row's own window below;
(e) the kernel family is the one the case names, and together the cases reach every route (dyn_ladder.REACH).

OPEN (dyn_ladder.OPEN, DESIGN.md "Dynamic ladder"): two weighted f32 cases miss (a) and (b) on rows with an exact ratio below 1e-4,
because the prologue rounds x sqrt(w) to f32, and K3's P-form from p0 = 1e6 misses (a) in f64 on a ``level`` row at ratio 3.5e-5.  They
are held to (c), (e) and to (a) on the rows from ratio 1e-4 up like every other case; what is left is expected to fail, and the test
fails if it stops failing."""
import numpy as np
import pytest

import cond_ladder as CL
import dyn_ladder as DL

pytestmark = pytest.mark.gpu

SEEN = set()                                           # `reach` of the cases that ran the kernel family they name


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _worst(units, rows=None):
    j = int(np.argmax(units))
    return float(units[j]), int(j if rows is None else rows[j])


def _scaled_twin(eng, case, dt, fr, coef, pred, name):
    """(d): the same panel at scale 1 through the same call"""
    s, tol, kt, kw = case["scale"], DL.TOL[dt], fr["kt"], case["kw"]
    one = DL.ladder(case, dt, scale=1.0)
    coef1, pred1, name1 = DL.run(eng, case, one)
    assert name1 == name, (name1, name)
    assert np.array_equal(np.isnan(coef), np.isnan(coef1)) and np.array_equal(np.isnan(pred), np.isnan(pred1))
    nobs = DL.observations(fr, case)
    tol_rows = np.full(len(nobs), tol)
    for i in np.flatnonzero((nobs >= kt) & (nobs < 2 * kt)):                               # barely determined windows: their own conditioning
        Xw = DL.window_matrix(one["offs"], one["valid"], one["X"], int(i), kw["window_size"], kw["null_policy"])
        with np.errstate(all="ignore"):
            tol_rows[i] = max(tol, 1e3 * np.linalg.cond(Xw.T @ Xw) * DL.EPS)
    m = (nobs >= kt) & np.isfinite(tol_rows)
    uc = (CL.bound_units(coef * s, coef1, 1.0).max(axis=1) / tol_rows)[m]
    up = (CL.bound_units(pred, pred1, 1.0) / tol_rows)[m]
    print(f"    scale {s:g} against scale 1 on {int(m.sum())} rows: coefficients {float(uc.max()):.3g}, predictions {float(up.max()):.3g} of the bound")
    assert uc.max() <= 1.0 and up.max() <= 1.0, (float(uc.max()), float(up.max()))


@pytest.mark.parametrize("case,dt", DL.PARAMS, ids=DL.PARAM_IDS)
def test_every_rung_stays_within_its_bound_of_the_truth_and_of_the_oracle(eng, case, dt):
    p = DL.prepared(case, dt)
    fr, rows, tr = p["fr"], p["rows"], p["truth"]
    coef, pred, name = DL.run(eng, case, fr)
    got = DL.compare(case, dt, coef, pred)
    strict = tr["ratio"] >= DL.STRICT_RATIO
    ut, at = _worst(got["truth_units"], rows)
    uo, ao = _worst(got["oracle_units"])
    j = int(np.argmax(got["truth_units"]))
    print(f"{case['id']}-{dt} [{name}]: vs truth {ut:.3g} of the bound at row {at} (exact ratio {tr['ratio'][j]:.3g}, {int(strict.sum())} of {len(rows)} rows "
          f"at the plain bound); vs oracle {uo:.3g} of twice the bound at row {ao}; NaN pattern differs on {len(got['nan_rows'])} rows")
    assert DL.family(name) == case["family"], (name, case["family"])                     # (e)
    SEEN.add(case["reach"])
    assert len(got["nan_rows"]) == 0, ("NaN pattern", got["nan_rows"][:10])                # (c)
    is_open = (case["id"], dt) in DL.OPEN
    held = tr["ratio"] >= DL.OPEN_RATIO if is_open else np.ones(len(rows), dtype=bool)
    bad = np.flatnonzero(~(got["truth_units"] <= 1.0) & held)                            # (a)
    assert bad.size == 0, ("outside the bound of the truth: (row, exact ratio, error / bound)",
                           [(int(rows[b]), float(tr["ratio"][b]), float(got["truth_units"][b])) for b in bad[:8]])
    if is_open:                                        # the rest of (a), and (b), are expected to fail on these: rows below ratio 1e-4
        rest = ~(got["truth_units"] <= 1.0) & ~held
        if rest.any() or (got["oracle_units"] > 1.0).any():
            pytest.xfail(f"open (dyn_ladder.OPEN): {ut:.3g} of the bound of the truth, {uo:.3g} of twice the bound of the oracle")
        pytest.fail("an OPEN case is inside its bounds: take it out of dyn_ladder.OPEN and DESIGN.md")
    bad = np.flatnonzero(~(got["oracle_units"] <= 1.0))                                  # (b)
    assert bad.size == 0, ("outside twice the bound of the oracle: (row, error / twice the bound)", [(int(b), float(got["oracle_units"][b])) for b in bad[:8]])
    if case["kind"] == "scaled" and case["entry"] == "rolling":                           # (d)
        _scaled_twin(eng, case, dt, fr, coef, pred, name)


def test_the_cases_reach_every_route(eng):
    """one cheap call per case that has not run yet (a deselected one), then: every route the ladder is meant for was reached.  What is
    observed is the kernel FAMILY (last_kernel); which form inside a family a shape takes (packed / own-halo / halo-wave tiles, single
    or cut chunks) follows from the case's shape and options, as in tests/dynamic_routes.py."""
    for c, dt in DL.PARAMS:
        if c["reach"] not in SEEN and DL.family(DL.run(eng, c, DL.ladder(c, dt))[2]) == c["family"]:
            SEEN.add(c["reach"])
    assert DL.REACH <= SEEN, DL.REACH - SEEN
