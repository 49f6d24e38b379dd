"""The conditioning ladders (cond_ladder.py) are fit to judge the static solves with: on every rung the oracle -- f64 on the rounded
inputs, the reference's pivoted QR -- agrees with a 50-digit solve to a tenth of the project bound, so whatever a GPU test measures
against the oracle at the bound is the kernels' error and not the reference's.  Also: the generator hits its rungs, and every ladder
has groups on both sides of, and between, the two lines the GPU tests hold ``status`` to.  No device."""
import mpmath
import numpy as np
import pytest

import cond_ladder as CL
from oracle import orc

SHAPES = ((8, 200), (20, 120))
ORACLE_SHARE = 0.1                                    # of the project bound tol + tol |beta|: the issue's condition on the inputs
WORST = {}


# seed 1, but: with it one group of this ladder (rung 10^-11.5) has the oracle at 0.38 of the bound -- a condition on the inputs, so the seed moves
SEEDS = {("factor", "f64", 20, 120): 2}


def _frame(kind, dt, kt, n):
    return CL.ladder(kind, dt, kt, n, seed=SEEDS.get((kind, dt, kt, n), 1))


@pytest.mark.parametrize("kt,n", SHAPES)
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("kind", CL.KINDS)
def test_oracle_agrees_with_a_50_digit_solve_on_every_rung(kind, dt, kt, n):
    """mpmath.qr_solve at 50 digits on the same rounded inputs, every group (three seeds per rung)."""
    fr = _frame(kind, dt, kt, n)
    tol = CL.TOL[dt]
    worst, at = 0.0, None
    with mpmath.workdps(50):
        for g, r in enumerate(fr["target"]):
            X, y = CL.design(fr, g)
            beta = orc.get_coefficients(y, X)
            exact, _ = mpmath.qr_solve(mpmath.matrix(X.tolist()), mpmath.matrix(y.tolist()))
            exact = np.array([float(v) for v in exact])
            u = float(CL.bound_units(beta, exact, tol).max())
            if u > worst:
                worst, at = u, float(r)
    WORST[(kind, dt, kt, n)] = (worst, at)
    top = max(WORST, key=lambda k: WORST[k][0])
    print(f"oracle vs 50 digits, {kind} {dt} kt={kt} n={n}: worst error / bound {worst:.3g} at rung {at:g}"
          f"  [worst of the {len(WORST)} ladders so far: {WORST[top][0]:.3g} at {top}, rung {WORST[top][1]:g}]")
    assert worst <= ORACLE_SHARE, (worst, at)


@pytest.mark.parametrize("kt,n", SHAPES)
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("kind", CL.KINDS)
def test_every_rung_is_hit_and_every_zone_is_populated(kind, dt, kt, n):
    fr = _frame(kind, dt, kt, n)
    ratio = CL.exact_ratios(fr)
    assert len(ratio) == len(CL.rungs(dt)) * CL.SEEDS_PER_RUNG
    off = np.abs(np.log10(ratio / fr["target"]))
    assert off.max() <= 0.5, (float(off.max()), float(fr["target"][off.argmax()]))         # within half a decade of the rung
    keep, between, flag = CL.zones(ratio, dt)
    assert min(keep.sum(), between.sum(), flag.sum()) >= 3, (int(keep.sum()), int(between.sum()), int(flag.sum()))
    # at least two rungs under the threshold the rule had before it was measured (1e-3 / 1e-10)
    assert len(np.unique(fr["target"][ratio < (1e-3 if dt == "f32" else 1e-10)])) >= 2


def test_every_case_of_the_gpu_module_populates_every_zone():
    """the shapes the GPU tests draw, weights, dropped rows and the ridge penalty included: three groups per zone, and no group whose
    factorisation breaks down in exact arithmetic"""
    seen = set()
    for c in CL.cases():
        key = (c["dt"], c["kind"], c["kt"], str(c["rows"]), c["weights"], c["policy"], c["ridge"])
        if key in seen:
            continue
        seen.add(key)
        fr = CL.case_frame(c)
        ratio = CL.exact_ratios(fr, CL.case_alpha(c), c["policy"] != "ignore")
        assert (ratio > 0).all(), CL.case_id(c)
        keep, between, flag = CL.zones(ratio, c["dt"])
        if c["ridge"]:                                # the penalty lifts the bottom rungs: the flag zone may be empty, the others not
            assert min(keep.sum(), between.sum()) >= 3, (CL.case_id(c), int(keep.sum()), int(between.sum()))
        else:
            assert min(keep.sum(), between.sum(), flag.sum()) >= 3, (CL.case_id(c), int(keep.sum()), int(between.sum()), int(flag.sum()))


def test_the_distinct_coefficients_come_back_in_column_order():
    fr = _frame("pair", "f64", 8, 200)
    g = int(np.flatnonzero(fr["target"] == 1.0)[0])
    X, y = CL.design(fr, g)
    assert np.allclose(orc.get_coefficients(y, X), np.linspace(-2, 2, 8), atol=0.05)
