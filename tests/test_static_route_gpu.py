"""The routes of the static dispatcher, held to a recording: every shape of tests/static_routes.json must launch exactly the kernel
string recorded for it before the dispatcher was split (plan resolver, route picker, one function per route).  The shapes
test_routing_gpu.py samples are also checked against the oracle at that file's tolerances -- the route must still be right."""
import numpy as np
import pytest

import static_routes as SR

pytestmark = pytest.mark.gpu

CASES = SR.load()


def _chunks():
    """one parametrised case per (section, rows / ragged of the grids, option)"""
    out = {}
    for c in CASES:
        key = [c["section"]]
        if c["section"] in ("grid", "options"):
            key += [f"{c['rows']}{'r' if c['ragged'] else 'a'}"] + [f"{k}={v}" for k, v in c.get("options", {}).items()]
        out.setdefault("-".join(key), []).append(c)
    return out


CHUNKS = _chunks()


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("chunk", sorted(CHUNKS))
def test_every_recorded_shape_takes_its_recorded_kernel(eng, chunk):
    from test_nulls_gpu import _expected

    wrong = []
    for c, y, cols, offs, w in SR.frames(CHUNKS[chunk]):
        opts = c.get("options", {})
        try:
            for k, v in opts.items():
                eng.set_option(k, v)
            out = eng.least_squares(y, cols, offs, weights=w, want=("coef", "pred"), **SR.solver_kwargs(c))
            name = eng.last_kernel
        finally:
            for k in opts:
                eng.set_option(k, None)
        if name != c["name"]:
            wrong.append((c["id"], name, c["name"]))
        if c["section"] == "grid" and (c["kt"], c["weights"]) in ((8, 0), (17, 1), (31, 0)):   # the shapes test_routing_gpu.py samples
            coef, pred, _ = _expected(y, cols, offs, w, False, c["policy"])
            tol = 1e-4 if c["dtype"] == "f32" else 1e-6
            assert np.allclose(out["coef"], coef, rtol=tol, atol=tol), (c["id"], name)
            assert np.allclose(out["pred"], pred, rtol=tol, atol=tol, equal_nan=True), (c["id"], name)
    assert not wrong, wrong[:10]


def test_rejected_solver_is_rejected_at_every_width(eng):
    """solve_method="qr" with alpha > 0 is no ridge solver (ls.rs:366): statistics mode answers alike below and above the wide path's 32 columns"""
    from polars_ols_amd._lib import PolsPanic

    codes = []
    for kt in (31, 32):
        y, cols, offs, _ = SR.frame({"dtype": "f64", "kt": kt, "groups": 3, "rows": 100, "seed": 7})
        with pytest.raises(PolsPanic) as e:
            eng.least_squares_statistics(y, cols, offs, solve_method="qr", alpha=1.0)
        assert "supported solver methods for Ridge" in str(e.value)
        codes.append(e.value.code)
    assert codes == [-4, -4]
