"""The static dispatcher without a device: pols_debug_static_route (offsets scan -> solve plan -> route picker) must name, for every
recorded shape of tests/static_routes.json, the family of the kernel string the library launched for it before the dispatcher was
split; and the plan resolver must answer every rejected (alpha, l1_ratio, positive, solve_method) combination with the code and the
message the monolithic dispatcher gave."""
import ctypes as C

import pytest

import static_routes as SR
from polars_ols_amd import _lib as L

CASES = SR.load()
SECTIONS = sorted({c["section"] for c in CASES})


def _params(lib, case):
    kw = case.get("params", {})
    p = L.OlsParams()
    lib.pols_ols_params_default(C.byref(p))
    p.alpha = float(kw.get("alpha", 0.0))
    p.has_l1_ratio = int(kw.get("l1_ratio") is not None)
    p.l1_ratio = float(kw.get("l1_ratio") or 0.0)
    p.positive = int(bool(kw.get("positive", False)))
    p.solve_method = L.SOLVE_METHODS[kw.get("solve_method")]
    p.has_rcond = int(kw.get("rcond") is not None)
    p.rcond = float(kw.get("rcond") or 0.0)
    p.null_policy = kw.get("null_policy_code", L.NULL_POLICIES[case.get("policy", "ignore")])
    return p


def _route(case, offs=None):
    """-> (return code, route or error message)"""
    lib = L.lib()
    if offs is None:
        offs = SR.frame(case)[2]
    b = L.Batch(dtype=L.POLS_F32 if case["dtype"] == "f32" else L.POLS_F64, mem=L.POLS_MEM_HOST, n_rows=int(offs[-1]), n_groups=len(offs) - 1,
                group_offsets=offs.ctypes.data_as(C.POINTER(C.c_int64)), n_features=case["kt"],
                weights=1 if case.get("weights") else None, valid=1 if case.get("valid") else None)   # (only tested for NULL: no column is read)
    p = _params(lib, case)
    opts = case.get("options", {})
    keys = (C.c_char_p * len(opts))(*[k.encode() for k in opts])
    vals = (C.c_char_p * len(opts))(*[v.encode() for v in opts.values()])
    buf = C.create_string_buffer(64)
    rc = lib.pols_debug_static_route(C.byref(b), C.byref(p), keys, vals, len(opts), buf, len(buf))
    return rc, (buf.value.decode() if rc == 0 else lib.pols_last_error().decode())


@pytest.mark.parametrize("section", SECTIONS)
def test_picker_names_the_family_of_every_recorded_route(section):
    cases = [c for c in CASES if c["section"] == section]
    assert cases
    wrong = []
    for c, _y, _cols, offs, _w in SR.frames(cases):
        rc, route = _route(c, offs)
        if rc != 0 or route != SR.family(c["name"]):
            wrong.append((c["id"], rc, route, c["name"]))
    assert not wrong, wrong[:10]


def test_recorded_grid_reaches_every_route():
    assert {SR.family(c["name"]) for c in CASES} == {"wide", "svd_all", "k2", "k2w", "streamed", "classes_streamed_top", "classes", "k1"}


RIDGE = "Only 'Cholesky', 'LU', & 'SVD' are currently supported solver methods for Ridge."
CD = "Only solve_method 'CD' (coordinate descent) is currently supported for Elastic Net / Lasso problems."
ALPHA = "'alpha' must be strictly positive"
L1 = "'l1_ratio' must be strictly between 0. and 1."
# (alpha, l1_ratio, positive, solve_method) -> message; every one is POLS_ERR_PANIC
REJECTED = [
    (1.0, None, False, "qr", RIDGE), (1.0, None, False, "cd", RIDGE), (1.0, None, False, "cd_active_set", RIDGE),
    (0.0, None, False, "cd", RIDGE), (0.0, None, False, "cd_active_set", RIDGE), (1.0, 0.0, False, "qr", RIDGE),
    (0.1, 0.5, False, "qr", CD), (0.1, 0.5, False, "svd", CD), (0.1, 0.5, False, "chol", CD), (0.1, 0.5, False, "lu", CD),
    (1.0, None, True, "svd", CD), (0.0, None, True, "chol", CD), (-1.0, None, False, "chol", CD), (-1.0, None, False, "qr", CD),
    (0.0, None, True, None, ALPHA), (0.0, 0.5, False, "cd", ALPHA), (-1.0, None, False, None, ALPHA),
    (-1.0, 0.5, True, "cd_active_set", ALPHA), (float("nan"), None, False, None, ALPHA),
    (0.1, 1.5, False, None, L1), (0.1, -0.5, False, "cd", L1), (0.1, float("nan"), True, None, L1),
]
ACCEPTED = [(0.0, None, False, m) for m in (None, "qr", "svd", "chol", "lu")] + [(1.0, None, False, m) for m in (None, "svd", "chol", "lu")] + \
           [(0.1, 0.5, False, m) for m in (None, "cd", "cd_active_set")] + [(0.1, None, True, None), (0.1, 1.0, False, None), (0.1, 0.0, True, "cd"), (0.0, 0.5, False, None)]   # (the last: alpha == 0 with no method is the OLS branch whatever l1_ratio says)


@pytest.mark.parametrize("kt", [4, 40])
def test_resolver_rejects_what_the_dispatcher_rejected(kt):
    shape = {"dtype": "f64", "kt": kt, "groups": 3, "rows": 100, "seed": 1}
    for alpha, l1, positive, method, msg in REJECTED:
        rc, got = _route(dict(shape, params={"alpha": alpha, "l1_ratio": l1, "positive": positive, "solve_method": method}))
        assert (rc, got) == (-4, msg), (alpha, l1, positive, method, rc, got)
    for alpha, l1, positive, method in ACCEPTED:
        rc, got = _route(dict(shape, params={"alpha": alpha, "l1_ratio": l1, "positive": positive, "solve_method": method}))
        assert rc == 0, (alpha, l1, positive, method, rc, got)


def test_null_policy_checks_come_first():
    shape = {"dtype": "f32", "kt": 4, "groups": 3, "rows": 100, "seed": 1}
    assert _route(dict(shape, params={"null_policy_code": 9})) == (-1, "unknown null_policy 9")
    assert _route(dict(shape, params={"null_policy_code": 9, "alpha": 1.0, "solve_method": "qr"})) == (-1, "unknown null_policy 9")
    assert _route(dict(shape, valid=True, policy="ignore")) == (-1, "a validity mask needs a drop-family null_policy")
    assert _route(dict(shape, valid=True, policy="zero")) == (-1, "a validity mask needs a drop-family null_policy")
    assert _route(dict(shape, valid=True, policy="drop"))[0] == 0


def test_unknown_option_and_descending_offsets_are_errors():
    shape = {"dtype": "f32", "kt": 4, "groups": 3, "rows": 100, "seed": 1}
    rc, msg = _route(dict(shape, options={"NO_SUCH_KNOB": "1"}))
    assert rc == -1 and "NO_SUCH_KNOB" in msg
    lib = L.lib()
    offs = (C.c_int64 * 3)(0, 10, 5)
    b = L.Batch(dtype=L.POLS_F32, mem=L.POLS_MEM_HOST, n_rows=5, n_groups=2, group_offsets=offs, n_features=2)
    p = L.OlsParams()
    lib.pols_ols_params_default(C.byref(p))
    buf = C.create_string_buffer(32)
    assert lib.pols_debug_static_route(C.byref(b), C.byref(p), None, None, 0, buf, 32) == -1
    assert lib.pols_last_error().decode() == "group_offsets must be ascending"
