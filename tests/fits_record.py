"""The recorded results of the per-group fit entries (ridge_cv, rlm, elastic_net_cv, glm, iv2sls, absorb, absorb2, glsar) and the frames
they were recorded on.

CASES describes every case -- entry, columns, group sizes, the null pattern and policy, the entry's parameters, library options, host or
device batch, the fields wanted -- and frame() rebuilds its frame from a seed derived from the case id.  tests/fits_record.json holds, per
case and dtype, what the library produced on the commit named in the file -- the parent of the latest change that has to leave the
entries' outputs bit for bit as they were (last: the one-wave solve / resid / finish kernels put on csrc/fit_group.inl; every case that was
in the file before came out with the digests it had) --: the ``last_kernel`` string, a sha256 of the input frame and a sha256 of the raw bytes
of every returned array (the first 16 hex digits of each, one line per case: the file stays as long as the case list) -- or, for the calls the library refuses, the exception type, the error code and the message.  It is a measurement
of that parent, never of the code under test: scripts/record_fits.py wrote it, test_fits_record_gpu.py holds the library to it.

The Python front end refuses most bad arguments before the C entry sees them, so a rejection case reaches the entry's own checks by
``poke``: the structs the front end built are changed between the front end and the C call (run(), _Poked)."""
import json
import zlib
from pathlib import Path

import numpy as np

import statistics_record as SR
from statistics_record import BASE, DRIFTED, DTYPES, SEG, SEG_OPT  # noqa: F401  (shared with the statistics recording)

PATH = Path(__file__).resolve().parent / "fits_record.json"
ENTRIES = ("ridge_cv", "rlm", "elastic_net_cv", "glm", "iv2sls", "absorb", "absorb2", "glsar")
COMMON = ("coef", "pred", "resid", "status")
FN = {"ridge_cv": "pols_ridge_cv", "rlm": "pols_rlm", "elastic_net_cv": "pols_elastic_net_cv", "glm": "pols_glm", "iv2sls": "pols_iv2sls",
      "absorb": "pols_least_squares_absorb", "absorb2": "pols_least_squares_absorb2", "glsar": "pols_glsar"}
RIDGE_GRID = [0.0, 0.1, 1.0, 10.0]
ENET_GRID = [0.5, 0.05, 0.5, 0.2, 0.01]          # a repeated value: the visiting order is descending and stable
ENET_KW = {"n_folds": 3, "max_iter": 200}
# rlm at k = 4 keeps 13 tiles (3 328 rows) of a group resident: 4 000 rows are streamed, the others stay
RLM_BOTH = [300, 4000, 0, 3000]
# absorb2 keeps a group of up to 7 435 weighted / 11 684 unweighted rows resident
ABSORB2_MIXED = [7600, 60, 0, 200]
# the groups that end in the failure branches: three rows at k = 4 (no degrees of freedom), none, one, and two ordinary groups -- the
# first of which has its second feature overwritten with a copy of its first (`edge`: a Cholesky pivot fails)
EDGE = [60, 3, 0, 1, 40]
EDGE_SEG = [1500, 3, 0, 700]
SEGMENTED = ("ridge_cv", "elastic_net_cv", "iv2sls", "absorb", "absorb2", "glsar")


def _case(id, entry, k=4, sizes=BASE, **more):
    """kw: the entry's parameters; opts: library options; host / weights / icpt; nulls + policy; want: "all" or the fields; ids:
    "sorted" (inside every group) or "shuffled"; offset (glm); edge: group 0's second feature becomes a copy of its first; poke: [(struct, field, value)] applied between the front end and the C
    entry; reject: the library is expected to refuse the call"""
    assert entry in ENTRIES, entry
    return dict(id=id, entry=entry, k=k, sizes=sizes, **more)


def _both(id, entry, **more):
    return [_case(f"{id}-dev", entry, **more), _case(f"{id}-host", entry, host=True, **more)]


def _kw(entry):
    return {"ridge_cv": {"alphas": RIDGE_GRID}, "elastic_net_cv": dict(ENET_KW, alphas=ENET_GRID), "iv2sls": {"n_endog": 1}}.get(entry, {})


OWN = {"ridge_cv": ("alpha", "alpha_index", "score", "cv_scores", "coef_path"), "rlm": ("scale", "n_iter", "weights"),
       "elastic_net_cv": ("alpha", "alpha_index", "score", "cv_scores", "alphas_used", "coef_path", "n_iter"),
       "glm": ("deviance", "se", "n_iter", "linpred"),
       "iv2sls": ("se", "t_values", "p_values", "cov", "sigma2", "first_stage_f", "partial_r2", "sargan", "sargan_p", "n_obs"),
       "absorb": ("se", "t_values", "p_values", "sigma2", "r2_within", "r2", "fe", "n_obs", "n_categories"),
       "absorb2": ("se", "t_values", "p_values", "sigma2", "r2_within", "r2", "fe1", "fe2", "n_obs", "n_categories", "n_categories2",
                   "n_components", "n_iter"),
       "glsar": ("se", "t_values", "p_values", "cov", "sigma2", "rho", "dw", "dw_ols", "n_iter", "n_obs")}

CASES = []
for _e in ENTRIES:
    # 1. every field wanted, then each of the entry's own alone; device and host
    CASES += _both(f"{_e}-all", _e, kw=_kw(_e))
    for _f in OWN[_e]:
        CASES += _both(f"{_e}-only-{_f}", _e, kw=_kw(_e), want=(_f,))
    # 2. weights + intercept; 10 % of the rows hold a NaN under "drop".  glsar refuses both: the intercept alone, the NaNs under "zero"
    if _e == "glsar":
        CASES += _both("glsar-icpt", _e, icpt=True)
        CASES += _both("glsar-zero", _e, nulls=0.1, policy="zero")
    else:
        CASES += _both(f"{_e}-wi", _e, kw=_kw(_e), weights=True, icpt=True)
        CASES += _both(f"{_e}-drop", _e, kw=_kw(_e), nulls=0.1, policy="drop")
    CASES += [_case(f"{_e}-empty-host", _e, kw=_kw(_e), sizes=[], host=True)]          # n_groups == 0: nothing runs, nothing is refused
# 3. long groups cut into segments
for _e in SEGMENTED:
    CASES += _both(f"{_e}-seg", _e, kw=_kw(_e), k=3, sizes=SEG, opts=SEG_OPT)
CASES += _both("glm-seg", "glm", k=3, sizes=SEG, opts=SEG_OPT)                         # (stays resident: the segments are not asked for)
CASES += _both("glm-seg-split", "glm", k=3, sizes=SEG, opts=dict(SEG_OPT, GLM_ENGINE="split"))
# 4. the entries' own branches
CASES += _both("elastic_net_cv-drop_y_zero_x", "elastic_net_cv", kw=_kw("elastic_net_cv"), nulls=0.1, policy="drop_y_zero_x")   # counted
CASES += _both("elastic_net_cv-auto", "elastic_net_cv", kw=dict(ENET_KW, n_alphas=6))
CASES += _both("rlm-stream", "rlm", opts={"RLM_ENGINE": "stream"})
CASES += _both("rlm-both", "rlm", sizes=RLM_BOTH)
CASES += [_case("rlm-bisquare-dev", "rlm", kw={"norm": "bisquare"})]
CASES += _both("glm-offset", "glm", offset=True)
CASES += _both("glm-split", "glm", opts={"GLM_ENGINE": "split"})
CASES += _both("glm-classes", "glm", sizes="glm_classes", want=("coef", "status", "deviance", "n_iter"))
CASES += [_case("glm-poisson-dev", "glm", kw={"family": "poisson"})]
CASES += _both("iv2sls-HC1", "iv2sls", kw={"n_endog": 1, "cov_type": "HC1"})
CASES += _both("iv2sls-no_rows", "iv2sls", kw={"n_endog": 1}, want=("coef", "status", "first_stage_f", "partial_r2", "n_obs"))
CASES += _both("absorb-sorted", "absorb", ids="sorted")
CASES += _both("absorb-cluster", "absorb", kw={"cov_type": "cluster"})
CASES += _both("absorb-no_resid", "absorb", want=("coef", "status", "fe", "n_obs", "n_categories"))
CASES += _both("absorb2-global", "absorb2", opts={"ABSORB2_ROUTE": "global"})
CASES += _both("absorb2-mixed", "absorb2", sizes=ABSORB2_MIXED, weights=True)
CASES += _both("absorb2-mixed_frame_unweighted", "absorb2", sizes=ABSORB2_MIXED)
CASES += _both("absorb2-cluster", "absorb2", kw={"cov_type": "cluster"})
CASES += [_case("absorb2-no_resid-dev", "absorb2", want=("coef", "status", "fe1", "fe2", "n_iter"))]
CASES += _both("glsar-cochrane_orcutt", "glsar", kw={"method": "cochrane_orcutt"})
CASES += _both("glsar-two_step", "glsar", kw={"max_iter": 1})
# 4b. the groups without a fit: every field wanted
for _e in ENTRIES:
    CASES += _both(f"{_e}-edge", _e, kw=_kw(_e), sizes=EDGE, edge=True)
for _e in SEGMENTED:
    CASES += _both(f"{_e}-edge-seg", _e, kw=_kw(_e), sizes=EDGE_SEG, edge=True, opts=SEG_OPT)
# 5. rejections: (exception type, code, message).  MISALIGN: a one-element offset view of a larger device tensor
NAN, INF, MISALIGN, TWO31 = float("nan"), float("inf"), "misalign", 1 << 31


def _rej(id, entry, poke=(), **more):
    more.setdefault("kw", _kw(entry))
    return _case(f"reject-{entry}-{id}", entry, poke=list(poke), reject=True, **more)


for _e in ("absorb", "absorb2"):
    CASES += [_rej("alpha", _e, [("p", "alpha", 1.0)]), _rej("positive", _e, [("p", "positive", 1)]),
              _rej("l1_ratio", _e, [("p", "has_l1_ratio", 1), ("p", "l1_ratio", 0.5)]),
              _rej("no_feature", _e, [("b", "n_features", 0)]),
              _rej("ids_null", _e, [("q", "ids", None)]),
              _rej("cov_type", _e, [("q", "cov_type", 2)]),
              _rej("rows_2p31", _e, [("b", "n_rows", TWO31)]), _rej("rows_2p31-host", _e, [("b", "n_rows", TWO31)], host=True),
              _rej("mask_ignore", _e, mask=True, nulls=0.1),
              _rej("null_policy", _e, [("p", "null_policy", 99)]),
              _rej("pred_misaligned", _e, [("o", "pred", MISALIGN)]), _rej("resid_misaligned", _e, [("o", "resid", MISALIGN)])]
CASES += [_rej("fe_misaligned", "absorb", [("ro", "fe", MISALIGN)]),
          _rej("ids2_null", "absorb2", [("q", "ids2", None)]),
          _rej("max_iter", "absorb2", [("q", "max_iter", 0)]),
          _rej("tol_zero", "absorb2", [("q", "tol", 0.0)]), _rej("tol_nan", "absorb2", [("q", "tol", NAN)]),
          _rej("tol_inf", "absorb2", [("q", "tol", INF)]),
          _rej("fe1_misaligned", "absorb2", [("ro", "fe1", MISALIGN)]), _rej("fe2_misaligned", "absorb2", [("ro", "fe2", MISALIGN)])]
CASES += [_rej("grid_empty", "ridge_cv", [("q", "n_alphas", 0)]),
          _rej("grid_65", "ridge_cv", kw={"alphas": [0.1] * 65}),
          _rej("grid_negative", "ridge_cv", [("q", "alphas[0]", -1.0)]),
          _rej("positive", "ridge_cv", [("p", "positive", 1)]),
          _rej("alpha", "rlm", [("p", "alpha", 1.0)]), _rej("norm", "rlm", [("q", "norm", 9)]), _rej("c_inf", "rlm", [("q", "c", INF)]),
          _rej("max_iter", "rlm", [("q", "max_iter", 0)]), _rej("tol", "rlm", [("q", "tol", 0.0)]),
          _rej("weights_misaligned", "rlm", [("ro", "weights", MISALIGN)]),
          _rej("l1_ratio", "elastic_net_cv", [("q", "l1_ratio", 2.0)]), _rej("grid_empty", "elastic_net_cv", [("q", "n_alphas", 0)]),
          _rej("grid_129", "elastic_net_cv", [("q", "n_alphas", 129)]),
          _rej("auto_one", "elastic_net_cv", [("q", "n_alphas", 1)], kw=dict(ENET_KW, n_alphas=6)),
          _rej("auto_eps", "elastic_net_cv", [("q", "eps", 0.0)], kw=dict(ENET_KW, n_alphas=6)),
          _rej("auto_ridge", "elastic_net_cv", [("q", "l1_ratio", 0.0)], kw=dict(ENET_KW, n_alphas=6)),
          _rej("grid_negative", "elastic_net_cv", [("q", "alphas[0]", -1.0)]),
          _rej("folds", "elastic_net_cv", [("q", "n_folds", 1)]), _rej("max_iter", "elastic_net_cv", [("q", "max_iter", 0)]),
          _rej("tol", "elastic_net_cv", [("q", "tol", 0.0)]),
          _rej("alpha", "glm", [("p", "alpha", 1.0)]), _rej("family", "glm", [("q", "family", 9)]),
          _rej("max_iter", "glm", [("q", "max_iter", 0)]), _rej("tol", "glm", [("q", "tol", NAN)]),
          _rej("linpred_misaligned", "glm", [("ro", "linpred", MISALIGN)]),
          _rej("alpha", "iv2sls", [("p", "alpha", 1.0)]), _rej("n_endog", "iv2sls", [("q", "n_endog", 0)]),
          _rej("instruments", "iv2sls", [("q", "n_instruments", 0)]), _rej("z_null", "iv2sls", [("q", "z_cols", None)]),
          _rej("cov_type", "iv2sls", [("q", "cov_type", 6)]),
          _rej("weights", "glsar", [("b", "weights", MISALIGN)]), _rej("null_policy_drop", "glsar", [("p", "null_policy", 2)]),
          _rej("method", "glsar", [("q", "method", 9)]), _rej("max_iter", "glsar", [("q", "max_iter", 0)]),
          _rej("tol_zero", "glsar", [("q", "tol", 0.0)]), _rej("tol_nan", "glsar", [("q", "tol", NAN)])]
for _c in CASES:
    _c["seed"] = zlib.crc32(_c["id"].encode())
    assert _c.get("want", "all") == "all" or set(_c["want"]) <= set(COMMON + OWN[_c["entry"]]), _c["id"]
assert len({c["id"] for c in CASES}) == len(CASES)


DIGEST_HEX = 16     # a digest in the file is the first 16 hex digits (64 bits) of the sha256: 2 890 of them stay a reviewable file


def digest(*arrays):
    return SR.digest(*arrays)[:DIGEST_HEX]


def dump(path, commit, cases):
    """The recording as JSON with one line per case, so that the file stays about as long as the case list."""
    head = json.dumps({"recorded_on_commit": commit, "device": "MI355X (gfx950)", "digest": f"sha256, first {DIGEST_HEX} hex digits"})
    body = ",\n".join(f"{json.dumps(cid)}:{json.dumps(by_dt, separators=(',', ':'))}" for cid, by_dt in cases.items())
    Path(path).write_text(head[:-1] + ', "cases": {\n' + body + "\n}}\n")


def load(path=PATH):
    """-> (commit, {(case id, dtype name): recorded entry})"""
    doc = json.loads(Path(path).read_text())
    return doc["recorded_on_commit"], {(cid, dt): e for cid, by_dt in doc["cases"].items() for dt, e in by_dt.items()}


def _sizes(case, dtype):
    if case["sizes"] != "glm_classes":
        return case["sizes"]
    # one group in each of glm's two resident classes and one beyond them (tiles of 256 rows, counted from a 16-byte grid point)
    from polars_ols_amd import _lib as L

    kt, cols, elem = case["k"] + int(bool(case.get("icpt"))), case["k"] + 1 + int(bool(case.get("weights"))) + int(bool(case.get("offset"))), \
        np.dtype(dtype).itemsize
    cap = L.lib().pols_glm_resident_tiles(kt, cols, elem, 1)
    cap2 = min(cap, L.lib().pols_glm_resident_tiles(kt, cols, elem, 2))
    assert 0 < cap2 < cap, (cap2, cap)
    return [cap2 * 256 - 40, 50, cap * 256 - 40, 0, cap * 256 + 300]


def frame(case, dtype):
    """-> dict of host arrays: y, cols, offs, valid (uint8 or None), w (or None), and the entry's further columns: offset (glm, or None),
    z (iv2sls: the instruments), ids (absorb: one int64 column, absorb2: two)"""
    rng = np.random.default_rng(case["seed"])
    entry = case["entry"]
    offs = np.concatenate([[0], np.cumsum(_sizes(case, dtype))]).astype(np.int64)
    n, k = int(offs[-1]), case["k"]
    cols = [rng.standard_normal(n).astype(dtype) for _ in range(k)]
    signal = sum(c.astype(np.float64) for c in cols) if cols else np.zeros(n)
    z, ids, offset = [], [], None
    if entry == "iv2sls":                      # the last regressor is endogenous: it shares the error u with the target
        z = [rng.standard_normal(n).astype(dtype) for _ in range(2)]
        u = rng.standard_normal(n)
        cols[-1] = (z[0].astype(np.float64) - 0.5 * z[1] + 0.7 * u + 0.3 * rng.standard_normal(n)).astype(dtype)
        y = (sum(c.astype(np.float64) for c in cols) + 0.5 * u + 0.3 * rng.standard_normal(n)).astype(dtype)
    elif entry == "glm":
        offset = (0.2 * rng.standard_normal(n)).astype(dtype) if case.get("offset") else None
        eta = 0.5 * signal + (offset.astype(np.float64) if offset is not None else 0.0)
        if case.get("kw", {}).get("family") == "poisson":
            y = rng.poisson(np.exp(0.3 * eta)).astype(dtype)
        else:
            y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(dtype)
    else:
        for i in range({"absorb": 1, "absorb2": 2}.get(entry, 0)):
            col = rng.integers(0, 7 - 2 * i, n).astype(np.int64)
            if case.get("ids") == "sorted":
                for s, e in zip(offs[:-1], offs[1:]):
                    col[s:e].sort()
            ids.append(col)
        y = (signal + sum(0.3 * (i + 1) * c for i, c in enumerate(ids)) + 0.5 * rng.standard_normal(n)).astype(dtype)
    w = rng.uniform(0.5, 2.0, n).astype(dtype) if case.get("weights") else None
    valid = None
    if case.get("nulls", 0.0) > 0:
        hit = rng.random(n) < case["nulls"]
        if case.get("mask"):
            valid = (~hit).astype(np.uint8)
        else:                                  # one NaN per null row, in a column drawn for the row: the target, a feature, an instrument, the weight
            rows = np.flatnonzero(hit)
            into = [y] + cols + z + ([w] if w is not None else [])
            for r, j in zip(rows, rng.integers(0, len(into), size=len(rows))):
                into[j][r] = np.nan
    if case.get("edge"):                       # (behind every draw: no other case's frame moves)
        cols[1][offs[0]:offs[1]] = cols[0][offs[0]:offs[1]]
    return dict(y=y, cols=cols, offs=offs, valid=valid, w=w, offset=offset, z=z, ids=ids)


def frame_digest(case, dtype):
    f = frame(case, dtype)
    return digest(f["y"], *f["cols"], f["offs"], f["valid"], f["w"], f["offset"], *f["z"], *f["ids"])


class _Poked:
    """The library as the engine sees it, with one entry wrapped: the structs the front end built are changed before the C entry runs."""

    def __init__(self, lib, fn, poke, dtype):
        self.__dict__.update(_lib=lib, _fn=fn, _poke=poke, _dtype=dtype, _keep=[])

    def __getattr__(self, name):
        real = getattr(self._lib, name)
        if name != self._fn:
            return real

        def call(h, b, p, q, o, ro):
            import torch

            s = dict(b=b._obj, p=p._obj, q=q._obj, o=o._obj, ro=ro._obj)
            for struct, field, value in self._poke:
                if value == "misalign":
                    big = torch.empty(int(s["b"].n_rows) + 1, dtype=torch.float32 if self._dtype == np.float32 else torch.float64, device="cuda")
                    self._keep.append(big)
                    value = big[1:].data_ptr()
                if field == "alphas[0]":
                    s[struct].alphas[0] = value
                    continue
                if (struct, field) == ("b", "n_rows"):          # the offsets have to end at n_rows for the size check to be reached
                    s["b"].group_offsets[s["b"].n_groups] = value
                setattr(s[struct], field, value)
            return real(h, b, p, q, o, ro)

        return call


def run(eng, case, dtype):
    """One case through the engine -> ("ok", last_kernel, {field: sha256 of the array's bytes}) or ("rejected", type, code, message)"""
    import torch

    from polars_ols_amd import _lib as L

    f = frame(case, dtype)
    host = bool(case.get("host"))
    put = (lambda a: a) if host else (lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda())
    entry, opts, kw = case["entry"], case.get("opts", {}), dict(case.get("kw", {}))
    want = case.get("want", "all")
    want = COMMON + OWN[entry] if want == "all" else tuple(want)
    kw.update(weights=put(f["w"]), valid=put(f["valid"]), add_intercept=bool(case.get("icpt")), null_policy=case.get("policy", "ignore"), want=want)
    y, cols = put(f["y"]), [put(c) for c in f["cols"]]
    lib = eng._lib
    try:
        for key, v in opts.items():
            eng.set_option(key, v)
        if case.get("poke"):
            eng._lib = _Poked(lib, FN[entry], case["poke"], dtype)
        if entry == "ridge_cv":
            out = eng.ridge_cv(y, cols, f["offs"], kw.pop("alphas"), **kw)
        elif entry == "elastic_net_cv":
            out = eng.elastic_net_cv(y, cols, f["offs"], kw.pop("alphas", None), **kw)
        elif entry == "glm":
            out = eng.glm(y, cols, f["offs"], offset=put(f["offset"]), **kw)
        elif entry == "iv2sls":
            out = eng.iv2sls(y, cols, [put(c) for c in f["z"]], f["offs"], **kw)
        elif entry == "absorb":
            out = eng.absorb(y, cols, put(f["ids"][0]), f["offs"], **kw)
        elif entry == "absorb2":
            out = eng.absorb2(y, cols, put(f["ids"][0]), put(f["ids"][1]), f["offs"], **kw)
        elif entry == "glsar":
            out = eng.glsar(y, cols, f["offs"], **kw)
        else:
            out = eng.rlm(y, cols, f["offs"], **kw)
        eng.synchronize()
        name = eng.last_kernel if len(f["offs"]) > 1 else None      # (a frame without groups launches nothing: the name is the last call's)
    except L.PolsError as e:
        if e.code == -3:                       # POLS_ERR_HIP: a device error is no rejection
            raise
        return "rejected", type(e).__name__, e.code, str(e)
    finally:
        eng._lib = lib
        for key in opts:
            eng.set_option(key, None)
    assert set(out) == set(want), (sorted(out), want)
    return "ok", name, {k: digest(a.cpu().numpy() if hasattr(a, "cpu") else a) for k, a in sorted(out.items())}
