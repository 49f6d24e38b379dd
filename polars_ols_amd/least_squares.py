"""Host-side mirror of the reference's Python operator interface for the hot path.

Same names, argument meaning, defaults and error behaviour as ``polars_ols/least_squares.py`` and the
``least_squares`` namespace of ``polars_ols/__init__.py`` (reference file:line cited per item), re-stated over a
dict-of-columns frame because Polars is not available in the build image: columns are 1-D numpy arrays (host path)
or CUDA torch tensors (device path), a *null* is a NaN, and ``.over(key)`` is done here by a stable sort-by-key
(what Polars' ``.over`` gather does on the host) followed by ONE batched call into libpols_mi355x for all groups.

    from polars_ols_amd import Frame, col
    df = Frame({"y": y, "x1": x1, "x2": x2, "group": g})
    pred = df.select(col("y").least_squares.ols("x1", "x2", mode="predictions").over("group"))["y"]
    coef = df.select(col("y").least_squares.from_formula("x1 + x2", mode="coefficients").over("group"))["coefficients"]

What runs where: null-policy row filtering, sqrt(w) handling for null policies, group sort / scatter are data
marshalling (the reference does them with Polars ops in src/expressions.rs:201-296 and least_squares.py:163-239);
every solve and prediction runs in the HIP kernels behind the C-ABI.  There is no CPU compute path.
"""
from __future__ import annotations

import logging
import re
from dataclasses import asdict, dataclass
from typing import Any, Dict, List, Literal, Optional, Sequence, Set, Tuple, Union, get_args

import numpy as np

from . import _lib
from ._lib import PolsPanic
from .engine import (Engine, Layout, _absorb_params, _absorb2_params, _enet_cv_params, _is_torch, _glm_params, _glsar_params, _iv_params,
                     _random_effects_params, _ridge_cv_grid, _rlm_params, default_engine)

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

logger = logging.getLogger(__name__)

__all__ = [
    "compute_least_squares", "compute_recursive_least_squares", "compute_rolling_least_squares",
    "compute_least_squares_from_formula", "compute_multi_target_least_squares", "predict",
    "OLSKwargs", "RLSKwargs", "RollingKwargs", "NullPolicy", "OutputMode", "SolveMethod",
    "Frame", "Expr", "col", "struct", "Coefficients", "Statistics", "Influence", "LeastSquares",
    "compute_ridge_cv", "RidgeCV",
    "compute_elastic_net_cv", "ElasticNetCV",
    "compute_rlm", "RLM",
    "compute_glm", "GLM",
    "compute_iv2sls", "IV2SLS",
    "compute_glsar", "GLSAR",
    "compute_absorbed_least_squares", "AbsorbedOLS",
    "compute_random_effects", "RandomEffects",
]

# ---- polars_ols/least_squares.py:47-63 --------------------------------------------------------------------------
NullPolicy = Literal["zero", "drop", "ignore", "drop_zero", "drop_y_zero_x", "drop_window"]
OutputMode = Literal["predictions", "residuals", "coefficients", "statistics", "influence"]
SolveMethod = Literal["qr", "svd", "chol", "lu", "cd", "cd_active_set"]

_VALID_NULL_POLICIES: Set[str] = set(get_args(NullPolicy))
_VALID_OUTPUT_MODES: Set[str] = set(get_args(OutputMode))
_VALID_SOLVE_METHODS: Set[Any] = set(get_args(SolveMethod)).union({None})
_EPSILON: float = 1.0e-12


@dataclass
class Kwargs:  # least_squares.py:66-77
    null_policy: str = "ignore"

    def to_dict(self) -> Dict[str, Any]:
        return asdict(self)

    def __post_init__(self):
        assert self.null_policy in _VALID_NULL_POLICIES, \
            f"'null_policy' must be one of {_VALID_NULL_POLICIES}. You passed: {self.null_policy}"


@dataclass
class OLSKwargs(Kwargs):  # least_squares.py:80-118
    alpha: Optional[float] = 0.0
    l1_ratio: Optional[float] = None
    max_iter: Optional[int] = 1_000
    tol: Optional[float] = 1.0e-5
    positive: Optional[bool] = False
    solve_method: Optional[str] = None
    rcond: Optional[float] = None

    def __post_init__(self):
        valid_ols_policies = _VALID_NULL_POLICIES - {"drop_window"}
        assert self.null_policy in valid_ols_policies, \
            f"'null_policy' must be one of {valid_ols_policies}. You passed: {self.null_policy}"
        assert self.solve_method in _VALID_SOLVE_METHODS, \
            f"'solve_method' must be one of {_VALID_SOLVE_METHODS}. You passed: {self.solve_method}"


@dataclass
class RLSKwargs(Kwargs):  # least_squares.py:121-140
    half_life: Optional[float] = None
    initial_state_covariance: Optional[float] = 10.0
    initial_state_mean: Union[Optional[List[float]], float] = None
    null_policy: str = "drop"


@dataclass
class RollingKwargs(Kwargs):  # least_squares.py:143-160
    # (use_woodbury is accepted and does not select a code path; at 11 to 32 features a window without a Cholesky factorisation gives NaN
    #  where the reference's LU gives inf / NaN / huge numbers -- Engine.plan_rolling_least_squares' docstring, include/pols_mi355x.h)
    window_size: int = 1_000_000
    min_periods: Optional[int] = None
    use_woodbury: Optional[bool] = None
    alpha: Optional[float] = None
    null_policy: str = "drop_window"


# ---- frame / expression plumbing ---------------------------------------------------------------------------------

class Coefficients:
    """The coefficients struct of the reference (src/expressions.rs:114-143): one field per feature, NaN = null.

    ``values`` is [n_groups x k] for static models (``keys`` = the group keys in sorted order; Polars broadcasts the
    struct to every row of the group -- ``to_rows()``), [n_rows x k] for rls / rolling."""

    def __init__(self, names: Sequence[str], values, keys=None, row_group=None):
        self.names, self.values, self.keys, self._row_group = list(names), values, keys, row_group

    def unnest(self) -> Dict[str, Any]:
        return {n: self.values[:, j] for j, n in enumerate(self.names)}

    def to_rows(self):
        return self.values if self._row_group is None else self.values[self._row_group]

    def __repr__(self):
        return f"Coefficients(names={self.names}, shape={tuple(self.values.shape)})"


class Expr:
    """A column reference (optionally scaled) or a deferred least-squares expression."""

    def __init__(self, name: Optional[str] = None, scale: float = 1.0, fn=None, over=None, alias: Optional[str] = None,
                 factors: Tuple[str, ...] = ()):
        self._name, self._scale, self._fn, self._over, self._alias = name, scale, fn, over, alias
        self._factors = tuple(factors)                         # further columns multiplied in (formula interactions ``a:b``)

    # column arithmetic that the reference's own tests use on features (e.g. ``-pl.col("x2")``, test_ols.py:615) and that
    # its formula front-end builds for interaction terms (utils.py:104-106)
    def __neg__(self):
        return Expr(self._name, -self._scale, alias=self._alias, factors=self._factors)

    def __mul__(self, c):
        if isinstance(c, Expr):
            if c._fn is not None or self._fn is not None:
                raise TypeError("cannot multiply deferred least-squares expressions")
            return Expr(self._name, self._scale * c._scale, alias=self._alias, factors=self._factors + (c._name,) + c._factors)
        return Expr(self._name, self._scale * float(c), alias=self._alias, factors=self._factors)

    __rmul__ = __mul__

    def alias(self, name: str) -> "Expr":
        return Expr(self._name, self._scale, self._fn, self._over, name, self._factors)

    def over(self, key) -> "Expr":
        return Expr(self._name, self._scale, self._fn, key, self._alias, self._factors)

    @property
    def least_squares(self) -> "LeastSquares":
        return LeastSquares(self)

    @property
    def output_name(self) -> str:
        return self._alias or self._name

    def _column(self, frame: "Frame"):
        c = frame[self._name]
        for f in self._factors:
            c = c * frame[f]
        return c if self._scale == 1.0 else c * self._scale


def col(name: str) -> Expr:
    return Expr(name)


def struct(*cols) -> Expr:
    """pl.struct(...) stand-in: bundles the target columns of a multi-target regression."""
    fields = [parse_into_expr(c) for c in cols]
    e = Expr(fields[0]._name)
    e._fields = fields
    return e


def parse_into_expr(e) -> Expr:  # polars_ols/utils.py:21-58 (strings are column names)
    if isinstance(e, Expr):
        return e
    if isinstance(e, str):
        return Expr(e)
    raise TypeError(f"cannot parse {type(e)} into a column expression")


class Frame(dict):
    """dict of equally long 1-D columns (numpy or CUDA torch)."""

    def select(self, *exprs: Expr, engine: Optional[Engine] = None) -> Dict[str, Any]:
        out: Dict[str, Any] = {}
        for e in exprs:
            if e._fn is None:
                out[e.output_name] = e._column(self)
            else:
                name, val = e._fn(self, e._over, engine)
                out[e._alias or name] = val
        return out

    def with_columns(self, *exprs: Expr, engine: Optional[Engine] = None) -> "Frame":
        f = Frame(self)
        f.update(self.select(*exprs, engine=engine))
        return f


# ---- helpers over numpy / torch columns ---------------------------------------------------------------------------

def _xp(a):
    return torch if _is_torch(a) else np


def _take(a, idx):
    return a[idx]


def _to_index(idx, like):
    if _is_torch(idx):
        return idx if _is_torch(like) else idx.cpu().numpy()
    if _is_torch(like):
        return torch.as_tensor(idx, device=like.device)
    return idx


class _Groups:
    """What ``.over(key)`` needs (README.md:19, :57): the groups' offsets / keys and the row movers between frame order and the
    group-sorted order the batched entries take.  Built by the engine's native ingestion (``pols_layout_*``: stable radix sort,
    run lengths, gather kernels) wherever the key column lives; non-integer keys are dictionary-encoded first, like Polars'
    own group-by.  ``key is None`` is the whole-frame fit: one group, nothing moves."""

    def __init__(self, eng: Engine, key, n: int):
        self._lay, self.n = None, n
        if key is None:
            self.offsets, self.keys, self.identity = np.array([0, n], dtype=np.int64), None, True
            return
        codes, uniq = key, None
        if _is_torch(key) and not key.is_cuda:
            key = codes = key.numpy()
        if _is_torch(key):
            if key.dtype.is_floating_point or key.dtype.is_complex:
                uniq, codes = torch.unique(key, return_inverse=True)
                uniq = uniq.cpu().numpy()
        else:
            codes = np.asarray(key)
            if codes.dtype.kind not in "iub":
                uniq, codes = np.unique(codes, return_inverse=True)
        self._lay = Layout(eng, codes)
        self.offsets, self.identity = self._lay.offsets, self._lay.identity
        self.keys = self._lay.keys if uniq is None else uniq[self._lay.keys]

    def take(self, cols):
        """frame order -> group order; ``None`` entries pass through."""
        return list(cols) if self.identity else self._lay.take(cols)

    def untake(self, a):
        """group order -> frame order (a column or an [n, k] table)."""
        return a if self.identity else self._lay.untake([a])[0]

    def gid_frame(self, like):
        """index of its group for every frame row, where ``like`` lives."""
        if self._lay is None:
            g = np.zeros(self.n, dtype=np.int64)
        else:
            g = self._lay.row_groups()
        return _to_index(g, like)

    def gid_sorted(self, like):
        """the same for every group-sorted row."""
        if self._lay is not None and self._lay.on_device and _is_torch(like):
            return self._lay.take([self._lay.row_groups()])[0]
        return _to_index(np.repeat(np.arange(len(self.offsets) - 1, dtype=np.int64), np.diff(self.offsets)), like)


def _pre_process_data(frame: Frame, target: Expr, features: Sequence[Expr], sample_weights, add_intercept: bool):
    """least_squares.py:163-196 up to (not including) the sqrt_w multiplications, which the kernels fuse:
    returns (y, x columns, feature names, add_intercept flag for the engine, weights or None)."""
    names = [f.output_name for f in features]
    icpt = False
    if add_intercept:
        if any(n == "const" for n in names):
            logger.info("feature named 'const' already detected, assuming it is an intercept")  # :185-186
        else:
            names = names + ["const"]                                                          # appended LAST (:188)
            icpt = True
    w = None
    if sample_weights is not None:
        w = parse_into_expr(sample_weights)._column(frame)
        # sqrt_w = w.sqrt().fill_null(1e-12)  (:193): a null weight acts as weight 1e-24.  That fill happens BEHIND the C-ABI, on the
        # device (pols_least_squares: one pass over the weights column unless the batch promises null_free; the dynamic and Arrow
        # entries in dyn_prep.hip / arrow.hip) -- nothing to do here.
    return target._column(frame), [f._column(frame) for f in features], names, icpt, w


def _has_nan(a) -> bool:
    return bool(torch.isnan(a).any()) if _is_torch(a) else bool(np.isnan(a).any())


def _ones_like(a):
    return torch.ones_like(a) if _is_torch(a) else np.ones_like(a)


def _static_fit(eng: Engine, y, xs, offs, w, icpt: bool, want, kw: OLSKwargs):
    d = kw.to_dict()
    d.pop("null_policy")
    return eng.least_squares(y, xs, offs, weights=w, add_intercept=icpt, want=want, **d)


class Statistics(dict):
    """mode="statistics": the fields of the reference's struct (src/expressions.rs:448-466), one entry per group:
    ``r2 mae mse`` [G], ``feature_names``, ``coefficients standard_errors t_values p_values`` [G, k]; ``keys`` holds the
    group keys of an ``.over`` (None for a whole-frame fit, where G == 1)."""

    def __init__(self, names, out, keys):
        super().__init__(r2=out["r2"], mae=out["mae"], mse=out["mse"], feature_names=list(names),
                         coefficients=out["coef"], standard_errors=out["std_err"], t_values=out["t_values"],
                         p_values=out["p_values"])
        self.keys_ = keys
        # cov_type="cluster": the clusters G per group ([G] one-way, [G, 2] two-way: G_A, G_B); None otherwise
        self.n_clusters = out.get("n_clusters")
        if self.n_clusters is not None:
            self["n_clusters"] = self.n_clusters


def _static_statistics(eng: Engine, y, xs, offs, w, icpt: bool, kw: OLSKwargs, names, keys, cov=None) -> Statistics:
    d = kw.to_dict()
    if cov is not None and cov[0] == "cluster":               # ("cluster", id columns in group order, use_correction)
        d["cov_type"], d["clusters"], d["use_correction"] = cov
    elif cov is not None:                                      # (cov_type, maxlags): robust standard errors / t / p
        d["cov_type"], d["maxlags"] = cov
    out = eng.least_squares_statistics(y, xs, offs, weights=w, add_intercept=icpt, **d)
    st = out["status"]
    bad = bool((st == 4).any())
    if bad:  # the reference asserts df > 0 and panics the whole query (src/statistics.rs:131-134)
        raise PolsPanic(-4, "Degrees of freedom <= 0. Cannot compute standard errors.")
    return Statistics(names, out, keys)


class Influence(dict):
    """mode="influence": per-row influence diagnostics and prediction intervals (pols_least_squares_influence; the definitions are
    in include/pols_mi355x.h).  The requested per-row columns -- any of ``leverage student_internal student_external cooks_d dffits
    se_mean se_obs mean_lo mean_hi obs_lo obs_hi`` -- are in the FRAME's row order (un-taken through ``.over`` like predictions);
    ``sigma2 df t_crit`` [G] are per group and ``keys`` holds the group keys of an ``.over`` (None for a whole-frame fit).

    A group with df <= 0 has NaN rows and raises nothing: one short group should not fail a per-row result for a whole panel
    (mode="statistics" raises there, like the reference)."""

    def __init__(self, fields, out, keys, untake):
        super().__init__({f: untake(out[f]) for f in fields})
        for g in _lib.INFLUENCE_GROUP_FIELDS:
            self[g] = out[g]
        self["keys"] = keys
        self.fields = list(fields)
        self.keys_ = keys


def _influence_request(mode: str, influence_kwds: Optional[Dict[str, Any]], kind: str = "ols", kw: Optional[OLSKwargs] = None,
                       cov_type: str = "nonrobust", cov_kwds: Optional[Dict[str, Any]] = None):
    """(level, fields) of a mode="influence" request, None for every other mode; ValueError for what has no influence form: RLS /
    rolling / expanding / multi-target models, influence_kwds with another mode, unknown keys or fields, a level outside (0, 1), a
    non-default cov_type, and l1 (lasso, elastic net) or positive fits, where no hat matrix is defined."""
    if mode != "influence":
        if influence_kwds:
            raise ValueError(f"influence_kwds apply to mode='influence' only (got mode={mode!r})")
        return None
    if kind != "ols":
        raise ValueError(f"mode='influence' applies to single-target least squares, not to {kind} models")
    if cov_type != "nonrobust" or cov_kwds:
        raise ValueError(f"mode='influence' has only the constant-variance form: cov_type={cov_type!r} / cov_kwds do not apply")
    kwds = dict(influence_kwds or {})
    unknown = set(kwds) - {"level", "fields"}
    if unknown:
        raise ValueError(f"unknown influence_kwds {sorted(unknown)} (level, fields)")
    level = kwds.get("level", 0.95)
    if isinstance(level, bool) or not isinstance(level, (int, float)) or not 0.0 < float(level) < 1.0:
        raise ValueError(f"influence_kwds['level'] must lie in (0, 1), got {level!r}")
    fields = kwds.get("fields")
    fields = list(_lib.INFLUENCE_FIELDS) if fields is None else ([fields] if isinstance(fields, str) else list(fields))
    bad = [f for f in fields if f not in _lib.INFLUENCE_FIELDS]
    if bad or not fields:
        raise ValueError(f"unknown influence fields {bad}; known: {list(_lib.INFLUENCE_FIELDS)}")
    if kw is not None and (kw.positive or (kw.l1_ratio is not None and kw.l1_ratio > 0.0)):
        raise ValueError("mode='influence' needs a hat matrix: not defined for l1-penalised (lasso, elastic net) or positive fits")
    return float(level), fields


def _apply_static(frame: Frame, over, eng: Optional[Engine], target: Expr, features: Sequence[Expr], sample_weights,
                  add_intercept: bool, mode: str, kw: OLSKwargs, cov=None, infl=None):
    """compute_least_squares body: least_squares.py:199-239 + src/expressions.rs:390-446 (null policies :201-296)."""
    y, xs, names, icpt, w = _pre_process_data(frame, target, features, sample_weights, add_intercept)
    n = y.shape[0]
    eng = eng or default_engine(y.device.index or 0 if _is_torch(y) else 0)
    # ---- group layout (.over)
    grp = _Groups(eng, None if over is None else (frame[over] if isinstance(over, str) else over), n)
    offs, keys = grp.offsets, grp.keys
    ids = _cluster_ids(frame, cov[1], y) if cov is not None and cov[0] == "cluster" else []
    moved = grp.take([y, w] + list(xs) + ids)                 # (cluster ids move with their rows, 8 bytes each)
    y_s, w_s, xs_s = moved[0], moved[1], moved[2:2 + len(xs)]
    if ids:
        cov = ("cluster", moved[2 + len(xs):], cov[2])

    policy = kw.null_policy
    if mode == "influence":
        level, fields = infl
        out = eng.least_squares_influence(y_s, xs_s, offs, weights=w_s, add_intercept=icpt, interval_level=level,
                                          want=tuple(fields) + _lib.INFLUENCE_GROUP_FIELDS, **kw.to_dict())
        return "influence", Influence(fields, out, keys, grp.untake)
    if mode != "statistics":
        # Null policies are fused into the kernels (staging pass: dropped rows get weight 0, surviving nulls become 0;
        # prediction pass: zero-filled features, "drop" masks the rows that were not fitted) -- ex.rs:201-296, 398-427.
        want = ("coef",) if mode == "coefficients" else (("pred",) if mode == "predictions" else ("resid",))
        d = kw.to_dict()
        out = eng.least_squares(y_s, xs_s, offs, weights=w_s, add_intercept=icpt, want=want, **d)
        coef, pred = out.get("coef"), out.get("pred") if mode == "predictions" else out.get("resid")
    else:
        # handle_nulls ahead of the statistics code (ex.rs:469-471): the entry filters / zero-fills on the device itself
        return "statistics", _static_statistics(eng, y_s, xs_s, offs, w_s, icpt, kw, names, keys, cov)
    if mode == "coefficients":
        # without .over the single struct broadcasts to every row of the frame, like a Polars scalar (gid is all zeros)
        return "coefficients", Coefficients(names, coef, keys, grp.gid_frame(coef))
    return target.output_name, grp.untake(pred)                # back to the frame's row order


class RidgeCV(dict):
    """mode="cv" of a ridge path (pols_ridge_cv; the definitions are in include/pols_mi355x.h), one entry per group: ``alpha``
    (the chosen candidate), ``alpha_index`` (its index in ``alphas``, -1 where no candidate is usable), ``score`` (its leave-one-out
    mean squared error) [G], ``cv_scores`` [G, n_alphas] (NaN for an unusable candidate); ``alphas`` is the grid as passed and
    ``keys`` holds the group keys of an ``.over`` (None for a whole-frame fit, where G == 1)."""

    def __init__(self, out, keys, alphas):
        super().__init__(alpha=out["alpha"], alpha_index=out["alpha_index"], score=out["score"], cv_scores=out["cv_scores"],
                         keys=keys, alphas=alphas)
        self.keys_ = keys


_VALID_RIDGE_CV_MODES = ("predictions", "residuals", "coefficients", "cv")


def _apply_ridge_cv(frame: Frame, over, eng: Optional[Engine], target: Expr, features: Sequence[Expr], sample_weights,
                    add_intercept: bool, mode: str, grid, null_policy: str):
    """compute_ridge_cv body: the group layout of _apply_static around Engine.ridge_cv."""
    y, xs, names, icpt, w = _pre_process_data(frame, target, features, sample_weights, add_intercept)
    eng = eng or default_engine(y.device.index or 0 if _is_torch(y) else 0)
    grp = _Groups(eng, None if over is None else (frame[over] if isinstance(over, str) else over), y.shape[0])
    moved = grp.take([y, w] + list(xs))
    want = {"predictions": ("pred",), "residuals": ("resid",), "coefficients": ("coef",),
            "cv": ("alpha", "alpha_index", "score", "cv_scores")}[mode]
    out = eng.ridge_cv(moved[0], moved[2:], grp.offsets, grid, want=want, weights=moved[1], add_intercept=icpt, null_policy=null_policy)
    if mode == "cv":
        return "cv", RidgeCV(out, grp.keys, grid.copy())
    if mode == "coefficients":
        return "coefficients", Coefficients(names, out["coef"], grp.keys, grp.gid_frame(out["coef"]))
    return target.output_name, grp.untake(out["pred"] if mode == "predictions" else out["resid"])


class ElasticNetCV(dict):
    """mode="cv" of an elastic-net path (pols_elastic_net_cv; the definitions are in include/pols_mi355x.h), one entry per group:
    ``alpha`` (the chosen candidate), ``alpha_index`` (its index, -1 where there is no choice), ``score`` (its mean K-fold
    validation error), ``status`` [G], ``cv_scores``, ``alphas`` (every group's candidates) and ``n_iter`` [G, n_alphas]; ``keys``
    holds the group keys of an ``.over`` (None for a whole-frame fit, where G == 1)."""

    def __init__(self, out, keys, l1_ratio, n_folds):
        super().__init__(alpha=out["alpha"], alpha_index=out["alpha_index"], score=out["score"], status=out["status"],
                         cv_scores=out["cv_scores"], alphas=out["alphas_used"], n_iter=out["n_iter"], keys=keys, l1_ratio=l1_ratio,
                         n_folds=n_folds)
        self.keys_ = keys


_VALID_ENET_CV_MODES = ("predictions", "residuals", "coefficients", "cv")


def _apply_enet_cv(frame: Frame, over, eng: Optional[Engine], target: Expr, features: Sequence[Expr], sample_weights,
                   add_intercept: bool, mode: str, null_policy: str, kw):
    """compute_elastic_net_cv body: the group layout of _apply_static around Engine.elastic_net_cv."""
    y, xs, names, icpt, w = _pre_process_data(frame, target, features, sample_weights, add_intercept)
    eng = eng or default_engine(y.device.index or 0 if _is_torch(y) else 0)
    grp = _Groups(eng, None if over is None else (frame[over] if isinstance(over, str) else over), y.shape[0])
    moved = grp.take([y, w] + list(xs))
    want = {"predictions": ("pred",), "residuals": ("resid",), "coefficients": ("coef",),
            "cv": ("status", "alpha", "alpha_index", "score", "cv_scores", "alphas_used", "n_iter")}[mode]
    out = eng.elastic_net_cv(moved[0], moved[2:], grp.offsets, want=want, weights=moved[1], add_intercept=icpt, null_policy=null_policy, **kw)
    if mode == "cv":
        return "cv", ElasticNetCV(out, grp.keys, kw["l1_ratio"], kw["n_folds"])
    if mode == "coefficients":
        return "coefficients", Coefficients(names, out["coef"], grp.keys, grp.gid_frame(out["coef"]))
    return target.output_name, grp.untake(out["pred"] if mode == "predictions" else out["resid"])


class RLM(dict):
    """mode="rlm" of an M-estimator fit (pols_rlm; the definitions are in include/pols_mi355x.h): per group ``coef`` [G, k],
    ``scale`` (the last MAD scale), ``n_iter`` (updates made) and ``status`` (0 converged, 1 no fit, 2 no rows, 3 stopped at
    max_iter) [G]; ``weights`` holds the robust weights of the last update in FRAME order (NaN for the rows outside the fit);
    ``keys`` holds the group keys of an ``.over`` (None for a whole-frame fit, where G == 1)."""

    def __init__(self, out, keys, weights, norm, c):
        super().__init__(coef=out["coef"], scale=out["scale"], n_iter=out["n_iter"], status=out["status"], weights=weights,
                         keys=keys, norm=norm, c=c)
        self.keys_ = keys


_VALID_RLM_MODES = ("predictions", "residuals", "coefficients", "rlm")


def _apply_rlm(frame: Frame, over, eng: Optional[Engine], target: Expr, features: Sequence[Expr], sample_weights,
               add_intercept: bool, mode: str, norm: str, c, max_iter: int, tol: float, null_policy: str):
    """compute_rlm body: the group layout of _apply_static around Engine.rlm."""
    y, xs, names, icpt, w = _pre_process_data(frame, target, features, sample_weights, add_intercept)
    eng = eng or default_engine(y.device.index or 0 if _is_torch(y) else 0)
    grp = _Groups(eng, None if over is None else (frame[over] if isinstance(over, str) else over), y.shape[0])
    moved = grp.take([y, w] + list(xs))
    want = {"predictions": ("pred",), "residuals": ("resid",), "coefficients": ("coef",),
            "rlm": ("coef", "status", "scale", "n_iter", "weights")}[mode]
    out = eng.rlm(moved[0], moved[2:], grp.offsets, norm=norm, c=c, max_iter=max_iter, tol=tol, want=want, weights=moved[1],
                  add_intercept=icpt, null_policy=null_policy)
    if mode == "rlm":
        return "rlm", RLM(out, grp.keys, grp.untake(out["weights"]), norm, c)
    if mode == "coefficients":
        return "coefficients", Coefficients(names, out["coef"], grp.keys, grp.gid_frame(out["coef"]))
    return target.output_name, grp.untake(out["pred"] if mode == "predictions" else out["resid"])


class GLM(dict):
    """mode="glm" of a generalised linear model fit (pols_glm; the definitions are in include/pols_mi355x.h): per group ``coef`` and
    ``se`` (standard errors, dispersion 1) [G, k], ``deviance``, ``n_iter`` (updates made) and ``status`` (0 converged, 1 no fit,
    2 no rows, 3 stopped at max_iter) [G]; ``linpred`` holds the linear predictor eta in FRAME order; ``keys`` holds the group keys
    of an ``.over`` (None for a whole-frame fit, where G == 1)."""

    def __init__(self, out, keys, linpred, family):
        super().__init__(coef=out["coef"], se=out["se"], deviance=out["deviance"], n_iter=out["n_iter"], status=out["status"],
                         linpred=linpred, keys=keys, family=family)
        self.keys_ = keys


_VALID_GLM_MODES = ("predictions", "residuals", "coefficients", "glm")


def _apply_glm(frame: Frame, over, eng: Optional[Engine], target: Expr, features: Sequence[Expr], sample_weights, offset,
               add_intercept: bool, mode: str, family: str, max_iter: int, tol: float, null_policy: str):
    """compute_glm body: the group layout of _apply_static around Engine.glm."""
    y, xs, names, icpt, w = _pre_process_data(frame, target, features, sample_weights, add_intercept)
    off = None if offset is None else parse_into_expr(offset)._column(frame)
    eng = eng or default_engine(y.device.index or 0 if _is_torch(y) else 0)
    grp = _Groups(eng, None if over is None else (frame[over] if isinstance(over, str) else over), y.shape[0])
    moved = grp.take([y, w, off] + list(xs))
    want = {"predictions": ("pred",), "residuals": ("resid",), "coefficients": ("coef",),
            "glm": ("coef", "status", "deviance", "se", "n_iter", "linpred")}[mode]
    out = eng.glm(moved[0], moved[3:], grp.offsets, family=family, offset=moved[2], max_iter=max_iter, tol=tol, want=want,
                  weights=moved[1], add_intercept=icpt, null_policy=null_policy)
    if mode == "glm":
        return "glm", GLM(out, grp.keys, grp.untake(out["linpred"]), family)
    if mode == "coefficients":
        return "coefficients", Coefficients(names, out["coef"], grp.keys, grp.gid_frame(out["coef"]))
    return target.output_name, grp.untake(out["pred"] if mode == "predictions" else out["resid"])


class IV2SLS(dict):
    """mode="statistics" of a two-stage least squares fit (pols_iv2sls; the definitions are in include/pols_mi355x.h): per group
    ``coefficients standard_errors t_values p_values`` [G, k] (``feature_names``: exogenous, endogenous, const), ``cov`` [G, k, k],
    ``sigma2 sargan sargan_p n_obs status`` [G] and ``first_stage_f partial_r2`` [G, n_endog] (``endog_names``); ``keys`` holds the
    group keys of an ``.over`` (None for a whole-frame fit, where G == 1)."""

    def __init__(self, names, endog_names, out, keys, cov_type):
        super().__init__(feature_names=list(names), endog_names=list(endog_names), coefficients=out["coef"], standard_errors=out["se"],
                         t_values=out["t_values"], p_values=out["p_values"], cov=out["cov"], sigma2=out["sigma2"],
                         first_stage_f=out["first_stage_f"], partial_r2=out["partial_r2"], sargan=out["sargan"],
                         sargan_p=out["sargan_p"], n_obs=out["n_obs"], status=out["status"], keys=keys, cov_type=cov_type)
        self.keys_ = keys


_VALID_IV_MODES = ("predictions", "residuals", "coefficients", "statistics")


def _apply_iv2sls(frame: Frame, over, eng: Optional[Engine], target: Expr, exog: Sequence[Expr], endog: Sequence[Expr],
                  instruments: Sequence[Expr], sample_weights, add_intercept: bool, mode: str, cov_type: str, small_sample: bool,
                  null_policy: str):
    """compute_iv2sls body: the group layout of _apply_static around Engine.iv2sls."""
    feats = list(exog) + list(endog)
    y, xs, names, icpt, w = _pre_process_data(frame, target, feats, sample_weights, add_intercept)
    zs = [z._column(frame) for z in instruments]
    eng = eng or default_engine(y.device.index or 0 if _is_torch(y) else 0)
    grp = _Groups(eng, None if over is None else (frame[over] if isinstance(over, str) else over), y.shape[0])
    moved = grp.take([y, w] + list(xs) + zs)
    want = {"predictions": ("pred",), "residuals": ("resid",), "coefficients": ("coef",),
            "statistics": ("coef", "status") + _lib.IV_FIELDS}[mode]
    out = eng.iv2sls(moved[0], moved[2:2 + len(xs)], moved[2 + len(xs):], grp.offsets, n_endog=len(endog), cov_type=cov_type,
                     small_sample=small_sample, want=want, weights=moved[1], add_intercept=icpt, null_policy=null_policy)
    if mode == "statistics":
        return "statistics", IV2SLS(names, [e.output_name for e in endog], out, grp.keys, cov_type)
    if mode == "coefficients":
        return "coefficients", Coefficients(names, out["coef"], grp.keys, grp.gid_frame(out["coef"]))
    return target.output_name, grp.untake(out["pred"] if mode == "predictions" else out["resid"])


class GLSAR(dict):
    """mode="statistics" of an AR(1) feasible GLS fit (pols_glsar; the definitions are in include/pols_mi355x.h): per group
    ``coefficients standard_errors t_values p_values`` [G, k] (``feature_names``), ``cov`` [G, k, k], ``sigma2 rho dw dw_ols n_iter
    n_obs status`` [G] (``rho``: the AR(1) coefficient of the errors, ``dw`` / ``dw_ols``: Durbin-Watson of the transformed and of the
    OLS residuals, status 3 = stopped at max_iter); ``keys`` holds the group keys of an ``.over`` (None for a whole-frame fit,
    where G == 1)."""

    def __init__(self, names, out, keys, method):
        super().__init__(feature_names=list(names), keys=keys, coefficients=out["coef"], standard_errors=out["se"],
                         t_values=out["t_values"], p_values=out["p_values"], cov=out["cov"], sigma2=out["sigma2"], rho=out["rho"],
                         dw=out["dw"], dw_ols=out["dw_ols"], n_iter=out["n_iter"], n_obs=out["n_obs"], status=out["status"],
                         method=method)
        self.keys_ = keys


_VALID_GLSAR_MODES = ("predictions", "residuals", "coefficients", "statistics")


def _apply_glsar(frame: Frame, over, eng: Optional[Engine], target: Expr, features: Sequence[Expr], add_intercept: bool, mode: str,
                 method: str, max_iter: int, tol: float, null_policy: str):
    """compute_glsar body: the group layout of _apply_static around Engine.glsar (the rows of a group keep their frame order)."""
    y, xs, names, icpt, _ = _pre_process_data(frame, target, features, None, add_intercept)
    eng = eng or default_engine(y.device.index or 0 if _is_torch(y) else 0)
    grp = _Groups(eng, None if over is None else (frame[over] if isinstance(over, str) else over), y.shape[0])
    moved = grp.take([y] + list(xs))
    want = {"predictions": ("pred",), "residuals": ("resid",), "coefficients": ("coef",),
            "statistics": ("coef", "status") + _lib.GLSAR_FIELDS}[mode]
    out = eng.glsar(moved[0], moved[1:], grp.offsets, method=method, max_iter=max_iter, tol=tol, want=want, add_intercept=icpt,
                    null_policy=null_policy)
    if mode == "statistics":
        return "statistics", GLSAR(names, out, grp.keys, method)
    if mode == "coefficients":
        return "coefficients", Coefficients(names, out["coef"], grp.keys, grp.gid_frame(out["coef"]))
    return target.output_name, grp.untake(out["pred"] if mode == "predictions" else out["resid"])


class AbsorbedOLS(dict):
    """mode="statistics" of an absorbed-effect fit (pols_least_squares_absorb; the definitions are in include/pols_mi355x.h): per
    group ``coefficients standard_errors t_values p_values`` [G, k] (``feature_names``; with an intercept the last coefficient is the
    mean effect c0 and its standard error / t / p are NaN), ``sigma2 r2_within r2 n_obs n_categories status`` [G]; ``keys`` holds the
    group keys of an ``.over`` (None for a whole-frame fit, where G == 1).  A two-way fit (pols_least_squares_absorb2) also carries
    ``n_categories2 n_components n_iter`` [G]; a one-way fit has no such keys."""

    def __init__(self, names, out, keys, cov_type):
        super().__init__(feature_names=list(names), coefficients=out["coef"], standard_errors=out["se"], t_values=out["t_values"],
                         p_values=out["p_values"], sigma2=out["sigma2"], r2_within=out["r2_within"], r2=out["r2"], n_obs=out["n_obs"],
                         n_categories=out["n_categories"], status=out["status"], keys=keys, cov_type=cov_type)
        for key in ("n_categories2", "n_components", "n_iter"):    # (a two-way fit only: the one-way object keeps its keys)
            if key in out:
                self[key] = out[key]
        self.keys_ = keys


_VALID_ABSORB_MODES = ("predictions", "residuals", "coefficients", "statistics", "effects")


def _apply_absorb(frame: Frame, over, eng: Optional[Engine], target: Expr, features: Sequence[Expr], absorb, sample_weights,
                  add_intercept: bool, mode: str, cov_type: str, null_policy: str, two_way=None):
    """compute_absorbed_least_squares body: the group layout of _apply_static around Engine.absorb (``two_way``: the max_iter / tol of
    Engine.absorb2, ``absorb`` then holds two columns); the id columns move with their rows."""
    y, xs, names, icpt, w = _pre_process_data(frame, target, features, sample_weights, add_intercept)
    ids = _cluster_ids(frame, list(absorb) if two_way is not None else [absorb], y)
    eng = eng or default_engine(y.device.index or 0 if _is_torch(y) else 0)
    grp = _Groups(eng, None if over is None else (frame[over] if isinstance(over, str) else over), y.shape[0])
    moved = grp.take([y, w] + list(xs) + ids)
    ys, ws, xss, idss = moved[0], moved[1], moved[2:2 + len(xs)], moved[2 + len(xs):]
    effects = ("fe",) if two_way is None else ("fe1", "fe2")
    own = _lib.ABSORB_FIELDS if two_way is None else _lib.ABSORB2_FIELDS
    want = {"predictions": ("pred",), "residuals": ("resid",), "coefficients": ("coef",), "effects": effects,
            "statistics": ("coef", "status") + tuple(f for f in own if f not in effects)}[mode]
    common = dict(cov_type=cov_type, want=want, weights=ws, add_intercept=icpt, null_policy=null_policy)
    if two_way is None:
        out = eng.absorb(ys, xss, idss[0], grp.offsets, **common)
    else:
        out = eng.absorb2(ys, xss, idss[0], idss[1], grp.offsets, max_iter=two_way[0], tol=two_way[1], **common)
    if mode == "statistics":
        return "statistics", AbsorbedOLS(names, out, grp.keys, cov_type)
    if mode == "coefficients":
        return "coefficients", Coefficients(names, out["coef"], grp.keys, grp.gid_frame(out["coef"]))
    if mode == "effects" and two_way is not None:                  # both effects, keyed by the absorbed columns (in their order)
        keys = [c if isinstance(c, str) else f"effect_{j + 1}" for j, c in enumerate(absorb)]
        return target.output_name, {key: grp.untake(out[f]) for key, f in zip(keys, effects)}
    return target.output_name, grp.untake(out[{"predictions": "pred", "residuals": "resid", "effects": "fe"}[mode]])


class RandomEffects(dict):
    """mode="statistics" of a random-effects fit (pols_random_effects; the definitions are in include/pols_mi355x.h): per group
    ``coefficients standard_errors t_values p_values coefficients_between`` [G, k] (``feature_names``), ``coefficients_within``
    [G, n_features], ``sigma2_e sigma2_u rho hausman hausman_p n_obs n_categories status`` [G]; ``keys`` holds the group keys of an
    ``.over`` (None for a whole-frame fit, where G == 1)."""

    def __init__(self, names, out, keys):
        super().__init__(feature_names=list(names), keys=keys, coefficients=out["coef"], standard_errors=out["se"],
                         t_values=out["t_values"], p_values=out["p_values"], coefficients_between=out["coef_between"],
                         coefficients_within=out["coef_within"], sigma2_e=out["sigma2_e"], sigma2_u=out["sigma2_u"], rho=out["rho"],
                         hausman=out["hausman"], hausman_p=out["hausman_p"], n_obs=out["n_obs"], n_categories=out["n_categories"],
                         status=out["status"])
        self.keys_ = keys


_VALID_RANDOM_EFFECTS_MODES = ("predictions", "residuals", "coefficients", "statistics", "effects", "theta")


def _apply_random_effects(frame: Frame, over, eng: Optional[Engine], target: Expr, features: Sequence[Expr], entity, add_intercept: bool,
                          mode: str, null_policy: str):
    """compute_random_effects body: the group layout of _apply_static around Engine.random_effects; the id column moves with its rows."""
    y, xs, names, icpt, _ = _pre_process_data(frame, target, features, None, add_intercept)
    ids = _cluster_ids(frame, [entity], y)
    eng = eng or default_engine(y.device.index or 0 if _is_torch(y) else 0)
    grp = _Groups(eng, None if over is None else (frame[over] if isinstance(over, str) else over), y.shape[0])
    moved = grp.take([y] + list(xs) + ids)
    ys, xss, idss = moved[0], moved[1:1 + len(xs)], moved[1 + len(xs):]
    rows = {"predictions": "pred", "residuals": "resid", "effects": "effects", "theta": "theta"}
    want = {"coefficients": ("coef",),
            "statistics": ("coef", "status") + tuple(f for f in _lib.RANDOM_EFFECTS_FIELDS if f not in ("effects", "theta"))}.get(mode) or (rows[mode],)
    out = eng.random_effects(ys, xss, idss[0], grp.offsets, want=want, add_intercept=icpt, null_policy=null_policy)
    if mode == "statistics":
        return "statistics", RandomEffects(names, out, grp.keys)
    if mode == "coefficients":
        return "coefficients", Coefficients(names, out["coef"], grp.keys, grp.gid_frame(out["coef"]))
    return target.output_name, grp.untake(out[rows[mode]])


def _apply_dynamic(frame: Frame, over, eng: Optional[Engine], target: Expr, features: Sequence[Expr], sample_weights,
                   add_intercept: bool, mode: str, kind: str, kw):
    """compute_recursive_least_squares / compute_rolling_least_squares bodies (ls.py:332-409 around
    src/expressions.rs:593-701): the plugin gets sqrt_w-scaled, intercept-extended columns, a validity mask from the
    null policy, and zero-filled data (NullPolicy::Zero conversion, ex.rs:603,629,656,683).  All of that is done by the
    C-ABI entries themselves (csrc/dyn_prep.hip); this function only lays the groups out and hands the raw columns over."""
    y, xs, names, icpt, w = _pre_process_data(frame, target, features, sample_weights, add_intercept)
    n = y.shape[0]
    eng = eng or default_engine(y.device.index or 0 if _is_torch(y) else 0)
    policy = kw.null_policy
    grp = _Groups(eng, None if over is None else (frame[over] if isinstance(over, str) else over), n)
    moved = grp.take([y, w] + list(xs))                        # raw columns: everything else happens behind the C-ABI
    ys, ws, xss = moved[0], moved[1], moved[2:]
    want = ("coef",) if mode == "coefficients" else ("pred",)
    if kind == "rls":
        mean = kw.initial_state_mean if mode == "coefficients" else None      # quirk: ex.rs:636 passes None for predictions
        out = eng.recursive_least_squares(ys, xss, grp.offsets, weights=ws, add_intercept=icpt, want=want, half_life=kw.half_life,
                                          initial_state_covariance=kw.initial_state_covariance,
                                          initial_state_mean=mean, null_policy=policy)
    else:
        out = eng.rolling_least_squares(ys, xss, grp.offsets, weights=ws, add_intercept=icpt, want=want,
                                        window_size=kw.window_size, min_periods=kw.min_periods, use_woodbury=kw.use_woodbury,
                                        alpha=kw.alpha, null_policy=policy)
    res = grp.untake(out["coef"] if mode == "coefficients" else out["pred"])
    if mode == "coefficients":
        return "coefficients", Coefficients(names, res)
    return target.output_name, (y - res if mode == "residuals" else res)


# ---- the reference's module-level functions (least_squares.py:242-491) -------------------------------------------

_VALID_COV_TYPES = ("nonrobust", "HC0", "HC1", "HC2", "HC3", "HAC", "cluster")


def _cluster_ids(frame: Frame, groups, like) -> list:
    """The cluster id columns of cov_kwds["groups"] as int64 where ``like`` lives: names / expressions are read from the frame,
    arrays taken as they are; ids that are not integers are dictionary-encoded (their order is that of np.unique / torch.unique)."""
    out = []
    for g in groups:
        a = g if (_is_torch(g) or isinstance(g, np.ndarray)) else parse_into_expr(g)._column(frame)
        if a.shape[0] != like.shape[0]:
            raise ValueError(f"cov_kwds['groups']: {a.shape[0]} ids for {like.shape[0]} rows")
        if _is_torch(a):
            if a.dtype.is_floating_point or a.dtype.is_complex:
                a = torch.unique(a, return_inverse=True)[1]
            a = a.to(torch.int64)
            a = a.to(like.device) if _is_torch(like) else a.cpu().numpy()
        else:
            a = np.asarray(a)
            a = a.astype(np.int64) if a.dtype.kind in "iub" else np.unique(a, return_inverse=True)[1].astype(np.int64)
            if _is_torch(like):
                a = torch.as_tensor(a, device=like.device)
        out.append(a)
    return out


def _robust_cov(cov_type: str, cov_kwds: Optional[Dict[str, Any]], mode: str, kind: str = "ols"):
    """(cov_type, maxlags) of a robust request, ("cluster", id columns, use_correction) of a cluster-robust one, None for the default
    "nonrobust"; ValueError for what has no robust form: an unknown cov_type, a mode other than "statistics", multi-target / RLS /
    rolling models, HAC without cov_kwds={"maxlags": L}, "cluster" without cov_kwds={"groups": ...} or with other keys."""
    if cov_type not in _VALID_COV_TYPES:
        raise ValueError(f"'cov_type' must be one of {_VALID_COV_TYPES}, got {cov_type!r}")
    if cov_type == "nonrobust" and not cov_kwds:
        return None
    if kind != "ols":
        raise ValueError(f"cov_type / cov_kwds apply to single-target least squares in mode='statistics', not to {kind} models")
    if mode != "statistics":
        raise ValueError(f"cov_type={cov_type!r} needs mode='statistics' (got mode={mode!r})")
    kwds = dict(cov_kwds or {})
    if cov_type == "cluster":
        # statsmodels' spelling: cov_kwds={"groups": one id column or two (two-way), "use_correction": bool}
        if "maxlags" in kwds:
            raise ValueError("cov_kwds 'maxlags' applies to cov_type='HAC' only, not to 'cluster'")
        unknown = set(kwds) - {"groups", "use_correction"}
        if unknown:
            raise ValueError(f"unknown cov_kwds {sorted(unknown)} for cov_type='cluster' (groups, use_correction)")
        groups = kwds.get("groups")
        if groups is None:
            raise ValueError("cov_type='cluster' needs cov_kwds={'groups': <column name | Expr | array | [a, b]>}")
        groups = list(groups) if isinstance(groups, (list, tuple)) else [groups]
        if not 1 <= len(groups) <= 2:
            raise ValueError(f"cov_kwds['groups']: one or two id columns (got {len(groups)})")
        return "cluster", groups, bool(kwds.get("use_correction", True))
    unknown = set(kwds) - {"maxlags"}
    if unknown:
        raise ValueError(f"unknown cov_kwds {sorted(unknown)}")
    if cov_type == "HAC":
        lags = kwds.get("maxlags")
        if lags is None or isinstance(lags, bool) or int(lags) != lags or lags < 0:
            raise ValueError(f"cov_type='HAC' needs cov_kwds={{'maxlags': L}} with an integer L >= 0 (got {cov_kwds!r})")
        return cov_type, int(lags)
    if kwds:
        raise ValueError(f"cov_kwds {kwds} apply to cov_type='HAC' only")
    return cov_type, None


def compute_least_squares(target, *features, sample_weights=None, add_intercept: bool = False,
                          mode: str = "predictions", ols_kwargs: Optional[OLSKwargs] = None, cov_type: str = "nonrobust",
                          cov_kwds: Optional[Dict[str, Any]] = None, influence_kwds: Optional[Dict[str, Any]] = None) -> Expr:
    """``cov_type`` ("HC0" .. "HC3", "HAC" with ``cov_kwds={"maxlags": L}``) makes the standard errors, t- and p-values of
    mode="statistics" robust; the other fields do not depend on it.  mode="influence" (``influence_kwds={"level": 0.95,
    "fields": [...]}``) returns an ``Influence``: per-row diagnostics and prediction intervals in the frame's row order.  A group
    with df <= 0 has NaN rows there and does not raise, where mode="statistics" raises."""
    assert mode in _VALID_OUTPUT_MODES, f"'mode' must be one of {_VALID_OUTPUT_MODES}"
    kw = ols_kwargs or OLSKwargs()
    infl = _influence_request(mode, influence_kwds, "ols", kw, cov_type, cov_kwds)
    cov = None if infl is not None else _robust_cov(cov_type, cov_kwds, mode)
    t, fs = parse_into_expr(target), [parse_into_expr(f) for f in features]
    return Expr(t._name, fn=lambda frame, over, eng: _apply_static(frame, over, eng, t, fs, sample_weights, add_intercept, mode, kw, cov, infl))


def compute_ridge_cv(target, *features, alphas, sample_weights=None, add_intercept: bool = False, mode: str = "predictions",
                     null_policy: str = "ignore") -> Expr:
    """Ridge with the penalty chosen per group from ``alphas`` by closed-form leave-one-out error (scikit-learn's RidgeCV for every
    group of the frame in one call).  Modes "predictions", "residuals" and "coefficients" are those of the chosen candidate, as
    ``ridge(alpha=chosen)`` returns them; mode="cv" returns a ``RidgeCV`` with the choice and every candidate's score."""
    if mode not in _VALID_RIDGE_CV_MODES:
        raise ValueError(f"'mode' must be one of {_VALID_RIDGE_CV_MODES}, got {mode!r}")
    if null_policy not in _VALID_NULL_POLICIES:
        raise ValueError(f"'null_policy' must be one of {sorted(_VALID_NULL_POLICIES)}, got {null_policy!r}")
    grid = _ridge_cv_grid(alphas)
    t, fs = parse_into_expr(target), [parse_into_expr(f) for f in features]
    return Expr(t._name, fn=lambda frame, over, eng: _apply_ridge_cv(frame, over, eng, t, fs, sample_weights, add_intercept, mode, grid, null_policy))


def compute_elastic_net_cv(target, *features, alphas=None, n_alphas: int = 100, eps: float = 1e-3, l1_ratio: float = 0.5, n_folds: int = 5,
                           max_iter: int = 1000, tol: float = 1e-5, positive: bool = False, sample_weights=None,
                           add_intercept: bool = False, mode: str = "predictions", null_policy: str = "ignore") -> Expr:
    """Elastic net with the penalty chosen per group by K-fold cross-validation over a path (scikit-learn's ElasticNetCV /
    LassoCV with contiguous folds for every group of the frame in one call).  ``alphas`` None: every group gets its own grid of
    ``n_alphas`` values from its alpha_max down to ``eps`` times it.  Modes "predictions", "residuals" and "coefficients" are those
    of the chosen candidate fitted on all of the group's rows; mode="cv" returns an ``ElasticNetCV``."""
    if mode not in _VALID_ENET_CV_MODES:
        raise ValueError(f"'mode' must be one of {_VALID_ENET_CV_MODES}, got {mode!r}")
    if null_policy not in _VALID_NULL_POLICIES:
        raise ValueError(f"'null_policy' must be one of {sorted(_VALID_NULL_POLICIES)}, got {null_policy!r}")
    _, grid = _enet_cv_params(None, alphas, n_alphas, eps, l1_ratio, n_folds, max_iter, tol, positive)
    kw = dict(alphas=grid, n_alphas=n_alphas, eps=eps, l1_ratio=l1_ratio, n_folds=n_folds, max_iter=max_iter, tol=tol, positive=positive)
    t, fs = parse_into_expr(target), [parse_into_expr(f) for f in features]
    return Expr(t._name, fn=lambda frame, over, eng: _apply_enet_cv(frame, over, eng, t, fs, sample_weights, add_intercept, mode, null_policy, kw))


def compute_rlm(target, *features, norm: str = "huber", c: Optional[float] = None, max_iter: int = 50, tol: float = 1e-8,
                sample_weights=None, add_intercept: bool = False, mode: str = "predictions", null_policy: str = "ignore") -> Expr:
    """Huber / bisquare M-estimator regression per group (statsmodels' RLM with its MAD scale for every group of the frame in
    one call).  Modes "predictions", "residuals" and "coefficients" are those of the robust coefficients; mode="rlm" returns an
    ``RLM`` with the coefficients, scale, iteration count, status and the robust weights in frame order."""
    if mode not in _VALID_RLM_MODES:
        raise ValueError(f"'mode' must be one of {_VALID_RLM_MODES}, got {mode!r}")
    if null_policy not in _VALID_NULL_POLICIES:
        raise ValueError(f"'null_policy' must be one of {sorted(_VALID_NULL_POLICIES)}, got {null_policy!r}")
    _rlm_params(None, norm, c, max_iter, tol)
    t, fs = parse_into_expr(target), [parse_into_expr(f) for f in features]
    return Expr(t._name, fn=lambda frame, over, eng: _apply_rlm(frame, over, eng, t, fs, sample_weights, add_intercept, mode, norm, c,
                                                                max_iter, tol, null_policy))


def compute_glm(target, *features, family: str = "binomial", offset=None, max_iter: int = 25, tol: float = 1e-8, sample_weights=None,
                add_intercept: bool = False, mode: str = "predictions", null_policy: str = "ignore") -> Expr:
    """Logistic ("binomial") / Poisson regression per group with the canonical link (R's glm / statsmodels' GLM for every group of
    the frame in one call); ``offset`` is an optional column added to the linear predictor, ``sample_weights`` are prior weights.
    Mode "predictions" returns the fitted means, "residuals" y minus them, "coefficients" the coefficients; mode="glm" returns a
    ``GLM`` with the coefficients, standard errors, deviance, iteration count, status and the linear predictor in frame order."""
    if mode not in _VALID_GLM_MODES:
        raise ValueError(f"'mode' must be one of {_VALID_GLM_MODES}, got {mode!r}")
    if null_policy not in _VALID_NULL_POLICIES:
        raise ValueError(f"'null_policy' must be one of {sorted(_VALID_NULL_POLICIES)}, got {null_policy!r}")
    _glm_params(None, family, max_iter, tol)
    t, fs = parse_into_expr(target), [parse_into_expr(f) for f in features]
    return Expr(t._name, fn=lambda frame, over, eng: _apply_glm(frame, over, eng, t, fs, sample_weights, offset, add_intercept, mode,
                                                                family, max_iter, tol, null_policy))


def compute_iv2sls(target, *exog, endog, instruments, cov_type: str = "nonrobust", small_sample: bool = True, sample_weights=None,
                   add_intercept: bool = False, mode: str = "predictions", null_policy: str = "ignore") -> Expr:
    """Two-stage least squares per group (linearmodels' / statsmodels' IV2SLS for every group of the frame in one call): ``exog``
    are the exogenous regressors, ``endog`` the endogenous ones and ``instruments`` the excluded instruments (at least as many as
    ``endog``).  Modes "predictions" (x'b from the actual regressors), "residuals" and "coefficients" (exogenous, endogenous,
    const); mode="statistics" returns an ``IV2SLS`` with standard errors (``cov_type`` "nonrobust" / "HC0" / "HC1"), t and p
    values, the covariance matrix, the first-stage F and partial R2 of every endogenous regressor and Sargan's test."""
    if mode not in _VALID_IV_MODES:
        raise ValueError(f"'mode' must be one of {_VALID_IV_MODES}, got {mode!r}")
    if null_policy not in _VALID_NULL_POLICIES:
        raise ValueError(f"'null_policy' must be one of {sorted(_VALID_NULL_POLICIES)}, got {null_policy!r}")
    endog = [endog] if isinstance(endog, (str, Expr)) else list(endog)
    instruments = [instruments] if isinstance(instruments, (str, Expr)) else list(instruments)
    t, ex = parse_into_expr(target), [parse_into_expr(f) for f in exog]
    en, zs = [parse_into_expr(f) for f in endog], [parse_into_expr(f) for f in instruments]
    icpt = add_intercept and not any(f.output_name == "const" for f in ex + en)
    _iv_params(None, len(ex) + len(en), len(zs), len(en), cov_type, small_sample, icpt)
    return Expr(t._name, fn=lambda frame, over, eng: _apply_iv2sls(frame, over, eng, t, ex, en, zs, sample_weights, add_intercept, mode,
                                                                   cov_type, small_sample, null_policy))


def compute_glsar(target, *features, method: str = "prais_winsten", max_iter: int = 100, tol: float = 1e-6, add_intercept: bool = False,
                  mode: str = "predictions", null_policy: str = "ignore") -> Expr:
    """Regression with AR(1) errors per group by feasible GLS (statsmodels' GLSAR, Stata's prais / prais, corc for every group of the
    frame in one call): the rows of a group are its time series in frame order.  ``method``: "prais_winsten" or "cochrane_orcutt";
    ``max_iter`` / ``tol``: the updates of rho at the most and the stop rule (``max_iter=1``: the two-step estimator).  Modes
    "predictions" (x'b on the original scale), "residuals" and "coefficients"; mode="statistics" returns a ``GLSAR`` with rho, standard
    errors, t and p values, the covariance matrix and the Durbin-Watson statistics before and after.  ``null_policy``: "ignore" or
    "zero"."""
    if mode not in _VALID_GLSAR_MODES:
        raise ValueError(f"'mode' must be one of {_VALID_GLSAR_MODES}, got {mode!r}")
    if null_policy not in ("ignore", "zero"):
        raise ValueError(f"glsar: 'null_policy' must be 'ignore' or 'zero' (the drop family is not built), got {null_policy!r}")
    _glsar_params(None, method, max_iter, tol)
    t, fs = parse_into_expr(target), [parse_into_expr(f) for f in features]
    return Expr(t._name, fn=lambda frame, over, eng: _apply_glsar(frame, over, eng, t, fs, add_intercept, mode, method, max_iter, tol,
                                                                  null_policy))


def compute_absorbed_least_squares(target, *features, absorb, cov_type: str = "nonrobust", sample_weights=None,
                                   add_intercept: bool = False, mode: str = "predictions", null_policy: str = "ignore",
                                   max_iter: Optional[int] = None, tol: Optional[float] = None) -> Expr:
    """Regression per group that absorbs one categorical effect (the "within" estimator: ``areg``, ``xtreg, fe``,
    ``PanelOLS(entity_effects=True)``) without a dummy column per category.  ``absorb``: the id column (a name, an expression or an
    array; under ``.over(key)`` it moves with its rows).  Modes "predictions" (x'b plus the row's effect), "residuals",
    "coefficients" (the slopes; with ``add_intercept`` the mean effect last) and "effects" (the row's effect, centred on the mean
    effect with ``add_intercept``); mode="statistics" returns an ``AbsorbedOLS`` with standard errors (``cov_type`` "nonrobust" or
    "cluster", clustered on the absorbed id), t and p values, sigma2, the within and overall R2 and the category counts.
    ``absorb`` may also be a list or tuple of TWO columns: two-way fixed effects (``reghdfe y x, absorb(firm year)``) by alternating
    projections, ``max_iter`` sweeps per column at the most (default 10 000) with stop rule ``tol`` (default 1e-10); "cluster" then
    clusters on the first column, mode "effects" returns a dict of both effects keyed by the two columns, and the statistics also
    carry ``n_categories2 n_components n_iter``.  ``max_iter`` / ``tol`` do not apply to a single column."""
    if mode not in _VALID_ABSORB_MODES:
        raise ValueError(f"'mode' must be one of {_VALID_ABSORB_MODES}, got {mode!r}")
    if null_policy not in _VALID_NULL_POLICIES:
        raise ValueError(f"'null_policy' must be one of {sorted(_VALID_NULL_POLICIES)}, got {null_policy!r}")
    if absorb is None:
        raise ValueError("'absorb' names the id column whose effect is absorbed")
    t, fs = parse_into_expr(target), [parse_into_expr(f) for f in features]
    icpt = add_intercept and not any(f.output_name == "const" for f in fs)
    two_way = None
    if isinstance(absorb, (list, tuple)):
        if len(absorb) == 1:
            absorb = absorb[0]
        elif len(absorb) == 2:
            two_way = (10_000 if max_iter is None else max_iter, 1e-10 if tol is None else tol)
        else:
            raise ValueError(f"'absorb' takes one id column or two, got {len(absorb)} (three or more absorbed effects are not built)")
    if two_way is None:
        if max_iter is not None or tol is not None:
            raise ValueError("'max_iter' / 'tol' belong to the two-way iteration: a single absorbed column has a closed form")
        _absorb_params(None, len(fs), cov_type, icpt)
    else:
        _absorb2_params(None, len(fs), cov_type, icpt, *two_way)
    return Expr(t._name, fn=lambda frame, over, eng: _apply_absorb(frame, over, eng, t, fs, absorb, sample_weights, add_intercept, mode,
                                                                   cov_type, null_policy, two_way))


def compute_random_effects(target, *features, entity, sample_weights=None, add_intercept: bool = False, mode: str = "predictions",
                           null_policy: str = "ignore") -> Expr:
    """Random-effects panel regression per group (Stata's ``xtreg, re`` followed by ``hausman``, linearmodels' ``RandomEffects``):
    feasible GLS with Swamy-Arora variance components, closed form.  ``entity``: the id column of the panel's entities (a name, an
    expression or an array; under ``.over(key)`` it moves with its rows).  Modes "predictions" (z'b, no effect added), "residuals",
    "coefficients", "effects" (the row's predicted effect u_c) and "theta" (the row's quasi-demeaning factor); mode="statistics"
    returns a ``RandomEffects`` with standard errors, t and p values, the between and within coefficients, sigma2_e, sigma2_u, rho,
    the Hausman statistic with its p-value and the counts.  ``sample_weights`` are not built and raise."""
    if mode not in _VALID_RANDOM_EFFECTS_MODES:
        raise ValueError(f"'mode' must be one of {_VALID_RANDOM_EFFECTS_MODES}, got {mode!r}")
    if null_policy not in _VALID_NULL_POLICIES:
        raise ValueError(f"'null_policy' must be one of {sorted(_VALID_NULL_POLICIES)}, got {null_policy!r}")
    if entity is None:
        raise ValueError("'entity' names the id column of the panel's entities")
    t, fs = parse_into_expr(target), [parse_into_expr(f) for f in features]
    icpt = add_intercept and not any(f.output_name == "const" for f in fs)
    _random_effects_params(None, len(fs), icpt, sample_weights)
    return Expr(t._name, fn=lambda frame, over, eng: _apply_random_effects(frame, over, eng, t, fs, entity, add_intercept, mode, null_policy))


def compute_multi_target_least_squares(targets, *features, sample_weights=None, add_intercept: bool = False,
                                       mode: str = "predictions", ols_kwargs: Optional[OLSKwargs] = None) -> Expr:
    """Several targets regressed on the same features (least_squares.py:282-328, src/expressions.rs:521-591).  ``targets``
    is the list of target columns (the fields of the reference's struct); the result is a dict target -> column.

    A row is valid only if EVERY target (and, for the drop policies, every feature) is non-null (compute_is_valid_mask
    with m targets, ex.rs:539), so the joint mask is applied to all targets first and each one is then solved by the
    engine's multi-target entry: one Gram pass over [X | targets] and one factorisation shared by all targets -- what
    solve_multi_target (ls.rs:243-260) does with one SVD."""
    kw = ols_kwargs or OLSKwargs()
    _influence_request(mode, None, "multi-target")
    msg = "Consider running multiple independent regressions on a multi-expression target!"
    assert not kw.positive and (kw.l1_ratio is None or kw.l1_ratio == 0.0), (
        "Multi-target regression is only supported for unconstrained OLS & Ridge problems." + msg)
    assert kw.solve_method in {"svd", None}, "only solve_method='svd' is supported for multi-target regressions"
    if mode not in ("predictions", "residuals"):
        raise NotImplementedError("Only mode={'predictions', 'residuals'} is currently supported. " + msg)
    if isinstance(targets, Expr) and getattr(targets, "_fields", None):
        targets = targets._fields
    elif isinstance(targets, (str, Expr)):
        targets = [targets]
    ts, fs = [parse_into_expr(t) for t in targets], [parse_into_expr(f) for f in features]

    def run(frame: Frame, over, eng):
        y0, xs, names, icpt, w = _pre_process_data(frame, ts[0], fs, sample_weights, add_intercept)
        ys = [y0] + [t._column(frame) for t in ts[1:]]
        n = y0.shape[0]
        eng = eng or default_engine(y0.device.index or 0 if _is_torch(y0) else 0)
        grp = _Groups(eng, None if over is None else (frame[over] if isinstance(over, str) else over), n)
        offs = grp.offsets
        moved = grp.take([w] + list(ys) + list(xs))
        w_s, ys_s, xs_s = moved[0], moved[1:1 + len(ys)], moved[1 + len(ys):]
        # joint validity mask, fit on the rows it leaves, every row predicted from zero-filled features, "drop" masked
        # (ex.rs:539-585): all of it inside the entry (csrc/dyn_prep.hip).  A Polars caller reads null_count off its Series; here the
        # columns are arrays, so the null count is one reduction per column -- cheap next to the compaction pass (every column read
        # AND rewritten) that the entry runs whenever it cannot be promised a null-free frame.
        null_free = not any(_has_nan(c) for c in list(ys_s) + list(xs_s) + ([w_s] if w_s is not None else []))
        preds = eng.multi_target_least_squares(ys_s, xs_s, offs, weights=w_s, add_intercept=icpt, want=("pred",), alpha=kw.alpha,
                                               solve_method=kw.solve_method, rcond=kw.rcond, null_policy=kw.null_policy,
                                               null_free=null_free)["pred"]
        out = {}
        for t, y_s, pr in zip(ts, ys_s, preds):
            val = pr if mode == "predictions" else y_s - pr
            out[t.output_name] = grp.untake(val)
        return "predictions", out

    return Expr(ts[0]._name, fn=run)


def compute_recursive_least_squares(target, *features, sample_weights=None, add_intercept: bool = False,
                                    mode: str = "predictions", rls_kwargs: Optional[RLSKwargs] = None) -> Expr:
    _influence_request(mode, None, "rls")
    valid_output_modes = _VALID_OUTPUT_MODES - {"statistics", "influence"}
    assert mode in valid_output_modes, f"'mode' must be one of {valid_output_modes}"
    kw = rls_kwargs or RLSKwargs()
    t, fs = parse_into_expr(target), [parse_into_expr(f) for f in features]
    return Expr(t._name, fn=lambda frame, over, eng: _apply_dynamic(frame, over, eng, t, fs, sample_weights, add_intercept, mode, "rls", kw))


def compute_rolling_least_squares(target, *features, sample_weights=None, add_intercept: bool = False,
                                  mode: str = "predictions", rolling_kwargs: Optional[RollingKwargs] = None) -> Expr:
    _influence_request(mode, None, "rolling")
    valid_output_modes = _VALID_OUTPUT_MODES - {"statistics", "influence"}
    assert mode in valid_output_modes, f"'mode' must be one of {valid_output_modes}"
    kw = rolling_kwargs or RollingKwargs()
    t, fs = parse_into_expr(target), [parse_into_expr(f) for f in features]
    return Expr(t._name, fn=lambda frame, over, eng: _apply_dynamic(frame, over, eng, t, fs, sample_weights, add_intercept, mode, "rolling", kw))


_FORMULA_TOKEN = re.compile(r"\s*(?:(?P<name>[A-Za-z_][A-Za-z_0-9.]*)|(?P<num>\d+)|(?P<op>[+\-:*]))")


def _formula_terms(side: str) -> List[Tuple[str, ...]]:
    """One side of a patsy formula -> its term list in written order, each term a tuple of factor (column) names; the
    intercept is the empty tuple.  Grammar (patsy's operators on plain columns): ``+`` adds terms, ``-`` removes them,
    ``a:b`` is the interaction (product column), ``a*b`` = ``a + b + a:b``, ``1`` / ``0`` add / remove the intercept.
    Anything else patsy understands (function calls like ``log(x)`` / ``C(g)`` / ``I(..)``, parentheses, ``**``, ``/``,
    ``%in%``) raises NotImplementedError: the reference supports column-only formulas too (utils.py:66-72, 96-100)."""
    toks: List[Tuple[str, str]] = []
    pos = 0
    side = side.rstrip()
    while pos < len(side):
        m = _FORMULA_TOKEN.match(side, pos)
        if not m:
            raise NotImplementedError(f"formula syntax not supported at {side[pos:].strip()[:12]!r}: only column names joined by + - : * (and 0 / 1)")
        kind = m.lastgroup
        toks.append((kind, m.group(kind)))
        pos = m.end()
    i = 0

    def atom() -> List[Tuple[str, ...]]:
        nonlocal i
        if i >= len(toks) or toks[i][0] == "op":
            raise ValueError("formula: expected a column name")
        kind, v = toks[i]
        i += 1
        if kind == "num":
            if v not in ("0", "1"):
                raise NotImplementedError(f"formula: numeric term {v!r} (only 0 and 1 carry a meaning)")
            return [("<0>",)] if v == "0" else [()]
        return [(v,)]

    def interaction() -> List[Tuple[str, ...]]:
        nonlocal i
        left = atom()
        while i < len(toks) and toks[i] == ("op", ":"):
            i += 1
            right = atom()
            if left[0] in ((), ("<0>",)) or right[0] in ((), ("<0>",)):
                raise ValueError("formula: the intercept cannot take part in an interaction")
            left = [left[0] + tuple(f for f in right[0] if f not in left[0])]
        return left

    def product() -> List[Tuple[str, ...]]:
        nonlocal i
        left = interaction()
        while i < len(toks) and toks[i] == ("op", "*"):
            i += 1
            right = interaction()
            if any(t in ((), ("<0>",)) for t in left + right):
                raise ValueError("formula: the intercept cannot take part in an interaction")
            left = left + right + [a + tuple(f for f in b if f not in a) for a in left for b in right]
        return left

    terms: List[Tuple[str, ...]] = [()]                        # patsy starts every RHS with the intercept
    sign = "+"
    if toks and toks[0] in (("op", "+"), ("op", "-")):
        sign = toks[0][1]
        i = 1
    while True:
        for t in product():
            if t == ("<0>",):                                  # "+ 0" removes the intercept, "- 0" adds it
                t, add = (), sign == "-"
            else:
                add = sign == "+"
            if add and t not in terms:
                terms.append(t)
            elif not add and t in terms:
                terms.remove(t)
        if i >= len(toks):
            break
        if toks[i] not in (("op", "+"), ("op", "-")):
            raise ValueError(f"formula: unexpected {toks[i][1]!r}")
        sign = toks[i][1]
        i += 1
    return terms


def _term_expr(term: Tuple[str, ...]) -> Expr:
    """utils.py:101-106: one factor -> the column; several -> their product, named ``a:b``."""
    return col(term[0]) if len(term) == 1 else Expr(term[0], factors=term[1:], alias=":".join(term))


def _parse_formula(formula: str, include_dependent_variable: bool) -> Tuple[List[Expr], bool]:
    """build_expressions_from_patsy_formula (utils.py:61-108) without patsy (absent here): same term lists for formulas over
    plain columns (``y ~ x1 + x2:x3 - 1``), NotImplementedError for the rest.  The intercept flag follows the reference's
    rule TO THE LETTER: ``add_intercept = "-1" not in formula`` (utils.py:94) -- a literal substring test, so ``"x1 + x2 -1"``
    drops the intercept while ``"x1 + x2 - 1"`` (with a space) and ``"x1 + x2 + 0"`` keep it, whatever patsy's own reading."""
    if "(" in formula or ")" in formula:
        raise NotImplementedError("formula: function calls / categories / parentheses are not supported (utils.py:66-72, 96-100)")
    if "**" in formula:
        raise NotImplementedError("formula: '**' is not supported")
    parts = formula.split("~")
    if len(parts) > 2:
        raise ValueError("formula: more than one '~'")
    lhs, rhs = (parts[0], parts[1]) if len(parts) == 2 else ("", parts[0])
    lhs_terms = [t for t in _formula_terms(lhs) if t != ()] if lhs.strip() else []
    rhs_terms = [t for t in _formula_terms(rhs) if t != ()]    # the intercept term has no factors: skipped (utils.py:101-106)
    if include_dependent_variable:
        assert len(lhs_terms) == 1, "must provide exactly one LHS variable"
    else:
        assert len(lhs_terms) == 0, "can not provide LHS variables in this context"
    add_intercept = "-1" not in formula
    return [_term_expr(t) for t in lhs_terms + rhs_terms], add_intercept


def compute_least_squares_from_formula(formula: str, sample_weights=None, mode: str = "predictions", cov_type: str = "nonrobust",
                                       cov_kwds: Optional[Dict[str, Any]] = None, influence_kwds: Optional[Dict[str, Any]] = None,
                                       **kwargs) -> Expr:
    exprs, add_intercept = _parse_formula(formula, include_dependent_variable=True)   # ls.py:432-452
    kind = "rls" if kwargs.get("half_life") else ("rolling" if kwargs.get("window_size") else "ols")
    if _influence_request(mode, influence_kwds, kind, None, cov_type, cov_kwds) is None:
        _robust_cov(cov_type, cov_kwds, mode, kind)
    if kwargs.get("half_life"):
        return compute_recursive_least_squares(exprs[0], *exprs[1:], add_intercept=add_intercept, sample_weights=sample_weights,
                                               mode=mode, rls_kwargs=RLSKwargs(**kwargs))
    if kwargs.get("window_size"):
        return compute_rolling_least_squares(exprs[0], *exprs[1:], add_intercept=add_intercept, sample_weights=sample_weights,
                                             mode=mode, rolling_kwargs=RollingKwargs(**kwargs))
    return compute_least_squares(exprs[0], *exprs[1:], add_intercept=add_intercept, sample_weights=sample_weights, mode=mode,
                                 ols_kwargs=OLSKwargs(**kwargs), cov_type=cov_type, cov_kwds=cov_kwds, influence_kwds=influence_kwds)


def predict(coefficients: Coefficients, *features, frame: Frame, null_policy: str = "zero", add_intercept: bool = False,
            name: Optional[str] = None, engine: Optional[Engine] = None):
    """least_squares.py:455-491 + src/expressions.rs:706-741: row-wise features . coefficients."""
    assert null_policy in _VALID_NULL_POLICIES, "'null_policy' must be one of {drop, ignore, zero}"
    fs = [parse_into_expr(f) for f in features]
    xs = [f._column(frame) for f in fs]
    if add_intercept and any(f.output_name == "const" for f in fs):
        logger.warning("feature named 'const' already detected, assuming it is the intercept")
        add_intercept = False
    rows = coefficients.to_rows()
    assert rows.shape[1] == len(xs) + int(add_intercept), "number of coefficients must match number of features!"  # ex.rs:717-721
    eng = engine or default_engine((xs[0].device.index or 0) if _is_torch(xs[0]) else 0)   # the engine of the columns' device
    # the zero fill of "zero" and the masking of "drop" are the plugin body's (ex.rs:725, :732-738): done by the kernel
    return eng.predict(xs, rows, add_intercept=add_intercept, null_policy=null_policy)


# ---- the `least_squares` namespace (polars_ols/__init__.py:35-295) -----------------------------------------------

class LeastSquares:
    def __init__(self, expr: Expr):
        self._expr = expr

    def least_squares(self, *features, sample_weights=None, add_intercept: bool = False, mode: str = "predictions",
                      null_policy: str = "ignore", solve_method: Optional[str] = None, multi_target: bool = False,
                      cov_type: str = "nonrobust", cov_kwds: Optional[Dict[str, Any]] = None,
                      influence_kwds: Optional[Dict[str, Any]] = None, **ols_kwargs) -> Expr:
        kw = OLSKwargs(null_policy=null_policy, solve_method=solve_method, **ols_kwargs)
        if multi_target:
            _influence_request(mode, influence_kwds, "multi-target")
            _robust_cov(cov_type, cov_kwds, mode, "multi-target")
            return compute_multi_target_least_squares(self._expr, *features, sample_weights=sample_weights, add_intercept=add_intercept,
                                                      mode=mode, ols_kwargs=kw)
        return compute_least_squares(self._expr, *features, sample_weights=sample_weights, add_intercept=add_intercept, mode=mode,
                                     ols_kwargs=kw, cov_type=cov_type, cov_kwds=cov_kwds, influence_kwds=influence_kwds)

    def ols(self, *features, **kwargs) -> Expr:
        return self.least_squares(*features, **kwargs)

    def multi_target_ols(self, *features, **kwargs) -> Expr:
        return self.least_squares(*features, multi_target=True, **kwargs)

    def wls(self, *features, sample_weights, **kwargs) -> Expr:
        return self.least_squares(*features, sample_weights=sample_weights, **kwargs)

    def ridge(self, *features, alpha: float, **kwargs) -> Expr:
        return self.least_squares(*features, alpha=alpha, l1_ratio=0.0, **kwargs)

    def ridge_cv(self, *features, alphas, sample_weights=None, add_intercept: bool = False, mode: str = "predictions",
                 null_policy: str = "ignore") -> Expr:
        return compute_ridge_cv(self._expr, *features, alphas=alphas, sample_weights=sample_weights, add_intercept=add_intercept,
                                mode=mode, null_policy=null_policy)

    def elastic_net_cv(self, *features, alphas=None, n_alphas: int = 100, eps: float = 1e-3, l1_ratio: float = 0.5, n_folds: int = 5,
                       max_iter: int = 1000, tol: float = 1e-5, positive: bool = False, sample_weights=None,
                       add_intercept: bool = False, mode: str = "predictions", null_policy: str = "ignore") -> Expr:
        return compute_elastic_net_cv(self._expr, *features, alphas=alphas, n_alphas=n_alphas, eps=eps, l1_ratio=l1_ratio,
                                      n_folds=n_folds, max_iter=max_iter, tol=tol, positive=positive, sample_weights=sample_weights,
                                      add_intercept=add_intercept, mode=mode, null_policy=null_policy)

    def lasso_cv(self, *features, **kwargs) -> Expr:
        """elastic_net_cv with l1_ratio = 1"""
        if kwargs.get("l1_ratio", 1.0) != 1.0:
            raise ValueError("lasso_cv: l1_ratio is fixed at 1; use elastic_net_cv")
        kwargs["l1_ratio"] = 1.0
        return self.elastic_net_cv(*features, **kwargs)

    def glsar(self, *features, method: str = "prais_winsten", max_iter: int = 100, tol: float = 1e-6, add_intercept: bool = False,
              mode: str = "predictions", null_policy: str = "ignore") -> Expr:
        return compute_glsar(self._expr, *features, method=method, max_iter=max_iter, tol=tol, add_intercept=add_intercept, mode=mode,
                             null_policy=null_policy)

    def rlm(self, *features, norm: str = "huber", c: Optional[float] = None, max_iter: int = 50, tol: float = 1e-8,
            sample_weights=None, add_intercept: bool = False, mode: str = "predictions", null_policy: str = "ignore") -> Expr:
        return compute_rlm(self._expr, *features, norm=norm, c=c, max_iter=max_iter, tol=tol, sample_weights=sample_weights,
                           add_intercept=add_intercept, mode=mode, null_policy=null_policy)

    def glm(self, *features, family: str = "binomial", offset=None, max_iter: int = 25, tol: float = 1e-8, sample_weights=None,
            add_intercept: bool = False, mode: str = "predictions", null_policy: str = "ignore") -> Expr:
        return compute_glm(self._expr, *features, family=family, offset=offset, max_iter=max_iter, tol=tol,
                           sample_weights=sample_weights, add_intercept=add_intercept, mode=mode, null_policy=null_policy)

    def iv2sls(self, *exog, endog, instruments, cov_type: str = "nonrobust", small_sample: bool = True, sample_weights=None,
               add_intercept: bool = False, mode: str = "predictions", null_policy: str = "ignore") -> Expr:
        return compute_iv2sls(self._expr, *exog, endog=endog, instruments=instruments, cov_type=cov_type, small_sample=small_sample,
                              sample_weights=sample_weights, add_intercept=add_intercept, mode=mode, null_policy=null_policy)

    def absorb(self, *features, absorb, cov_type: str = "nonrobust", sample_weights=None, add_intercept: bool = False,
               mode: str = "predictions", null_policy: str = "ignore", max_iter: Optional[int] = None,
               tol: Optional[float] = None) -> Expr:
        return compute_absorbed_least_squares(self._expr, *features, absorb=absorb, cov_type=cov_type, sample_weights=sample_weights,
                                              add_intercept=add_intercept, mode=mode, null_policy=null_policy, max_iter=max_iter, tol=tol)

    def random_effects(self, *features, entity=None, sample_weights=None, add_intercept: bool = False, mode: str = "predictions",
                       null_policy: str = "ignore") -> Expr:
        return compute_random_effects(self._expr, *features, entity=entity, sample_weights=sample_weights, add_intercept=add_intercept,
                                      mode=mode, null_policy=null_policy)

    def lasso(self, *features, alpha: float, **kwargs) -> Expr:
        return self.least_squares(*features, alpha=alpha, l1_ratio=1.0, **kwargs)

    def elastic_net(self, *features, alpha: float, l1_ratio: float = 0.5, positive: bool = False, **kwargs) -> Expr:
        return self.least_squares(*features, alpha=alpha, l1_ratio=l1_ratio, positive=positive, **kwargs)

    def rls(self, *features, sample_weights=None, add_intercept: bool = False, mode: str = "predictions",
            null_policy: str = "drop", half_life: Optional[float] = None, initial_state_covariance: Optional[float] = 10.0,
            initial_state_mean=None) -> Expr:
        return compute_recursive_least_squares(
            self._expr, *features, sample_weights=sample_weights, add_intercept=add_intercept, mode=mode,
            rls_kwargs=RLSKwargs(null_policy=null_policy, half_life=half_life, initial_state_mean=initial_state_mean,
                                 initial_state_covariance=initial_state_covariance))

    def rolling_ols(self, *features, window_size: int, sample_weights=None, add_intercept: bool = False,
                    mode: str = "predictions", null_policy: str = "drop", min_periods: Optional[int] = None,
                    use_woodbury: Optional[bool] = None, alpha: Optional[float] = None) -> Expr:
        return compute_rolling_least_squares(
            self._expr, *features, sample_weights=sample_weights, add_intercept=add_intercept, mode=mode,
            rolling_kwargs=RollingKwargs(window_size=window_size, min_periods=min_periods, use_woodbury=use_woodbury,
                                         alpha=alpha, null_policy=null_policy))

    def expanding_ols(self, *features, **kwargs) -> Expr:
        return self.rls(*features, half_life=None, **kwargs)

    def from_formula(self, formula: str, **kwargs) -> Expr:
        features, add_intercept = _parse_formula(formula, include_dependent_variable=False)
        if kwargs.get("half_life") or kwargs.get("window_size"):
            _influence_request(kwargs.get("mode", "predictions"), kwargs.pop("influence_kwds", None),
                               "rls" if kwargs.get("half_life") else "rolling")
            _robust_cov(kwargs.pop("cov_type", "nonrobust"), kwargs.pop("cov_kwds", None), kwargs.get("mode", "predictions"),
                        "rls" if kwargs.get("half_life") else "rolling")
        if kwargs.get("half_life"):
            return self.rls(*features, add_intercept=add_intercept, **kwargs)
        if kwargs.get("window_size"):
            return self.rolling_ols(*features, add_intercept=add_intercept, **kwargs)
        return self.least_squares(*features, add_intercept=add_intercept, **kwargs)

    def predict(self, *features, name: Optional[str] = None, add_intercept: bool = False, null_policy: str = "zero") -> Expr:
        """``pl.col("coefficients").least_squares.predict(x1, x2)`` (__init__.py:274-287): the namespace's column is a
        coefficients struct (a ``Coefficients`` held in the frame, e.g. by ``with_columns(... mode="coefficients")``)."""
        assert null_policy in _VALID_NULL_POLICIES, "'null_policy' must be one of {drop, ignore, zero}"
        src = self._expr

        def run(frame: Frame, over, eng):
            coefficients = frame[src._name]
            if not isinstance(coefficients, Coefficients):
                raise TypeError(f"column '{src._name}' does not hold a coefficients struct")
            return name or "predictions", predict(coefficients, *features, frame=frame, null_policy=null_policy,
                                                  add_intercept=add_intercept, engine=eng)

        return Expr(src._name, fn=run, alias=name or "predictions")

    def predict_from_formula(self, formula: str, name: Optional[str] = None) -> Expr:  # __init__.py:289-295
        features, add_intercept = _parse_formula(formula, include_dependent_variable=False)
        has_const = any(f.output_name == "const" for f in features)
        return self.predict(*features, name=name, add_intercept=add_intercept and not has_const)
