"""Frames, route predictions, oracles and the guarded-call runner shared by test_extent_gpu.py and test_isolation_gpu.py.

Frames are small (a few thousand rows, a handful of groups), ragged, with odd group lengths and an odd row count: group heads sit off
the 16-byte grid of both dtypes and the last 16-byte chunk of every column crosses its end."""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional

import numpy as np

from arena import Frame, bits

STATIC_KT = (1, 6, 8, 10, 12, 17, 24, 31)
STATIC_BASE = (40, 200, 500, 1000, 1900, 3000, 120)          # seven groups: an odd number of odd lengths is an odd row count
GROUP_STATUS = (0, 1, 2, 3, 4)                               # pols_group_status


def tol_of(dtype) -> float:
    """the project's tolerances (atol = rtol): 1e-4 for f32 batches, 1e-6 for f64"""
    return 1e-4 if np.dtype(dtype) == np.float32 else 1e-6


def dt_name(dtype) -> str:
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


def offsets_of(sizes) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def odd_total(sizes) -> list:
    """odd lengths (>= the given ones) and a row count that is no multiple of 2: the last vector of a column crosses its end"""
    sizes = [int(s) | 1 for s in sizes]
    if sum(sizes) % 2 == 0:
        sizes[-1] += 1                                       # (an even number of groups: one even length)
    return sizes


def ragged_sizes(rng, kt: int, base=STATIC_BASE) -> list:
    return odd_total([max(kt + 3, b - int(rng.integers(0, b // 8 + 1))) for b in base])


def static_data(seed: int, dtype, kt: int, weights: bool, policy: str, sizes=None, nan_frac: float = 0.02) -> Dict:
    """kt Gaussian features, y = their sum + noise, optional weights in [0.5, 2]; under the drop policies 2 % of the targets are NaN"""
    rng = np.random.default_rng(seed)
    offs = offsets_of(ragged_sizes(rng, kt) if sizes is None else sizes)
    n = int(offs[-1])
    cols = [rng.standard_normal(n).astype(dtype) for _ in range(kt)]
    y = (sum(c.astype(np.float64) for c in cols) + 0.1 * rng.standard_normal(n)).astype(dtype)
    if policy != "ignore" and nan_frac > 0:
        y[rng.random(n) < nan_frac] = np.nan
    w = rng.uniform(0.5, 2.0, n).astype(dtype) if weights else None
    return {"y": y, "cols": cols, "offs": offs, "w": w}


def frame_of(d: Dict, **kw) -> Frame:
    return Frame(d["y"], d["cols"], d["offs"], w=d.get("w"), valid=d.get("valid"), extra=d.get("extra"), **kw)


# ---------------------------------------------------------------------------------------------------------------- the guarded call

def flatten(res: Dict) -> Dict:
    out = {}
    for k, v in res.items():
        if isinstance(v, (list, tuple)):
            for i, t in enumerate(v):
                out[f"{k}[{i}]"] = t
        else:
            out[k] = v
    return out


def host(v) -> np.ndarray:
    return np.array(v.detach().cpu().numpy() if hasattr(v, "detach") else v, copy=True)


def guarded(eng, what: str, call: Callable[[], Dict], fresh: bool = True):
    """One call with guarded outputs: the allocator's arenas re-armed, the call made, guards and coverage checked.  Returns the
    outputs as host arrays (lists flattened to ``key[i]``) and the kernel name."""
    eng.arena.begin(fresh=fresh)
    res = flatten(call())
    eng.synchronize()
    name = eng.last_kernel
    eng.arena.check(what)
    return {k: host(v) for k, v in res.items()}, name


def assert_same_bits(a: Dict, b: Dict, what: str, rows: Optional[Dict] = None) -> None:
    """every output of two calls bit-equal (``rows[key]``: only those rows / groups of that output)"""
    assert a.keys() == b.keys()
    for k in a:
        x, y = bits(a[k]), bits(b[k])
        if rows is not None:
            x, y = x[rows[k]], y[rows[k]]
        if not np.array_equal(x, y):
            idx = np.argwhere(x != y)
            raise AssertionError(f"{what}: '{k}' differs in {len(idx)} of {x.size} elements, first at {idx[:5].tolist()}")


def twice(eng, frame: Frame, what: str, call: Callable[[], Dict]):
    """The same frame and the same guarded outputs, the input guards NaN in one call and 7.0 in the other: the two results are
    bit-equal -- nothing outside a column's extent was used -- and each call kept to its outputs' extents and wrote all of them."""
    frame.guards(np.nan)
    a, name_a = guarded(eng, f"{what} [NaN guards]", call, fresh=True)
    frame.guards(7.0)
    b, name_b = guarded(eng, f"{what} [7.0 guards]", call, fresh=False)
    assert name_a == name_b, (what, name_a, name_b)
    assert_same_bits(a, b, f"{what} [{name_a}]: NaN against 7.0 in the input guards")
    return a, name_a


def close(got, ref, tol: float, what: str) -> None:
    """atol = rtol = tol; NaN where and only where the oracle has NaN"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaN pattern", np.argwhere(np.isnan(got) != np.isnan(ref))[:5].tolist())
    ok = np.isclose(got, ref, rtol=tol, atol=tol, equal_nan=True)
    if not ok.all():
        with np.errstate(all="ignore"):
            err = np.abs(got - ref) / (tol + tol * np.abs(ref))
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} outside atol = rtol = {tol:g}; worst error / bound {np.nanmax(err):.3g} "
                             f"at {np.unravel_index(int(np.nanargmax(err)), err.shape)}")


class Replay:
    """Stands in for an Engine in the checkers of test_ridge_cv_gpu / test_enet_cv_gpu, which make the call themselves: hands them
    the outputs a guarded call already produced."""

    def __init__(self, got: Dict, kernel: str):
        self._got, self.last_kernel = got, kernel

    def ridge_cv(self, *a, **kw):
        return self._got

    elastic_net_cv = ridge_cv

    def synchronize(self):
        pass


# ---------------------------------------------------------------------------------------------------------------- poisoned neighbours

POISONS = ("+inf", "-inf", "huge", "scale", "nan")


def every_other(offs):
    """(poisoned groups, clean groups, clean rows): groups 1, 3, 5, .. are poisoned"""
    G = len(offs) - 1
    bad = np.arange(1, G, 2)
    clean = np.setdiff1d(np.arange(G), bad)
    rows = np.zeros(int(offs[-1]), dtype=bool)
    for g in clean:
        rows[offs[g]:offs[g + 1]] = True
    return bad, clean, rows


def poisoned(columns, offs, bad, kind: str):
    """copies of ``columns`` (float arrays of n_rows values) with the rows of the groups ``bad`` overwritten: +-Inf, a huge finite
    value (1e30 for f32, 1e300 for f64), the rows scaled by 2^60, or NaN.  A value that is already NaN -- a null target of the drop
    policies' frames -- stays one under the other poisons: they are "not nulls", and turning a neighbour's nulls into rows would move the
    clean groups' rows inside the compacted frame of the gathered rolling kernel, whose prefix sums round by position."""
    out = []
    for c in columns:
        c = np.array(c, copy=True)
        huge = 1e30 if c.dtype == np.float32 else 1e300
        for g in bad:
            s, e = int(offs[g]), int(offs[g + 1])
            if kind == "scale":
                c[s:e] *= c.dtype.type(2.0 ** 60)
            elif kind == "nan":
                c[s:e] = np.nan
            else:
                c[s:e] = np.where(np.isnan(c[s:e]), c[s:e], c.dtype.type({"+inf": np.inf, "-inf": -np.inf, "huge": huge}[kind]))
        out.append(c)
    return out


def isolation(eng, fr: Frame, d: Dict, what: str, call: Callable[[], Dict], rows_of: Callable[[str, np.ndarray], object],
              kinds=POISONS, extra_keys=(), nan_oracle: Optional[Callable[[Dict, str], None]] = None) -> str:
    """The clean frame twice (bit-equal), then one run per poison with every other group's y, features, weights and ``extra_keys``
    columns overwritten: the clean groups' outputs are bit-equal to the clean run's.  Inf and large values are not nulls, so the route
    must not move, and neither does a NaN under "ignore".  Under the drop policies a NaN is a null and the null scan may pick a masked
    route: the caller then passes ``nan_oracle(got, kernel)``, which compares the clean groups with the oracle at the project tolerance.  ``rows_of(key, array)`` gives the index (into axis 0) of the clean groups' part of an output.
    Returns the clean run's kernel."""
    bad, _, _ = every_other(d["offs"])
    fr.guards(np.nan)
    first, name = guarded(eng, f"{what} [clean]", call, fresh=True)
    again, name2 = guarded(eng, f"{what} [clean, again]", call, fresh=False)
    assert name == name2
    assert_same_bits(first, again, f"{what} [{name}]: two runs of the clean frame")
    sel = {k: rows_of(k, v) for k, v in first.items()}
    n_cols = len(d["cols"])
    clean_extra = {k: d["extra"][k] for k in extra_keys}
    try:
        for kind in kinds:
            flat = [d["y"]] + list(d["cols"]) + ([d["w"]] if d.get("w") is not None else []) + [c for k in extra_keys for c in clean_extra[k]]
            p = poisoned(flat, d["offs"], bad, kind)
            at = 1 + n_cols + (1 if d.get("w") is not None else 0)
            ex = {}
            for k in extra_keys:
                ex[k] = p[at:at + len(clean_extra[k])]
                at += len(clean_extra[k])
            fr.load(p[0], p[1:1 + n_cols], p[1 + n_cols] if d.get("w") is not None else None, ex)
            got, name_p = guarded(eng, f"{what} [{kind} next door]", call, fresh=False)
            if kind == "nan" and nan_oracle is not None:
                nan_oracle(got, name_p)
                continue
            assert name_p == name, (what, kind, "the route moved", name, name_p)
            assert_same_bits(first, got, f"{what} [{name}]: {kind} in every other group", rows=sel)
    finally:
        fr.load(d["y"], d["cols"], d.get("w"), clean_extra)
    return name


# ---------------------------------------------------------------------------------------------------------------- static oracle

def static_expected(d: Dict, policy: str, icpt: bool = False, **kw):
    """(coef, pred, resid) of the oracle on the rows the policy keeps"""
    from test_nulls_gpu import _expected

    return _expected(d["y"], d["cols"], d["offs"], d.get("w"), icpt, policy, **kw)


def check_static(got: Dict, exp, tol: float, what: str, groups=None) -> None:
    coef, pred, resid = exp
    if groups is None:
        close(got["coef"], coef, tol, f"{what} coef")
        for key, ref in (("pred", pred), ("resid", resid)):
            if key in got:
                close(got[key], ref, tol, f"{what} {key}")
    else:
        g, rows = groups
        close(got["coef"][g], coef[g], tol, f"{what} coef")
        for key, ref in (("pred", pred), ("resid", resid)):
            if key in got:
                close(got[key][rows], ref[rows], tol, f"{what} {key}")
    if "status" in got:
        assert got["status"].dtype == np.int32 and np.isin(got["status"], GROUP_STATUS).all(), (what, got["status"])


# ---------------------------------------------------------------------------------------------------------------- dynamic frames

def dyn_sizes(kind: str, rng, lo: int = 30, hi: int = 200) -> list:
    """(a) about 40 short sequences (packed tiles), (b) one sequence of about 5 000 rows (the carry across tiles), (c) both"""
    if kind == "a":
        return odd_total(rng.integers(lo, hi + 1, size=40))
    if kind == "b":
        return [5003]
    short = rng.integers(lo, hi + 1, size=20)
    return odd_total(list(short[:12]) + [3001] + list(short[12:]) + [1501])


def dyn_data(seed: int, dtype, k: int, sizes, nan_frac: float = 0.0) -> Dict:
    rng = np.random.default_rng(seed)
    offs = offsets_of(sizes)
    n = int(offs[-1])
    cols = [rng.standard_normal(n).astype(dtype) for _ in range(k)]
    y0 = (sum(c.astype(np.float64) for c in cols) + 0.1 * rng.standard_normal(n)).astype(dtype)
    valid = None
    y = y0
    if nan_frac > 0:
        valid = (rng.random(n) >= nan_frac).astype(np.uint8)
        y = y0.copy()
        y[valid == 0] = np.nan
    return {"y": y, "y0": y0, "cols": cols, "offs": offs, "is_valid": valid}


def packed_tiles(offs, tile_rows: int) -> bool:
    """whether the row-parallel dynamic kernels cut this frame into packed tiles (whole sequences per tile, at least 70 % full)"""
    sizes = np.diff(offs)
    if int(sizes.max()) > tile_rows - 3:
        return False
    n_tiles, base = 0, -1
    for g in range(len(sizes)):
        if sizes[g] == 0:
            continue
        if base < 0 or offs[g + 1] - base > tile_rows:
            n_tiles += 1
            base = int(offs[g]) & ~3
    return n_tiles * tile_rows * 7 <= int(offs[-1]) * 10


def halo_batches(half_life) -> int:
    if half_life is None:
        return 0
    need = 36.0 * half_life                                   # ff^need = 2^-36 with ff = 2^(-1 / half_life)
    nb = 1 if need <= 256.0 else math.ceil(need / 256.0)
    return nb if nb <= 8 else 0


def rls_kernel(k: int, half_life, offs, dtype, engine: Optional[str] = None, nulls: bool = False, aligned: bool = True) -> str:
    """the kernel the RLS dispatcher takes (csrc/api_dynamic.hip, pick_rls_route)"""
    dt = dt_name(dtype)
    max_rows, n = int(np.diff(offs).max()), int(offs[-1])
    if k > 128:
        return f"k3y_rls_inverse_hbm_{dt}"
    if k > 32:
        return f"k3x_rls_inverse_{dt}"
    if k <= 10 and engine is None and aligned:
        tile = 1024 if k <= 6 else 512
        n_tiles = (n + tile - 1) // tile
        halo = 0 if (packed_tiles(offs, tile) or nulls or k > 9) else halo_batches(half_life)
        if halo and k <= 6 and halo <= 4 and n_tiles > 1:
            return f"k3s_rls_rows_lookback_{dt}"
        return f"k3s_rls_rows_halo_{dt}" if halo else f"k3s_rls_rows_{dt}"
    if k > 8:
        return f"k3sw_rls_scan_walk_{dt}" if engine == "chunk" else f"k3p_rls_inverse_wave_{dt}"
    if engine == "chunk" or max_rows > 4096:
        return f"k3s_rls_scan_walk_{dt}"
    return f"k3_rls_{dt}"


def rolling_kernel(k: int, window: int, policy: str, offs, dtype, valid=None, engine: Optional[str] = None, aligned: bool = True) -> str:
    """the kernel (family) the rolling dispatcher takes (csrc/api_dynamic.hip, pick_rolling_route); K4p's names carry a lane suffix,
    so its entry is a prefix"""
    from test_k4_gpu import _keeps_a_never_dropped_row

    dt = dt_name(dtype)
    mp = min(k, window)
    chunk = (f"k4y_rolling_inverse_hbm_{dt}" if k > 128 else f"k4x_rolling_inverse_{dt}" if k > 32 else
             f"k4w_rolling_walk_{dt}" if k > 8 else f"k4_rolling_walk_{dt}")
    if engine == "chunk" or k > 32:
        return chunk
    wave = f"k4p_rolling_inverse_wave_{dt}"
    fits = packed_tiles(offs, 1024) or window <= (508 if k <= 6 else 252)
    if valid is None:
        return f"k4_rolling_tiles_{dt}" if (k <= 10 and fits and aligned) else wave if k > 8 else chunk
    if policy == "drop":
        if k <= 10 and (window <= (508 if k <= 6 else 252) or int(np.diff(offs).max()) <= 1021):
            return f"k4_rolling_tiles_{dt}_gathered"
        return wave if k > 8 else chunk                       # (K4p on the compacted frame: "<wave>..._compacted")
    if k <= 10 and fits and aligned and not _keeps_a_never_dropped_row(offs, valid, window, mp):
        return f"k4_rolling_tiles_masked_{dt}"
    return wave if k > 8 else chunk


def check_rolling_singular(got: Dict, d: Dict, k: int, window: int, what: str, rows=None) -> None:
    """A window of fewer rows than features: min_periods = min(k, window) = window, every solved window's sums are singular, and what the
    reference's LU makes of a zero or noise pivot (inf, NaN, 1e15-sized numbers; include/pols_mi355x.h, DIVERGENCE) is no oracle for values
    or for which solved rows are NaN.  What IS defined: the rows in front of the warm-up row, and whole sequences shorter than
    min_periods, hold NaN coefficients, and a null row's prediction is NaN."""
    from test_k4_gpu import _before_warm_up

    offs, valid = d["offs"], d["is_valid"]
    n = int(offs[-1])
    v = np.ones(n, dtype=np.uint8) if valid is None else valid
    sel = np.ones(n, dtype=bool) if rows is None else rows
    pre = _before_warm_up(offs, v, min(k, window)) & sel
    assert pre.any() and np.isnan(got["coef"][pre]).all(), (what, "rows before the warm-up row")
    assert np.isnan(got["pred"][pre]).all(), (what, "predictions before the warm-up row")
    assert np.isnan(got["pred"][sel & ~v.astype(bool)]).all(), (what, "pred of a null row")


def check_rolling(got: Dict, ref: Dict, d: Dict, k: int, window: int, policy: str, tol: float, what: str, rows=None) -> None:
    if window < k:
        return check_rolling_singular(got, d, k, window, what, rows)
    """The NaN pattern everywhere; values at ``tol`` on the rows whose window holds at least 2 k observations (a window of fewer is
    arbitrarily ill-conditioned: there the project compares at the window's own conditioning, test_k4_gpu._band_check, which is what a
    window shorter than 2 k gets here on every row).  ``rows``: a row mask to restrict everything to."""
    from test_k4_gpu import _band_check, _solved_source, _window_obs

    offs, valid = d["offs"], d["is_valid"]
    got_c, got_p = got["coef"].astype(np.float64), got["pred"].astype(np.float64)
    ref_c, ref_p = ref["coef"], ref["pred"]
    sel = np.ones(len(got_p), dtype=bool) if rows is None else rows
    vm = np.ones(len(got_p), dtype=bool) if valid is None else valid.astype(bool)
    assert np.array_equal(np.isnan(got_c)[sel], np.isnan(ref_c)[sel]), (what, "coef NaN pattern")
    assert np.isnan(got_p[sel & ~vm]).all(), (what, "pred of a null row")
    assert np.array_equal(np.isnan(got_p)[sel & vm], np.isnan(ref_p)[sel & vm]), (what, "pred NaN pattern")
    sane = sel & np.isfinite(ref_c).all(axis=1) & (np.abs(ref_c).max(axis=1) < 1e3)
    if window >= 2 * k:
        well = sane & (_window_obs(offs, valid, window, policy) >= 2 * k)
        assert well.sum() > 0.5 * sane.sum(), (what, int(well.sum()), int(sane.sum()))
        close(got_c[well], ref_c[well], tol, f"{what} coef")
    else:
        well = sane
        X = np.column_stack([c.astype(np.float64) for c in d["cols"]])
        src = _solved_source(ref_c, offs) if (policy == "drop_window" and valid is not None) else None
        _band_check(what, got_c, ref_c, np.flatnonzero(sane), offs, valid, X, window, policy, tol, src=src)
        with np.errstate(all="ignore"):
            well = sane & np.isclose(got_c, ref_c, rtol=tol, atol=tol).all(axis=1)      # predictions: where the window allowed `tol`
    close(got_p[well & vm], ref_p[well & vm], tol, f"{what} pred")
