"""RLS on frames where a regressor falls silent -- exactly zero for a stretch of rows (an event dummy, a suspended series filled with
0, an exposure switched off) -- against the high-precision information-form reference (tests/rls_exact_ref.py).

In the exact recursion a silent column keeps its decayed information, so its coefficient keeps its old estimate.  K3c's truncated
forms (HALO, MODE 2, and LOOK-BACK-ONE, MODE 3) build a tile's carry-in from the rows just in front of it; when a column is stale in
those rows they extend the carry-in further back (k3c_scan.hip, DEEP carry-in).  Every route is pinned by eng.last_kernel.

Information-form routes (every K3c form, K3sw) must match the reference on every sampled row.  The P-form routes (K3, K3p, K3x, and
the lane-per-chunk K3s, which propagates the covariance form inside a chunk) share the reference implementation's own loss after a stretch ends (P / ff - k k' r cancels terms of size ff^-stretch): there every
row must be finite, and rows outside the band where the CPU oracle itself misses the exact answer (widened by BAND_MARGIN rows on
each side) must match."""
import functools
import zlib

import numpy as np
import pytest

from rls_exact_ref import exact_rls, precision_for

pytestmark = pytest.mark.gpu

# frames: sequence sizes, (column, first row, end row) of the silent stretch, prior (p0, mean); column 0 is a constant
FRAMES = {
    "before_underflow": ([12_000], (2, 3000, 5000), (10.0, None)),       # ends at row 5 000: ff^5000 / p0 is still an f64 at half_life 5
    "after_underflow": ([12_000], (2, 6000, 8000), (10.0, None)),        # ... at row 8 000 it is not: the truncated carry-in was singular
    "tile_aligned": ([12_288], (2, 2048, 6144), (10.0, None)),           # starts and ends on tile boundaries (1 024 and 512 rows)
    "short": ([12_000], (2, 3000, 3700), (10.0, None)),                  # control: shorter than a tile plus the halo
    "from_start": ([12_000], (2, 0, 4000), (10.0, None)),                # control: zero from the sequence's first row (the prior is exact)
    "to_end": ([12_000], (2, 7000, 12_000), (10.0, None)),               # silent to the sequence's end
    "seq_inside": ([4500, 7500], (2, 3000, 7000), (10.0, None)),         # the second sequence starts inside the stretch
    "mean": ([12_000], (2, 3000, 5000), (1e3, 0.25)),                    # a prior with a mean
    "long": ([20_000], (2, 4000, 11_000), (10.0, None)),                 # long half-lives: longer than a tile plus a 2 048-row halo
    "long_to_end": ([20_000], (2, 9000, 20_000), (10.0, None)),
    "packed": ([1000] * 12, (2, 1500, 9500), (10.0, None)),              # no sequence longer than a tile: packed tiles
    "small": ([6000], (2, 2000, 4000), (10.0, None)),                    # wide frames (the reference's cost grows with k^2)
}
BAND_MARGIN = 32


def _frame(name, k, dtype):
    sizes, (col, lo, hi), _ = FRAMES[name]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    rng = np.random.default_rng(zlib.crc32(f"{name}/{k}".encode()))
    X = [np.ones(n)] + [rng.standard_normal(n) for _ in range(k - 1)]
    X[col][lo:hi] = 0.0
    beta = rng.uniform(-2.0, 2.0, size=k)
    y = sum(b * c for b, c in zip(beta, X)) + 0.1 * rng.standard_normal(n)
    X = [c.astype(dtype) for c in X]
    return y.astype(dtype), X, offs


def _sample_rows(name, n, half_life, tile):
    _, (_, lo, hi), _ = FRAMES[name]
    reach = int(32 * (half_life or 8)) + 64
    parts = [np.arange(0, n, 23), [n - 1]]
    for e in (lo, hi):                                                   # dense around both ends of the stretch
        parts.append(np.arange(max(e - 16, 0), min(e + reach, n)))
    for t0 in range(tile, n, tile):                                      # every tile boundary
        parts.append(np.arange(max(t0 - 2, 0), min(t0 + 3, n)))
    return np.unique(np.concatenate([np.asarray(p, dtype=np.int64) for p in parts]))


@functools.lru_cache(maxsize=None)
def _reference(name, k, dtype_name, half_life):
    """(frame, exact coef / pred at the sampled rows, oracle coef / pred at the same rows): computed once per frame."""
    from oracle import orc

    dtype = np.dtype(dtype_name).type
    y, X, offs = _frame(name, k, dtype)
    n = int(offs[-1])
    _, (_, lo, hi), (p0, mean) = FRAMES[name]
    mean0 = None if mean is None else [mean] * k
    rows = _sample_rows(name, n, half_life, 1024 if k <= 6 else 512)
    ex = exact_rls(y, X, offs, rows, half_life=half_life, initial_state_covariance=p0, initial_state_mean=mean0,
                   digits=precision_for(half_life, min(hi, n) - lo))
    orc_out = orc.batched_rls(y, X, offs, half_life=half_life, initial_state_covariance=p0, initial_state_mean=mean0)
    return (y, X, offs, p0, mean0), rows, ex, {"coef": orc_out["coef"][rows], "pred": orc_out["pred"][rows]}


@pytest.fixture(scope="module")
def eng():
    from polars_ols_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.double().cpu().numpy()


def _run(eng, frame, half_life, opts):
    y, X, offs, p0, mean0 = frame
    for key, v in opts.items():
        eng.set_option(key, v)
    try:
        out = eng.recursive_least_squares(_cuda(y), [_cuda(c) for c in X], offs, half_life=half_life, initial_state_covariance=p0,
                                          initial_state_mean=mean0, null_free=True)
        eng.synchronize()
        return out, eng.last_kernel
    finally:
        for key in opts:
            eng.set_option(key, None)


def _check(name, rows, got, ex, orc_rows, tol, p_form, half_life):
    gc, gp = got["coef"][rows], got["pred"][rows]
    assert np.isfinite(gc).all() and np.isfinite(gp).all(), (name, rows[~np.isfinite(gc).all(axis=1)][:8])
    keep = np.ones(len(rows), dtype=bool)
    if p_form:
        # the band where the oracle (the reference implementation's P-form, in f64) misses the exact answer, widened by BAND_MARGIN rows
        miss = ~(np.isclose(orc_rows["coef"], ex["coef"], rtol=tol, atol=tol).all(axis=1) & np.isclose(orc_rows["pred"], ex["pred"], rtol=tol, atol=tol))
        for r in rows[miss]:
            keep &= np.abs(rows - r) > BAND_MARGIN
        assert keep.sum() > len(rows) // 2, name               # the band is a band, not the frame
    dc = np.abs(gc - ex["coef"]).max(axis=1)
    bad = keep & ~(np.isclose(gc, ex["coef"], rtol=tol, atol=tol).all(axis=1) & np.isclose(gp, ex["pred"], rtol=tol, atol=tol))
    assert not bad.any(), (name, half_life, int(bad.sum()), rows[bad][:10].tolist(), float(dc[bad].max()))


# (route id, features, half_life, options, expected kernel (dtype suffix added), P-form, frames)
K3C_FRAMES = ["before_underflow", "after_underflow", "tile_aligned", "short", "from_start", "to_end", "seq_inside", "mean"]
ROUTES = [
    ("lookback_hl5", 4, 5.0, {}, "k3s_rls_rows_lookback", False, K3C_FRAMES),
    ("lookback_hl21", 4, 21.0, {}, "k3s_rls_rows_lookback", False, ["long", "long_to_end", "tile_aligned", "seq_inside", "from_start"]),
    ("lookback_k6_spins0", 6, 5.0, {"RLS_SPINS": "0"}, "k3s_rls_rows_lookback", False, ["before_underflow", "after_underflow", "to_end", "seq_inside"]),
    ("lookback_hl21_spins0", 4, 21.0, {"RLS_SPINS": "0"}, "k3s_rls_rows_lookback", False, ["long", "long_to_end"]),
    ("lookback_early", 4, 5.0, {"RLS_EARLY": "1"}, "k3s_rls_rows_lookback", False, ["before_underflow", "tile_aligned", "to_end"]),
    ("halo_k7_hl43", 7, 43.0, {}, "k3s_rls_rows_halo", False, ["long", "long_to_end", "tile_aligned", "seq_inside", "from_start"]),
    ("halo_k9_hl56", 9, 56.5, {}, "k3s_rls_rows_halo", False, ["long", "long_to_end"]),
    ("halo_engine_hl5", 4, 5.0, {"RLS_ENGINE": "halo"}, "k3s_rls_rows_halo", False, ["before_underflow", "after_underflow", "tile_aligned", "to_end", "seq_inside", "mean"]),
    ("scan_engine", 4, 5.0, {"RLS_ENGINE": "scan"}, "k3s_rls_rows", False, ["before_underflow", "after_underflow", "to_end"]),
    ("scan_hl252", 4, 252.0, {}, "k3s_rls_rows", False, ["long"]),
    ("packed", 4, 5.0, {}, "k3s_rls_rows", False, ["packed"]),
    ("k3s_chunk", 4, 5.0, {"RLS_ENGINE": "chunk"}, "k3s_rls_scan_walk", True, ["before_underflow", "to_end"]),   # (P inside a chunk)
    ("k3sw_chunk_12", 12, 5.0, {"RLS_ENGINE": "chunk"}, "k3sw_rls_scan_walk", False, ["small"]),
    ("k3_seq", 4, 5.0, {"RLS_ENGINE": "seq"}, "k3_rls", True, ["before_underflow", "to_end"]),
    ("k3p_12", 12, 5.0, {}, "k3p_rls_inverse_wave", True, ["small"]),
    ("k3p_32", 32, 5.0, {}, "k3p_rls_inverse_wave", True, ["small"]),
    ("k3x_40", 40, 5.0, {}, "k3x_rls_inverse", True, ["small"]),
]
DTYPES = [(np.float64, 1e-6), (np.float32, 1e-4)]
# (P-form routes are held in f64 only: in f32 they lose more than the band's digits)
CASES = [pytest.param(r, f, dt, tol, id=f"{r[0]}-{f}-{np.dtype(dt).name}") for r in ROUTES for f in r[6] for dt, tol in DTYPES
         if not (r[5] and dt == np.float32)]


@pytest.mark.parametrize("route,frame,dtype,tol", CASES)
def test_rls_silent_column(eng, route, frame, dtype, tol):
    rid, k, half_life, opts, kernel, p_form, _ = route
    fr, rows, ex, orc_rows = _reference(frame, k, np.dtype(dtype).name, half_life)
    out, name = _run(eng, fr, half_life, opts)
    suffix = "_f32" if dtype == np.float32 else "_f64"
    assert name == kernel + suffix, (rid, name)
    _check(f"{rid}/{frame}", rows, {"coef": _np(out["coef"]), "pred": _np(out["pred"])}, ex, orc_rows, tol, p_form, half_life)
