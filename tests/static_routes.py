"""The recorded routes of the static least-squares dispatcher (tests/static_routes.json) and the frames they were recorded on.

The data file holds, per case, a shape description -- dtype, columns, weights, null policy, a recipe for the group sizes with its
seed, solver parameters, library options -- and the exact ``last_kernel`` string the library produced for it BEFORE the dispatcher
was split into a plan resolver, a route picker and one function per route.  It is a measurement of that parent, never of the code
under test: test_static_route_gpu.py holds the library to the strings, test_static_route_cpu.py holds ``pols_debug_static_route``
to their families without a device.

File layout: ``names_front_coded`` is the sorted table of kernel strings, each as "n|suffix" = the first n characters of the
previous string + suffix.  ``grid`` is the grid of test_routing_gpu.py: per (rows, aligned "a" / ragged "r") the names (indices into
the table) of the 112 shapes of its SHAPES list in order, on the very frames that test draws from its one generator seeded
rows + ragged and checks against the oracle.  ``options`` repeats grid chunks under a library option and lists only the shapes
(position: name) whose kernel differs from the grid's.  ``sections`` hold the other cases: ``common`` (shared fields), ``fields`` and
``rows`` (the last field ``name`` an index).  A case without ``sizes`` has ``groups`` groups of ``rows`` rows, exactly (``ragged`` 0)
or drawn like the grid's (``ragged`` 1)."""
import json
from pathlib import Path

import numpy as np

PATH = Path(__file__).resolve().parent / "static_routes.json"
DTYPES = {"f32": np.float32, "f64": np.float64}


def load(path=PATH):
    """-> list of case dicts (``name`` resolved to the recorded string, ``id`` unique)"""
    doc = json.loads(Path(path).read_text())
    names = []
    for coded in doc["names_front_coded"]:
        n, suffix = coded.split("|", 1)
        names.append((names[-1][:int(n)] if names else "") + suffix)
    out = []

    def grid_chunk(section, chunk, idx, extra):
        for (dt, kt, w, pol), i in zip(GRID_SHAPES, idx):
            out.append(dict(extra, groups=5, frames="routing_grid", dtype=dt, kt=kt, weights=w, policy=pol, rows=int(chunk[:-1]),
                            ragged=int(chunk[-1] == "r"), name=names[i], section=section))

    for chunk, idx in doc["grid"].items():
        grid_chunk("grid", chunk, idx, {})
    for opt, chunks in doc["options"].items():
        for chunk, diff in chunks.items():
            idx = [diff.get(str(j), i) for j, i in enumerate(doc["grid"][chunk])]
            grid_chunk("options", chunk, idx, {"options": dict([opt.split("=")])})
    for sec in doc["sections"]:
        for row in sec["rows"]:
            c = dict(sec.get("common", {}))
            c.update(zip(sec["fields"], row))
            out.append(dict(c, name=names[c["name"]], section=sec["section"]))
    count = {}
    for c in out:
        count[c["section"]] = count.get(c["section"], 0) + 1
        c["id"] = f"{c['section']}[{count[c['section']] - 1}]"
    return out


def group_sizes(case, rng):
    """The group sizes of a case: the recipe ``sizes`` or (groups, rows, ragged)."""
    rec = case.get("sizes")
    if rec is None:
        g, rows = case["groups"], case["rows"]
        if not case.get("ragged"):
            return np.full(g, rows, dtype=np.int64)
        return rng.integers(max(case["kt"] + 3, rows - rows // 8), rows + 1, size=g).astype(np.int64)
    kind = rec[0]
    if kind == "mix":                       # ["mix", [[count, rows], ...]]: shuffled
        s = np.concatenate([np.full(n, r, dtype=np.int64) for n, r in rec[1]])
    elif kind == "lognormal":               # ["lognormal", groups, median, sigma, [[count, rows], ...]]: shuffled, the extras included
        s = np.maximum(8, np.round(rec[2] * np.exp(rec[3] * rng.standard_normal(rec[1])))).astype(np.int64)
        s = np.concatenate([s] + [np.full(n, r, dtype=np.int64) for n, r in rec[4]])
    else:
        raise ValueError(kind)
    rng.shuffle(s)
    return s


def frame(case):
    """-> y, cols, offsets, weights (or None): full-rank columns, 2 % null targets under a null policy other than "ignore" """
    rng = np.random.default_rng(case["seed"])
    offs = np.concatenate([[0], np.cumsum(group_sizes(case, rng))]).astype(np.int64)
    dt, kt, n = DTYPES[case["dtype"]], case["kt"], int(offs[-1])
    x = rng.standard_normal((kt, n)).astype(dt)
    y = (x.sum(axis=0, dtype=np.float64) + 0.1 * rng.standard_normal(n)).astype(dt)
    if case.get("policy", "ignore") != "ignore":
        y[rng.random(n) < 0.02] = np.nan
    w = rng.uniform(0.5, 2.0, n).astype(dt) if case.get("weights") else None
    return y, list(x), offs, w


GRID_KT = (1, 3, 6, 8, 9, 10, 12, 15, 16, 17, 20, 24, 25, 31)
GRID_SHAPES = [(dt, kt, w, pol) for dt in ("f32", "f64") for kt in GRID_KT for w in (0, 1) for pol in ("ignore", "drop")]


def routing_grid_frames(rows, ragged):
    """The frames of test_routing_gpu.py's grid for one (rows, ragged), from the same generator consumed in the same order."""
    rng = np.random.default_rng(rows + int(ragged))
    for name, kt, w, pol in GRID_SHAPES:
        dt = DTYPES[name]
        sizes = rng.integers(max(kt + 3, rows - rows // 8), rows + 1, size=5) if ragged else np.full(5, rows)
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n = int(offs[-1])
        cols = [rng.standard_normal(n).astype(dt) for _ in range(kt)]
        y = (sum(c.astype(np.float64) for c in cols) + 0.1 * rng.standard_normal(n)).astype(dt)
        if pol == "drop":
            y[rng.random(n) < 0.02] = np.nan
        yield (name, kt, w, pol), y, cols, offs, (rng.uniform(0.5, 2.0, n).astype(dt) if w else None)


def frames(cases):
    """-> (case, y, cols, offsets, weights) for every case, in order; runs of "routing_grid" cases must be whole (rows, ragged) grids"""
    i = 0
    while i < len(cases):
        c = cases[i]
        if c.get("frames") != "routing_grid":
            yield (c,) + frame(c)
            i += 1
            continue
        for shape, y, cols, offs, w in routing_grid_frames(c["rows"], c["ragged"]):
            g = cases[i]
            assert (g["dtype"], g["kt"], g["weights"], g["policy"], g["rows"], g["ragged"]) == shape + (c["rows"], c["ragged"]), g["id"]
            yield g, y, cols, offs, w
            i += 1


def solver_kwargs(case):
    """keyword arguments of Engine.least_squares for the case's solver parameters"""
    kw = dict(case.get("params", {}))
    kw["null_policy"] = case.get("policy", "ignore")
    return kw


def family(name):
    """last_kernel string -> the route of the picker (the names of pols_debug_static_route)"""
    if " | " in name:
        return "classes_streamed_top" if name.startswith("k5_gram_stream") else "classes"
    if name.startswith("k2w_"):
        return "k2w"
    if name.startswith("k2_"):
        return "k2"
    if name.startswith("k8"):
        return "wide"
    if name == "k6_small_svd_all_groups":
        return "svd_all"
    if name.startswith(("k1_", "k1t_", "k1p_", "k1m_")):
        return "k1"
    assert name.startswith("k5_gram_stream"), name
    return "streamed"
