"""Engine.random_effects (K19) against Engine.absorb (K16) on the same frame in the same run, device-resident columns and outputs:
  10 000 groups x 1 000 rows x 8 features, f32 and f64, with 15 and with 100 ids per group (ids drawn per row),
  one f64 group of 300 000 rows with 5 000 ids (the table kernel's global route).
Per shape four calls, interleaved in one process after WARM warm-up rounds; per call the time between two device events, mean and
standard deviation over REPS rounds:
  re coef / re all            want = coef / every field of the entry
  absorb coef / absorb all    the baseline with the matching ``want``
and the ratios re / absorb.  absorb with statistics runs the column passes random effects runs for its coefficients alone (means, moments,
residuals), so re_coef_over_absorb_all is the ratio at equal column traffic.  No threshold is asserted.  With KERNELS=1 the script makes one
call of each kind on the shape numbered SHAPE (default 0) and nothing else -- the body of a kernel-trace run of its own.  The lines go to the file named by the first
argument (default profiles/random_effects_bench.txt) and to stdout."""
import json
import os
import sys
import time

import numpy as np

K = 8
SHAPES = [("f32", 10_000, 1_000, 15), ("f32", 10_000, 1_000, 100), ("f64", 10_000, 1_000, 15), ("f64", 10_000, 1_000, 100),
          ("f64", 1, 300_000, 5_000)]


def main(path):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from polars_ols_amd import _lib as L
    from polars_ols_amd.engine import Engine

    warm, reps = int(os.environ.get("WARM", 2)), int(os.environ.get("REPS", 7))
    trace_only = os.environ.get("KERNELS") == "1"
    eng = Engine(0)
    time.sleep(2.0)                                           # (let a benchmark process that has just exited finish tearing down)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    out = open(path, "w")

    def emit(d):
        print(json.dumps(d), flush=True)
        out.write(json.dumps(d) + "\n")
        out.flush()

    re_all = ("coef", "pred", "resid", "status") + L.RANDOM_EFFECTS_FIELDS
    ab_all = ("coef", "pred", "resid", "status") + L.ABSORB_FIELDS
    shapes = [SHAPES[int(os.environ.get("SHAPE", 0))]] if trace_only else SHAPES
    for dt_name, G, rows, n_ids in shapes:
        dt = torch.float32 if dt_name == "f32" else torch.float64
        n = G * rows
        offs = np.arange(G + 1, dtype=np.int64) * rows
        gen = torch.Generator(device="cuda").manual_seed(0)
        rnd = lambda: torch.randn(n, device="cuda", generator=gen, dtype=dt)  # noqa: E731
        ids = torch.randint(0, n_ids, (n,), device="cuda", generator=gen, dtype=torch.int64)
        shock = lambda: torch.randn(n_ids, device="cuda", generator=gen, dtype=dt)[ids]  # noqa: E731
        cols = [rnd() + 0.5 * shock() for _ in range(K)]
        y = sum((j + 1) * 0.1 * c for j, c in enumerate(cols)) + 1.5 * shock() + rnd()
        cases = {"re coef": lambda: eng.random_effects(y, cols, ids, offs, want=("coef",), add_intercept=True),
                 "re all": lambda: eng.random_effects(y, cols, ids, offs, want=re_all, add_intercept=True),
                 "absorb coef": lambda: eng.absorb(y, cols, ids, offs, want=("coef",), add_intercept=True),
                 "absorb all": lambda: eng.absorb(y, cols, ids, offs, want=ab_all, add_intercept=True)}
        shape = {"dtype": dt_name, "groups": G, "rows": rows, "ids": n_ids}
        if trace_only:
            for call in cases.values():
                call()
                eng.synchronize()
            emit(dict(shape, traced=list(cases)))
            continue
        times = {k: [] for k in cases}
        for rnd_i in range(warm + reps):
            for key, call in cases.items():
                eng.synchronize()
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call()
                eng.synchronize()
                t1.record()
                t1.synchronize()
                if rnd_i >= warm:
                    times[key].append(t0.elapsed_time(t1))
        res = cases["re coef"]()
        eng.synchronize()
        kern = eng.last_kernel
        status = eng.random_effects(y, cols, ids, offs, want=("status",), add_intercept=True)["status"]
        mean = {k: float(np.mean(v)) for k, v in times.items()}
        for key, v in times.items():
            d = dict(shape, call=key, ms_mean=round(mean[key], 4), ms_std=round(float(np.std(v)), 4), rounds=reps)
            if key.startswith("re"):
                d.update(kernel=kern, groups_ok=int((status == 0).sum().item()))
            emit(d)
        emit(dict(shape, re_coef_over_absorb_coef=round(mean["re coef"] / mean["absorb coef"], 3),
                  re_all_over_absorb_all=round(mean["re all"] / mean["absorb all"], 3),
                  re_coef_over_absorb_all=round(mean["re coef"] / mean["absorb all"], 3)))
        del res, cols, y, ids
        torch.cuda.empty_cache()
    eng.close()
    out.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                            "random_effects_bench.txt"))
