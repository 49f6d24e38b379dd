"""Engine.absorb2 (K17) on its two recorded shapes (f32, device-resident columns and outputs, ids drawn per row, unweighted, intercept):
  A  2 000 groups x 1 000 rows x 8 features, 50 x 20 ids per group   (the resident route: one workgroup per (group, column), column in LDS)
  B  one group of 1 000 000 rows x 8 features, 50 000 x 20 ids       (the global route: ten workgroups in all, the column in the scratch)
Per shape: ``absorb2 all`` (every field) and ``absorb2 coef`` (no residual pass), the sweeps the call made (the largest n_iter), and
``absorb one-way`` -- Engine.absorb (K16) on the same frame and the first id column, every field --, the yardstick: a two-way fit cannot
cost less than the one-way fit plus its sweeps.  Interleaved in one process after WARM warm-up rounds; per call the time between two
device events, mean and standard deviation over REPS rounds (shape B: one warm-up round and three timed ones at the most).  No
threshold is asserted.  The lines go to the file named by the first argument (default profiles/absorb2_bench.txt) and to stdout."""
import json
import os
import sys

import numpy as np

SHAPES = {"A": (2_000, 1_000, 8, 50, 20), "B": (1, 1_000_000, 8, 50_000, 20)}


def main(path):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from polars_ols_amd import _lib as L
    from polars_ols_amd.engine import Engine

    warm, reps = int(os.environ.get("WARM", 2)), int(os.environ.get("REPS", 7))
    eng = Engine(0)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    out = open(path, "w")

    def emit(d):
        print(json.dumps(d), flush=True)
        out.write(json.dumps(d) + "\n")
        out.flush()

    two = ("coef", "pred", "resid", "status") + L.ABSORB2_FIELDS
    one = ("coef", "pred", "resid", "status") + L.ABSORB_FIELDS
    for shape in os.environ.get("SHAPES", "A,B").split(","):
        G, rows, K, n1, n2 = SHAPES[shape]
        w_, r_ = (min(warm, 1), min(reps, 3)) if shape == "B" else (warm, reps)
        n = G * rows
        offs = np.arange(G + 1, dtype=np.int64) * rows
        gen = torch.Generator(device="cuda").manual_seed(0)
        rnd = lambda: torch.randn(n, device="cuda", generator=gen, dtype=torch.float32)  # noqa: E731
        ids1 = torch.randint(0, n1, (n,), device="cuda", generator=gen, dtype=torch.int64)
        ids2 = torch.randint(0, n2, (n,), device="cuda", generator=gen, dtype=torch.int64)
        s1 = torch.randn(n1, device="cuda", generator=gen, dtype=torch.float32)
        s2 = torch.randn(n2, device="cuda", generator=gen, dtype=torch.float32)
        cols = [rnd() + 0.5 * s1[ids1] + 0.5 * s2[ids2] for _ in range(K)]
        y = sum((j + 1) * 0.1 * c for j, c in enumerate(cols)) + s1[ids1] + s2[ids2] + rnd()
        cases = {"absorb2 all": lambda: eng.absorb2(y, cols, ids1, ids2, offs, want=two, add_intercept=True),
                 "absorb2 coef": lambda: eng.absorb2(y, cols, ids1, ids2, offs, want=("coef", "status", "n_iter"), add_intercept=True),
                 "absorb one-way": lambda: eng.absorb(y, cols, ids1, offs, want=one, add_intercept=True)}
        times = {k: [] for k in cases}
        for rnd_i in range(w_ + r_):
            for key, call in cases.items():
                eng.synchronize()
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call()
                eng.synchronize()
                t1.record()
                t1.synchronize()
                if rnd_i >= w_:
                    times[key].append(t0.elapsed_time(t1))
        res = cases["absorb2 coef"]()
        eng.synchronize()
        kern, sweeps, status = eng.last_kernel, int(res["n_iter"].max()), sorted(set(res["status"].cpu().tolist()))
        for key, v in times.items():
            d = {"shape": shape, "groups": G, "rows": rows, "features": K, "ids": [n1, n2], "call": key,
                 "ms_mean": round(float(np.mean(v)), 4), "ms_std": round(float(np.std(v)), 4), "rounds": r_}
            if key != "absorb one-way":
                d.update(kernel=kern, sweeps=sweeps, status=status)
            emit(d)
        emit({"shape": shape, "absorb2_all_over_one_way": round(float(np.mean(times["absorb2 all"]) / np.mean(times["absorb one-way"])), 3)})
        del cols, y, ids1, ids2
    eng.close()
    out.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "absorb2_bench.txt"))
