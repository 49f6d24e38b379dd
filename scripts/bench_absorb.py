"""Engine.absorb (K16) on 10 000 groups x 1 000 rows x 8 features (f32), 20 ids per group, device-resident columns and outputs, in two
id layouts -- sorted inside every group (the identity order) and drawn per row (the radix order):
  absorb coef   want = coef (order, count, index, means, gram, solve)
  absorb all    every field (adds the residual pass per category, the finish and the prediction pass)
  statistics    Engine.least_squares_statistics with an intercept on the same frame: the nearest entry without absorption
Interleaved in one process after WARM warm-up rounds; per call the time between two device events, mean and standard deviation over
REPS rounds.  bytes: three reads of the 9 columns (means, gram, residuals) plus the ids (8 bytes a row) and the int32 category index
written and read once.  No threshold is asserted.  The lines go to the file named by the first argument (default
profiles/absorb_bench.txt) and to stdout."""
import json
import os
import sys
import time

import numpy as np

G, ROWS, K, N_IDS = 10_000, 1_000, 8, 20


def main(path):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from polars_ols_amd import _lib as L
    from polars_ols_amd.engine import Engine

    warm, reps = int(os.environ.get("WARM", 2)), int(os.environ.get("REPS", 7))
    eng = Engine(0)
    time.sleep(2.0)                                           # (let a benchmark process that has just exited finish tearing down)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    out = open(path, "w")

    def emit(d):
        print(json.dumps(d), flush=True)
        out.write(json.dumps(d) + "\n")
        out.flush()

    n = G * ROWS
    offs = np.arange(G + 1, dtype=np.int64) * ROWS
    gen = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda: torch.randn(n, device="cuda", generator=gen, dtype=torch.float32)  # noqa: E731
    cols = [rnd() for _ in range(K)]
    drawn = torch.randint(0, N_IDS, (n,), device="cuda", generator=gen, dtype=torch.int64)
    sorted_ids = drawn.view(G, ROWS).sort(dim=1).values.reshape(-1).contiguous()
    shock = torch.randn(N_IDS, device="cuda", generator=gen, dtype=torch.float32)
    nbytes = 3 * 4 * n * (K + 1) + 8 * n + 2 * 4 * n
    all_fields = ("coef", "pred", "resid", "status") + L.ABSORB_FIELDS
    means = {}
    for layout, ids in (("sorted", sorted_ids), ("drawn per row", drawn)):
        y = sum((j + 1) * 0.1 * c for j, c in enumerate(cols)) + shock[ids] + rnd()
        cases = {"absorb coef": lambda: eng.absorb(y, cols, ids, offs, want=("coef",), add_intercept=True),
                 "absorb all": lambda: eng.absorb(y, cols, ids, offs, want=all_fields, add_intercept=True),
                 "statistics": lambda: eng.least_squares_statistics(y, cols, offs, add_intercept=True)}
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
        cases["absorb coef"]()
        eng.synchronize()
        kern = eng.last_kernel
        for key, v in times.items():
            d = {"layout": layout, "call": key, "ms_mean": round(float(np.mean(v)), 4), "ms_std": round(float(np.std(v)), 4), "rounds": reps}
            if key != "statistics":
                d.update(kernel=kern, bytes=nbytes, TBps=round(nbytes / (float(np.mean(v)) * 1e-3) / 1e12, 4))
            emit(d)
            means[(layout, key)] = float(np.mean(v))
        emit({"layout": layout, "absorb_coef_over_statistics": round(means[(layout, "absorb coef")] / means[(layout, "statistics")], 3),
              "absorb_all_over_statistics": round(means[(layout, "absorb all")] / means[(layout, "statistics")], 3)})
    eng.close()
    out.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "absorb_bench.txt"))
