"""bench.py --dump-outputs without a GPU: every output array written whole as float32 / float64 while they fit the budget, a fixed
row sample of each (with its row numbers) once they do not, and a command line that asks for no timed step refused."""
import importlib.util
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_dump_test", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_writes_every_array_whole_within_the_budget(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(0)
    res = {"coef": rng.standard_normal((10, 3)).astype(np.float32), "pred": rng.standard_normal(30),
           "status": np.array([0, 1, -2, 0, 0, 0, 3, 0, 0, 0], dtype=np.int32), "resid": None}
    bench.dump_outputs(res, tmp_path / "out", bench.DUMP_BYTES)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["coef.npy", "pred.npy", "status.npy"]
    coef, pred, status = (np.load(tmp_path / "out" / f"{k}.npy") for k in ("coef", "pred", "status"))
    assert coef.dtype == np.float32 and np.array_equal(coef, res["coef"])
    assert pred.dtype == np.float64 and np.array_equal(pred, res["pred"])
    assert status.dtype == np.float64 and np.array_equal(status, res["status"])


def test_dump_outputs_samples_the_same_rows_to_fit_the_budget(tmp_path):
    bench = _bench()
    g = torch.Generator().manual_seed(1)
    res = {"pred": torch.randn(1_000_000, dtype=torch.float64, generator=g),
           "coef": torch.randn(100_000, 4, dtype=torch.float32, generator=g),
           "status": torch.zeros(100_000, dtype=torch.int32)}
    budget = 1_000_000
    for run in ("a", "b"):
        bench.dump_outputs(res, tmp_path / run, budget, "_rank1")
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(f"{k}_rank1{s}.npy" for k in res for s in ("", "_rows")), files
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= budget
    for k, v in res.items():
        a, rows = np.load(tmp_path / "a" / f"{k}_rank1.npy"), np.load(tmp_path / "a" / f"{k}_rank1_rows.npy")
        assert a.dtype == (np.float64 if k != "coef" else np.float32) and rows.dtype == np.float64
        idx = rows.astype(np.int64)
        assert np.array_equal(idx, rows) and len(idx) > 1000 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < v.shape[0]
        assert idx[-1] > 0.99 * v.shape[0]                                       # the sample spans the whole array
        assert np.array_equal(a, v.numpy()[idx].astype(a.dtype))
        assert np.array_equal(rows, np.load(tmp_path / "b" / f"{k}_rank1_rows.npy"))    # a function of the shape alone
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{k}_rank1.npy"))


def test_bench_refuses_zero_timed_steps():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr and not r.stdout
