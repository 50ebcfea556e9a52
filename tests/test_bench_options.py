"""bench.py's options on the host: --steps / --warmup defaults per workload and the --dump-outputs writer."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_steps_are_what_the_command_line_says():
    b = load_bench()
    a = b.parse_args([])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (200, 20, False, None)
    a = b.parse_args(["--workload", "wholebody"])
    assert (a.steps, a.warmup) == (20, 3)
    a = b.parse_args(["--workload", "wholebody", "--steps", "200", "--warmup", "20", "--full"])
    assert (a.steps, a.warmup, a.full) == (200, 20, True)


def test_dump_keeps_small_outputs_whole(tmp_path):
    b = load_bench()
    X = torch.randn(8, 5, 3)
    b.write_outputs(str(tmp_path), {"X": X, "status": torch.arange(8, dtype=torch.int32), "loss": torch.tensor(0.5, dtype=torch.float64)})
    assert sorted(os.listdir(tmp_path)) == ["X.npy", "loss.npy", "status.npy"]
    x, st, loss = (np.load(tmp_path / f"{n}.npy") for n in ("X", "status", "loss"))
    assert x.dtype == np.float32 and np.array_equal(x, X.numpy())
    assert st.dtype == np.float32 and np.array_equal(st, np.arange(8))
    assert loss.dtype == np.float64 and loss.shape == () and loss == 0.5


def test_dump_samples_large_outputs_to_the_budget_with_a_fixed_seed(tmp_path):
    b = load_bench()
    rows = 4096
    X = np.arange(rows * 256, dtype=np.float32).reshape(rows, 256)
    s = np.arange(rows, dtype=np.float64)
    budget = 2 * 10 ** 6                                   # 4.2 MB of outputs
    for d in ("a", "b"):
        b.write_outputs(str(tmp_path / d), {"X": X, "s": s}, budget=budget)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= budget
    xa, sa = np.load(tmp_path / "a" / "X.npy"), np.load(tmp_path / "a" / "s.npy")
    assert 0 < xa.shape[0] < rows and xa.shape[1:] == (256,) and sa.shape == (xa.shape[0],)
    assert np.array_equal(xa[:, 0] / 256, sa)              # the same rows of every array of that length
    assert np.array_equal(xa, np.load(tmp_path / "b" / "X.npy")) and np.array_equal(sa, np.load(tmp_path / "b" / "s.npy"))
