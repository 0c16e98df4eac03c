"""bench.py --dump-outputs, host side: step_outputs names what a step returned and
dump_outputs writes it as float64 .npy files — full-range int64 as exact hi / lo halves,
large results as a fixed, seeded row sample within the size budget."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402


def _join(d, name):
    hi, lo = np.load(d / f"{name}_hi.npy"), np.load(d / f"{name}_lo.npy")
    assert hi.dtype == lo.dtype == np.float64
    return (hi.astype(np.int64) << 32) | lo.astype(np.int64)


def test_groupby_outputs_exact(tmp_path):
    rng = np.random.default_rng(1)
    keys = np.sort(rng.integers(-2**63, 2**63 - 1, size=(1000, 1), dtype=np.int64), axis=0)
    keys[0, 0], keys[-1, 0] = -2**63, 2**63 - 1
    sums = rng.standard_normal((1000, 1))
    info = bench.dump_outputs(tmp_path, bench.step_outputs("groupby", (keys, sums.view(np.uint64))))
    assert sorted(info) == ["keys_hi", "keys_lo", "sums"]
    assert all(v == {"rows_written": 1000, "rows": 1000} for v in info.values())
    assert np.array_equal(_join(tmp_path, "keys"), keys)
    got = np.load(tmp_path / "sums.npy")
    assert got.dtype == np.float64 and np.array_equal(got, sums)


def test_q1_outputs(tmp_path):
    keys = np.array([[65, 70], [78, 70], [82, 70]], dtype=np.int64)
    words = np.empty((3, 4), dtype=np.uint64)
    sums = np.array([[1.5, 2.25, 3.0], [4.0, 5.5, 6.0], [7.0, 8.0, 9.125]])
    words[:, :3] = sums.view(np.uint64)
    words[:, 3] = [10, 20, 2**40]
    bench.dump_outputs(tmp_path, bench.step_outputs("q1", (keys, words)))
    assert np.array_equal(np.load(tmp_path / "keys.npy"), keys.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "sums.npy"), sums)
    assert np.array_equal(np.load(tmp_path / "count.npy"), [10.0, 20.0, float(2**40)])


def test_large_output_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 600)
    col = torch.from_numpy(np.random.default_rng(2).integers(-2**63, 2**63 - 1, size=5000, dtype=np.int64))
    n = torch.tensor([4000])
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(a, bench.step_outputs("filter", (col, n)))
    bench.dump_outputs(b, bench.step_outputs("filter", (col.clone(), n)))
    # budget: 600 values over 1 (count) + 2 (hi, lo) per row -> 200 rows of the 4000 selected
    assert info["selected_hi"] == {"rows_written": 200, "rows": 4000}
    assert np.load(a / "count.npy").tolist() == [4000.0]
    got = _join(a, "selected")
    assert np.array_equal(got, _join(b, "selected"))
    sel = col[:4000].numpy()
    pos = np.searchsorted(np.sort(sel), got)
    assert np.array_equal(np.sort(sel)[pos], got)  # every sampled value is one of the selected
    order = {v: i for i, v in enumerate(sel.tolist())}
    rows = [order[v] for v in got.tolist()]
    assert rows == sorted(rows)  # in row order
    size = sum(f.stat().st_size for f in a.glob("*.npy"))
    assert size <= 8 * 600 + 128 * 3


def test_plan_outputs(tmp_path):
    r = {"l_shipmode": np.array([3, 5]), "high_line_count": np.array([7, 9]), "avg": np.array([0.5, 0.25])}
    outs = bench.step_outputs("q12expr", r)
    assert [(n, k) for n, _, k in outs] == [("l_shipmode", "int"), ("high_line_count", "int"), ("avg", "f64")]
    bench.dump_outputs(tmp_path, outs)
    assert np.load(tmp_path / "avg.npy").tolist() == [0.5, 0.25]


def test_plain_run_skips_the_extras(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.steps == 3 and not a.full and a.no_cpu_baseline and a.no_copy_floor and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    a = bench.parse()
    assert a.full and not a.no_cpu_baseline and not a.no_copy_floor
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline"])
    a = bench.parse()
    assert a.no_cpu_baseline and not a.no_copy_floor
