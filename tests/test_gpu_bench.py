"""bench.py end to end on a small Q1 input (main() in this process): a plain run times the
steps and prints the result line without the extras, --dump-outputs writes the last timed
step's groups (checked against the C oracle), and --full still adds the copy floor, the
launch-shape runs and the CPU baseline with its parity check."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = 100_003


def _run(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--rows", str(ROWS), *argv])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_and_dump(monkeypatch, capsys, tmp_path, orc):
    from nutdb_amd.workloads import Q1_COLS, Q1_DATE_K
    line = _run(monkeypatch, capsys, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert line["metric"] == bench.METRIC and line["unit"] == "rows/s" and line["higher_is_better"] is True
    assert line["dtype"] == "i64+f64" and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(ROWS / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert "cpu_baseline" not in line and "parity" not in line and "launch_shape" not in line["config"]
    assert line["roofline"]["copy_floor"] is None and line["roofline"]["achieved"] > 0
    sd, rf, ls, qty, price, disc = [orc.gen(s, ROWS) for s in Q1_COLS]
    ok, ow = orc.groupby([rf, ls], [(0, 0, (0,)), (0, 0, (1,)), (0, 4, (1, 2)), (1, 0, ())],
                         values=[qty, price, disc], preds=[(sd, 1, Q1_DATE_K)])
    got = {f.stem: np.load(f) for f in tmp_path.glob("*.npy")}
    assert sorted(got) == ["count", "keys", "sums"] == sorted(line["outputs"])
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["keys"], ok.astype(np.float64))
    assert np.array_equal(got["count"], ow[:, 3].astype(np.float64))
    want = np.ascontiguousarray(ow[:, :3]).view(np.float64)
    assert np.max(np.abs(got["sums"] - want) / np.abs(want)) <= 1e-12


def test_full_run_keeps_the_extras(monkeypatch, capsys):
    line = _run(monkeypatch, capsys, "--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "0.05")
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["parity"]["ok"] and line["parity"]["full_size"]
    assert line["cpu_baseline"]["value"] > 0
    assert line["roofline"]["copy_floor"]["ms"] > 0
    assert sorted(line["config"]["launch_shape"]["kernel_ms_full_size"]) == ["128x3", "128x4", "192x2"]
