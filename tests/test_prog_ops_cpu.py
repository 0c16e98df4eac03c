"""CPU: the expression-op functions themselves (nutdb_amd/csrc/prog_ops.hpp: what the generated
kernels, the planner's constant folding and the group-output expressions all call), built with
g++ into a stand-alone program (tests/c/test_prog_ops.cpp) and run over every edge operand of
tests/time_edges.py and tests/expr_edges.py.  Expected values: the Python restatement of the
calendar ops (pinned against `datetime` by tests/test_time_edges_cpu.py) and the numpy oracle
on one-node programs for the integer ops (pinned against exact arithmetic by
tests/test_expr_edges_cpu.py).  Bit-exact, no operand skipped; a second build runs the same
input under UBSan."""
import subprocess
from pathlib import Path

import pytest

import expr_edges as X
import time_edges as T
from oracle.expr import I64, eval_prog

ROOT = Path(__file__).resolve().parent.parent


def _rows():
    """(input line, expected output line) for every operand"""
    rows = []
    for p in range(9):
        rows += [(f"timepart {p} {s} 0", str(T.time_part(s, p))) for s in T.SECONDS]
    for u in range(6):
        rows += [(f"datetrunc {u} {d} 0", str(T.date_trunc(d, u))) for d in T.DAYS]
    for p in range(11):
        rows += [(f"datepart {p} {d} 0", str(T.date_part(d, p))) for d in T.DAYS]
    rows += [(f"addmonths 0 {d} {n}", str(T.add_months(int(d), int(n)))) for d, n in zip(*T.MONTHS)]
    a, b = X.EE
    for fn, op in (("div", "intdiv"), ("mod", "mod"), ("shl", "shl"), ("shr", "shr")):
        got, t, err = eval_prog(X.bin_(op), [a, b])
        assert t == I64
        flag = [f" {int(e)}" for e in err] if op in X.DIVS else [""] * len(a)
        rows += [(f"{fn} 0 {x} {y}", f"{g}{f}") for x, y, g, f in zip(a.tolist(), b.tolist(), got.tolist(), flag)]
    got, t, err = eval_prog(X.C0 + [("abs",)], [X.i64(X.E)])
    assert t == I64 and not err.any()
    rows += [(f"abs 0 {x} 0", str(g)) for x, g in zip(X.E, got.tolist())]
    return rows


ROWS = _rows()


def test_operands_are_all_in():
    n = 9 * len(T.SECONDS) + (6 + 11) * len(T.DAYS) + len(T.MONTHS[0]) + 4 * len(X.EE[0]) + len(X.E)
    assert len(ROWS) == n == 9 * 473 + 17 * 122 + 884 + 4 * 784 + 28
    inputs = {r[0] for r in ROWS}
    for v in (X.MIN, X.MAX, 2**40 + 1, 2**40 - 1, -2**40 + 1, -2**40 - 1):
        assert f"datepart 7 {v} 0" in inputs and f"datetrunc 5 {v} 0" in inputs
        assert any(r.startswith(f"addmonths 0 {v} ") for r in inputs)
    for v in (X.MIN, X.MAX, T.SEC_CLAMP + 1, T.SEC_CLAMP - 1, -T.SEC_CLAMP + 1, -T.SEC_CLAMP - 1):
        assert f"timepart 8 {v} 0" in inputs
    assert {f"div 0 {X.MIN} -1", f"mod 0 {X.MIN} -1", f"div 0 {X.MAX} 0", "shl 0 1 64", f"abs 0 {X.MIN} 0"} <= inputs


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "ubsan"])
def test_prog_ops_on_every_edge_operand(tmp_path, flags):
    exe = tmp_path / "test_prog_ops"
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "nutdb_amd" / "csrc"),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "c" / "test_prog_ops.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], input="".join(i + "\n" for i, _ in ROWS), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(ROWS)
    bad = [(i, w, g) for (i, w), g in zip(ROWS, got) if w != g]
    assert not bad, f"{len(bad)} of {len(ROWS)} differ; first (input, want, got): {bad[:5]}"
