"""CPU: the exactly defined math functions themselves (nutdb_amd/csrc/prog_ops.hpp: jroundf,
jroundi, jsqrt, jsignf / jsigni, jleast* / jgreatest*, jtoi64, jnarrow, jtof32: what the generated
kernels, the planner's constant folding and the group-output expressions all call), built with
g++ into a stand-alone program (tests/c/test_math_ops.cpp) and run over every edge operand of
tests/math_edges.py.  Expected values: that file's Python restatement (pinned against exact
arithmetic by tests/test_math_edges_cpu.py).  Bit-exact, no operand skipped; a second build runs
the same input under UBSan with the float-cast check (gcc's `undefined` leaves it out, and the
casts are where it matters)."""
import subprocess
from pathlib import Path

import pytest

import math_edges as M
from expr_edges import EE, MAX, MIN

ROOT = Path(__file__).resolve().parent.parent
NF = [0, 1, -1, 2, -2, 5, 18, -18]  # digit counts over f64
NI = [0, 2, -1, -2, -18]            # and over int64


def _rows():
    """(input line, expected output word) for every operand"""
    rows = []
    ib = [x % 2**64 for x in M.I]
    for m in range(4):
        for n in NF:
            rows += [(f"roundf {m} {n} {b:x} 0", M.word(M.round_f(x, m, n))) for b, x in zip(M.F_BITS, M.F)]
        for n in NI:
            rows += [(f"roundi {m} {n} {b:x} 0", M.word(M.round_i(x, m, n))) for b, x in zip(ib, M.I)]
    rows += [(f"sqrt 0 0 {b:x} 0", M.word(M.sqrt(x))) for b, x in zip(M.F_BITS, M.F)]
    rows += [(f"sqrt 0 0 {M.fbits(x):x} 0", M.word(M.sqrt(x))) for x in M.SQRT_X]
    rows += [(f"signf 0 0 {b:x} 0", M.word(M.sign(x))) for b, x in zip(M.F_BITS, M.F)]
    rows += [(f"signi 0 0 {b:x} 0", M.word(M.sign(x))) for b, x in zip(ib, M.I)]
    for g in (False, True):
        fn = "greatest" if g else "least"
        rows += [(f"{fn}f 0 0 {M.fbits(a):x} {M.fbits(b):x}", M.word(M.least(a, b, g))) for a, b in zip(*M.FF)]
        rows += [(f"{fn}i 0 0 {a % 2**64:x} {b % 2**64:x}", M.word(M.least(a, b, g)))
                 for a, b in zip(EE[0].tolist(), EE[1].tolist())]
    for c in range(8):
        rows += [(f"castf {c} 0 {b:x} 0", M.word(M.cast(x, c))) for b, x in zip(M.F_BITS, M.F)]
        rows += [(f"casti {c} 0 {b:x} 0", M.word(M.cast(x, c))) for b, x in zip(ib, M.I)]
    return rows


ROWS = _rows()


def test_operands_are_all_in():
    nf, ni = len(M.F), len(M.I)
    n = 4 * (len(NF) * nf + len(NI) * ni) + 2 * nf + len(M.SQRT_X) + ni + 2 * (len(M.FF[0]) + len(EE[0])) + 8 * (nf + ni)
    assert len(ROWS) == n > 9000
    inputs = {r[0] for r in ROWS}
    for v in (MIN, MAX, MIN + 5, MAX - 4, 5 * 10**17, -5 * 10**17):
        assert f"roundi 3 -18 {v % 2**64:x} 0" in inputs and f"roundi 0 -1 {v % 2**64:x} 0" in inputs
    for b in (M.SNAN, M.NEG_QNAN, M.fbits(2.0**63), M.fbits(-2.0**63), M.fbits(1e19), M.fbits(float("inf")), M.fbits(-0.5)):
        assert f"castf 0 0 {b:x} 0" in inputs and f"roundf 1 2 {b:x} 0" in inputs and f"sqrt 0 0 {b:x} 0" in inputs
    # the answers the issue names
    want = dict(ROWS)
    assert want[f"roundf 1 0 {M.fbits(-0.5):x} 0"] == 0x8000000000000000  # ceil(-0.5) = -0.0
    assert want[f"castf 0 0 {M.fbits(1e19):x} 0"] == MAX and want[f"castf 0 0 {M.SNAN:x} 0"] == 0
    assert want[f"castf 3 0 {M.fbits(128.0):x} 0"] == (-128) % 2**64 and want[f"castf 3 0 {M.fbits(127.5):x} 0"] == 127
    assert want[f"sqrt 0 0 {M.fbits(-1.0):x} 0"] == M.NEG_QNAN and want[f"sqrt 0 0 {M.SNAN:x} 0"] == M.SNAN | M.QUIET


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all"]],
                         ids=["plain", "ubsan"])
def test_math_ops_on_every_edge_operand(tmp_path, flags):
    exe = tmp_path / "test_math_ops"
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "nutdb_amd" / "csrc"),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "c" / "test_math_ops.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], input="".join(i + "\n" for i, _ in ROWS), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x, 16) for x in r.stdout.split()]
    assert len(got) == len(ROWS)
    bad = [(i, hex(w), hex(g)) for (i, w), g in zip(ROWS, got) if w != g]
    assert not bad, f"{len(bad)} of {len(ROWS)} differ; first (input, want, got): {bad[:5]}"
