"""CPU: any / anyLast / argMin / argMax without a GPU — the lowering (which
queries become plans, what describe() shows, which are refused and how) and the host + device
functions of csrc/pick.hpp (the tuple lower bound and the two order-word maps), built with g++
into a stand-alone program (tests/c/test_pick.cpp) and checked against Python on constructed
tuples and operands."""
import bisect
import struct
import subprocess
from pathlib import Path

import pytest

from nutdb_amd import NutError
from nutdb_amd.sql import Plan

ROOT = Path(__file__).resolve().parent.parent
I64_MIN, I64_MAX = -2**63, 2**63 - 1


def aggs(sql):
    d = Plan(sql).describe()
    assert d["kind"] == "groupby" and d["mode"] == "compiled"
    return d, [(a["op"], a.get("expr"), a.get("order")) for a in d["aggs"]]


@pytest.mark.parametrize("keys", ["", "k", "k, j, l", "k + 1, toYear(d)"], ids=["0", "1", "3", "computed"])
def test_accepted_with_keys(keys):
    sel = f"{keys}, " if keys else ""
    grp = f" group by {keys}" if keys else ""
    d, a = aggs(f"select {sel}argMax(a, b), argMin(a * 2, b), any(a), anyLast(x) from t where c > 1{grp}")
    assert a == [("argMax", "a", "b"), ("argMin", "(a * 2)", "b"), ("any", "a", None), ("anyLast", "x", None)]
    assert len(d["keys"]) == (keys.count(",") + 1 if keys else 0)
    assert [o["from"] for o in d["outputs"]][-4:] == ["agg"] * 4


def test_names_are_case_insensitive():
    _, a = aggs("select ARGMAX(a, b), argmin(a, b), ANY(a), anylast(a) from t")
    assert [x[0] for x in a] == ["argMax", "argMin", "any", "anyLast"]


def test_having_order_by_arithmetic_and_neighbours():
    d, a = aggs("select k, sum(a), countUnique(u), argMax(a, b) - min(a) as spread from t group by k "
                "having argMin(a, b) > 3 and any(a) < 9 order by anyLast(a) desc, argMax(a, b)")
    assert [x[0] for x in a] == ["sum", "count_distinct", "argMax", "min", "argMin", "any", "anyLast"]
    outs = {o["name"]: o for o in d["outputs"]}
    assert outs["spread"]["from"] == "expr" and d["having"] is True
    hidden = [o["name"] for o in d["outputs"] if o.get("hidden")]
    assert "argMin(a, b)" in hidden and "any(a)" in hidden and "anyLast(a)" in hidden
    assert [o["desc"] for o in d["order"]] == [True, False]
    # the ORDER BY argMax(a, b) is the hidden operand of `spread`'s, not a second aggregate
    assert sum(x[0] == "argMax" for x in a) == 1


def test_identical_calls_are_merged():
    _, a = aggs("select k, argMax(a, b), argMax(a, b) + 1, argMax(a, b + 0), argMax(x, b), argMin(a, b), any(a), any(a) * 2 "
                "from t group by k")
    assert a == [("argMax", "a", "b"), ("argMax", "a", "(b + 0)"), ("argMax", "x", "b"), ("argMin", "a", "b"),
                 ("any", "a", None)]


def test_other_query_shapes_lower():
    d = Plan("select k, argMax(a, b) from t group by k union all select k, any(a) from u group by k").describe()
    assert [b["aggs"][0]["op"] for b in d["union_all"]] == ["argMax", "any"]
    d = Plan("select k, v from (select k, argMax(a, b) as v from t group by k) as d where v > 1").describe()
    assert d["derived"]["aggs"][0]["op"] == "argMax"
    d = Plan("with w as (select k, anyLast(a) as v from t group by k) select k, v from w where v > 1").describe()
    assert d["derived"]["aggs"][0]["op"] == "anyLast"
    d = Plan("select count() from t where a > (select argMin(a, b) from t)").describe()
    assert d["subqueries"][0]["aggs"][0]["op"] == "argMin"


@pytest.mark.parametrize("sql,frag", [
    ("select argMax(a) from t", "argMax takes two arguments"),
    ("select argMin(a, b, c) from t", "argMin takes two arguments"),
    ("select any(a, b) from t", "any takes one argument"),
    ("select anyLast() from t", "anyLast takes one argument"),
    ("select argMax(a, case when b > 1 then b end) from t", "argMax: a NULL branch"),
    ("select k, any(case when a > 1 then a end) from t group by k", "any: a NULL branch"),
    ("select argMax(sum(a), b) from t", "aggregate 'sum' nested"),
    ("select argMin(a, count()) from t", "aggregate 'count' nested"),
    ("select argMax(a, any(b)) from t", "aggregate 'any' nested"),
    ("select t.k, argMax(t.a, u.b) from t join u on t.k = u.k group by t.k", "argMax over a JOIN"),
    ("select t.k, any(u.b) from t join u on t.k = u.k join w on w.k = u.k group by t.k", "any over a JOIN"),
    ("select k, anyLast(a) from t where exists (select 1 from u where u.k = t.k) group by k", "anyLast over a JOIN"),
])
def test_refusals(sql, frag):
    with pytest.raises(NutError) as e:
        Plan(sql)
    assert e.value.status == 7 and frag in str(e.value), str(e.value)


# ---------------------------------------------------------------- pick.hpp, stand-alone
def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


F64_BITS = [f64_bits(x) for x in (0.0, -0.0, float("inf"), float("-inf"), 1.0, -1.0, 5e-324, -5e-324,
                                  2.2250738585072009e-308, -2.2250738585072009e-308, 1.5, -1e300)] + \
           [0x7FF8000000000000, 0xFFF8000000000000, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FF0000000000001]
I64_BITS = [v & (2**64 - 1) for v in (0, 1, -1, I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1, 2**40, -2**40)]

# sorted group tuples and the tuples looked up in them: present ones, and absent ones below,
# between and above the groups
G1 = [I64_MIN, -7, 0, 3, 4, I64_MAX]
Q1 = G1 + [I64_MIN + 1, -8, -6, 1, 2, 5, I64_MAX - 1]
G2 = [(I64_MIN, I64_MIN), (I64_MIN, 0), (I64_MIN, I64_MAX), (-1, 5), (0, -3), (0, 0), (0, 9), (7, I64_MIN), (7, I64_MAX),
      (I64_MAX, I64_MIN), (I64_MAX, I64_MAX - 1)]
Q2 = G2 + [(I64_MIN, 1), (I64_MIN, -1), (-2, 0), (-1, 4), (-1, 6), (0, -4), (0, 1), (0, 10), (3, 3), (7, 0),
           (I64_MAX, I64_MAX), (I64_MAX - 1, 0)]


def script():
    lines, want = [], []
    for nk, groups, queries in ((1, [(g, 0) for g in G1], [(q, 12345) for q in Q1]), (2, G2, Q2),
                                (1, [], [(0, 0)]), (2, [(5, 5)], [(5, 4), (5, 5), (5, 6), (4, 9), (6, -9)]),
                                (0, [(0, 0)], [(77, -77)])):
        lines.append(f"g {nk} {len(groups)}")
        lines += [f"{a} {b}" for a, b in groups]
        cut = [g[:nk] for g in groups]
        for q in queries:
            lines.append(f"q {q[0]} {q[1]}")
            lb = bisect.bisect_left(cut, q[:nk])
            found = 0 if nk == 0 else lb if lb < len(cut) and cut[lb] == q[:nk] else -1
            want.append(f"{lb} {found}")
    for b in I64_BITS:
        lines.append(f"i {b:x}")
        want.append(f"{b ^ (1 << 63):016x}")
    for b in F64_BITS:
        lines.append(f"f {b:x}")
        want.append(f"{(~b & (2**64 - 1)) if b >> 63 else (b | (1 << 63)):016x}")
    return lines, want


def restatement_orders_as_specified():
    """the expected words themselves: the int64 map is monotone in the signed value; the f64 map
    puts -NaN < -inf < -1 < -denormal < -0 < +0 < denormal < 1 < inf < NaN"""
    def fo(b):
        return (~b & (2**64 - 1)) if b >> 63 else (b | (1 << 63))
    chain = [0xFFFFFFFFFFFFFFFF, 0xFFF8000000000000, f64_bits(float("-inf")), f64_bits(-1e300), f64_bits(-1.0),
             f64_bits(-2.2250738585072009e-308), f64_bits(-5e-324), f64_bits(-0.0), f64_bits(0.0), f64_bits(5e-324),
             f64_bits(1.0), f64_bits(float("inf")), 0x7FF0000000000001, 0x7FF8000000000000, 0x7FFFFFFFFFFFFFFF]
    words = [fo(b) for b in chain]
    assert words == sorted(words) and len(set(words)) == len(words)
    signed = sorted(v - 2**64 if v >> 63 else v for v in I64_BITS)
    assert [(v & (2**64 - 1)) ^ (1 << 63) for v in signed] == sorted((v & (2**64 - 1)) ^ (1 << 63) for v in signed)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_pick_hpp_stand_alone(tmp_path, flags):
    exe = tmp_path / "test_pick"
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "nutdb_amd" / "csrc"),
                    str(ROOT / "tests" / "c" / "test_pick.cpp"), "-o", str(exe)], check=True)
    restatement_orders_as_specified()
    lines, want = script()
    r = subprocess.run([str(exe)], input="".join(x + "\n" for x in lines), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    bad = [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not bad, bad[:5]
