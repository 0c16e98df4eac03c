"""GPU: the generated expression code (csrc/jit.cpp: the prelude's jmod, jdiv, jshl, jshr, jabs,
jfmod, jdatepart, the int -> f64 conversions of as_f, constants as kernel arguments) on the
edge operands of tests/expr_edges.py — the integer, conversion and calendar counterpart of
tests/test_gpu_nonfinite.py.  The reference is the numpy expression oracle (oracle/expr.py),
which tests/test_expr_edges_cpu.py holds to exact arithmetic on these same operands; where
Python has the exact answer at hand (datetime, fractions) it is compared as well.

Everything is bit-exact, with one rule taken from test_gpu_nonfinite.py: a NaN that an
operation MAKES from non-NaN operands (here only 0 * +-inf) has the hardware's sign, so
there isnan() is asked; a NaN operand passes through bit for bit.  Every test asserts how
many cells it compared.  Inputs are at most a few thousand rows: the cost is the hipRTC
compiles, about 27 distinct kernels in the file (constants are kernel arguments, so
sweeping them compiles nothing: test_expr_edges_cpu.py::test_constant_specs_share_one_source)."""
import numpy as np
import pytest
import torch

import expr_edges as X
from expr_edges import E, MAX, MIN, bits
from nutdb_amd import NutError, ProgQuery
from oracle.expr import F64, date_part, eval_prog, groupby_prog

pytestmark = pytest.mark.gpu

NEG_ZERO = 0x8000000000000000


def dev(x, ex):
    return torch.from_numpy(np.ascontiguousarray(x)).to(ex.device)


def run_eval(ex, cols, progs):
    """(words uint64 [nprogs, n], valid uint8 [nprogs, n]) of nut_eval_rows"""
    out, valid = ex.eval_rows([dev(c, ex) for c in cols], progs)
    return (np.stack([bits(o.cpu().numpy()) for o in out]), np.stack([v.cpu().numpy() for v in valid]))


def want_eval(cols, progs):
    """the same from the oracle: a masked-out row holds word 0 and valid 0; a row error is
    returned per program (True where the value or the mask program fails)"""
    words, valid, errs = [], [], []
    for val, mask in progs:
        v, _, e = eval_prog(val, cols)
        ok = np.ones(len(v), dtype=bool)
        if mask:
            m, _, me = eval_prog(mask, cols)
            ok = m != 0
            e = (e & ok) | me
        words.append(np.where(ok, bits(v), np.uint64(0)))
        valid.append(ok.astype(np.uint8))
        errs.append(e)
    return np.stack(words), np.stack(valid), np.stack(errs)


def check_eval(ex, name, cols, k=-1, cells=None):
    types, progs = X.eval_specs(k)[name]
    assert len(types) == len(cols)
    gw, gv = run_eval(ex, cols, progs)
    ww, wv, we = want_eval(cols, progs)
    assert not we.any()
    assert gw.shape == ww.shape and (cells is None or gw.size == cells), (gw.shape, cells)
    assert np.array_equal(gv, wv), name
    assert np.array_equal(gw, ww), (name, k, np.argwhere(gw != ww)[:5])
    return gw, gv


# ------------------------------------------------------------------ a. int ops over EE
def test_int_ops_all_pairs(ex):
    """add sub mul shl shr bitand bitor bitxor, the six compares, abs, bitnot over all 784
    ordered pairs of E: wrap, shift counts outside [0, 63] and negative, abs(MIN) = MIN"""
    cols = list(X.EE)
    gw, _ = check_eval(ex, "int_bin", cols, cells=8 * 784)
    check_eval(ex, "int_cmp_unary", cols, cells=8 * 784)
    a, b = X.EE
    shr = gw[X.INT_BIN.index("shr")].view(np.int64)
    out = (b < 0) | (b > 63)
    assert int(out.sum()) == 784 - 28 * 6  # E holds six counts inside [0, 63]: 0, 1, 2, 3, 7, 63
    assert np.array_equal(shr[out], np.where(a[out] < 0, -1, 0))
    assert not gw[X.INT_BIN.index("shl")][out].any()


def test_int_division_masked_and_bare(ex):
    """mod / intdiv over EE behind the mask col1 != 0: MIN % -1 = 0, MIN div -1 = MIN; the 28
    rows with a zero divisor are invalid and hold word 0.  Without the mask both programs fail
    the call."""
    cols = list(X.EE)
    a, b = X.EE
    gw, gv = check_eval(ex, "int_div_masked", cols, cells=2 * 784)
    for j in range(2):
        assert np.array_equal(gv[j], (b != 0).astype(np.uint8))
        assert int((gv[j] == 0).sum()) == 28 and not gw[j][b == 0].any()
    row = int(np.flatnonzero((a == MIN) & (b == -1))[0])
    assert gw[0][row] == 0 and gw[1].view(np.int64)[row] == MIN
    for name in ("int_mod_bare", "int_intdiv_bare"):
        with pytest.raises(NutError, match="division by zero"):
            run_eval(ex, cols, X.eval_specs()[name][1])


# ------------------------------------------------------------------ b. the right operand a constant
def test_int_ops_with_constants(ex):
    """the same ops as col0 <op> k with k every value of E (MIN, MAX and -1 among them) through
    the kernel arguments: three kernels for the 28 constants"""
    e = X.i64(E)
    cells = 0
    for k in E:
        cells += check_eval(ex, "int_bin_k", [e], k)[0].size + check_eval(ex, "int_cmp_k", [e], k)[0].size
        if k == 0:
            with pytest.raises(NutError, match="division by zero"):
                run_eval(ex, [e], X.eval_specs(0)["int_div_k"][1])
        else:
            cells += check_eval(ex, "int_div_k", [e], k)[0].size
    assert cells == 28 * 28 * 14 + 27 * 28 * 2


# ------------------------------------------------------------------ c. conversions, mixed types
def test_int_to_f64_and_mixed(ex):
    """to_f64 (round half to even at 2^53 + 1, MAX -> 2^63), int + f64, int * f64, int - f64,
    IF promotion and the six compares over E x F (NaN rows included), both operand orders"""
    i, f = X.EF
    types, progs = X.eval_specs()["mixed_a"]
    gw, gv = run_eval(ex, [i, f], progs)
    ww, _, we = want_eval([i, f], progs)
    assert gw.shape == (8, 1036) and gv.all() and not we.any()
    made = np.isnan(ww[2].view(np.float64)) & ~np.isnan(f)  # 0 * +-inf: the sign of a NaN made here is the hardware's
    assert int(made.sum()) == 2 and np.isnan(gw[2].view(np.float64)[made]).all()
    gw[2][made] = ww[2][made]
    assert np.array_equal(gw, ww), np.argwhere(gw != ww)[:5]
    tf = gw[0].view(np.float64)
    assert tf[i == 2**53 + 1][0] == 2.0**53 and tf[i == MAX][0] == 2.0**63 and tf[i == -2**53 - 1][0] == -2.0**53
    nan = np.isnan(f)
    assert int(nan.sum()) == 28 and not gw[4:8][:, nan].any()  # lt le gt ge with a NaN
    gw, _ = check_eval(ex, "mixed_b", [i, f], cells=6 * 1036)
    assert not gw[0][nan].any() and gw[1][nan].all()           # eq / ne with a NaN
    big = (i == 2**53 + 1) & (f == 2.0**53)
    assert int(big.sum()) == 2 and gw[0][big].all()            # 2^53 + 1 = 2.0^53 after the conversion


def test_int_div_is_f64(ex):
    a, b = X.EE
    nz = b != 0  # (x / 0 belongs to test_gpu_nonfinite.py)
    gw, _ = check_eval(ex, "int_div_f64", [a[nz], b[nz]], cells=756)
    assert gw[0].view(np.float64)[(a[nz] == MAX) & (b[nz] == MAX)][0] == 1.0


# ------------------------------------------------------------------ d. f64 arithmetic
def f64_arith(ex, a, b, c=None):
    cols = [a, b, np.zeros(len(a)) if c is None else c]
    progs = X.eval_specs()["f64_arith"][1]  # mod, a * b + c, div, mul: one kernel for the three tests
    gw, gv = run_eval(ex, cols, progs)
    assert gv.all()
    return gw, want_eval(cols, progs)[0]


def test_f64_mod_edges(ex):
    """fmod over FA x FB: huge quotients (1e300 mod 3, DBL_MAX mod 0.1), subnormal operands
    and results, x mod inf = x, and the sign of a zero result (the dividend's)"""
    gw, ww = f64_arith(ex, *X.FAB)
    assert gw[0].shape == (130,) and np.array_equal(ww[0], bits(X.FAB_WANT))
    assert np.array_equal(gw[0], ww[0]), [(X.FAB[0][r], X.FAB[1][r]) for r in np.flatnonzero(gw[0] != ww[0])[:5]]
    assert int((gw[0] == NEG_ZERO).sum()) == 21


def test_f64_mul_add_is_not_contracted(ex):
    """a * b + c rounds twice (the generated kernels are compiled with -ffp-contract=off, as
    the precompiled ones are): every triple here gives another word when fused"""
    a, b, c, twice = X.FMA
    gw, ww = f64_arith(ex, a, b, c)
    assert len(a) >= 64 and np.array_equal(ww[1], bits(twice))
    assert np.array_equal(gw[1], bits(twice)), int((gw[1] != bits(twice)).sum())


def test_f64_div_mul_correctly_rounded(ex):
    """/ and * over 4096 full-mantissa pairs, subnormal results to near overflow: both are
    correctly rounded IEEE operations, so the device equals the host bit for bit"""
    a, b = X.DIVP
    gw, ww = f64_arith(ex, a, b)
    with np.errstate(all="ignore"):
        assert np.array_equal(ww[2], bits(a / b)) and np.array_equal(ww[3], bits(a * b))
    assert gw[2].shape == gw[3].shape == (4096,)
    for j in (2, 3):
        bad = np.flatnonzero(gw[j] != ww[j])
        assert len(bad) == 0, (j, len(bad), [(a[r].hex(), b[r].hex()) for r in bad[:3]])


# ------------------------------------------------------------------ e. datepart
def test_datepart_edges(ex):
    days = X.i64(X.DAYS)
    gw, _ = check_eval(ex, "datepart", [days], cells=len(X.DAYS) * 8)
    got = gw.view(np.int64).T
    want = np.stack([date_part(days, p) for p in range(8)], axis=1)
    assert got.shape == (len(X.DAYS), 8) and np.array_equal(got, want)
    cal = np.array(X.IN_CALENDAR)
    assert int(cal.sum()) == 111
    assert got[cal].tolist() == [X.calendar_parts(d) for d, c in zip(X.DAYS, X.IN_CALENDAR) if c]
    at = {d: got[r].tolist() for r, d in enumerate(X.DAYS)}
    assert at[MIN] == at[-2**40 - 1] == at[-2**40] != at[-2**40 + 1] and at[MAX] == at[2**40 + 1] == at[2**40]


# ------------------------------------------------------------------ f. the other kernels
@pytest.mark.parametrize("name", sorted(X.SELECT_SPECS))
def test_select_rows_edges(ex, name):
    types, where = X.SELECT_SPECS[name]
    cols = list(X.EE)
    got = ex.select_rows([dev(c, ex) for c in cols], where).cpu().numpy()
    w, _, e = eval_prog(where, cols)
    want = np.flatnonzero(w != 0)
    assert not e.any() and 1 <= len(want) <= 783
    assert got.dtype == np.int64 and np.array_equal(got, want)


def groupby_table(groups):
    a, b = X.EE
    f = np.resize(X.f64(X.F), 784)
    g = np.arange(784, dtype=np.int64) * 7 % groups
    return [a, b, f, g]


OPNUM = {"sum": 0, "count": 1, "min": 2, "max": 3}


@pytest.mark.parametrize("nk,hint,groups", [(0, 0, 1), (1, 4, 3), (1, 64, 50)], ids=["global", "private", "shared"])
def test_groupby_edges(ex, nk, hint, groups):
    """SUM (wrapping) / COUNT / MIN / MAX of the int programs, MIN and MAX of fmod and of
    int + f64 (above 2^53, up to +inf), the divisions behind the aggregate mask col1 != 0"""
    cols = groupby_table(groups)
    keys = [cols[3]][:nk]
    q = ProgQuery(keys=[dev(k, ex) for k in keys], cols=[dev(c, ex) for c in cols], aggs=X.GROUPBY_AGGS)
    gk, gw = ex.groupby(q, group_hint=hint).to_host_words()
    ok, ow, types = groupby_prog(keys, cols, None, [(OPNUM[o], v, m) for o, v, m in X.GROUPBY_AGGS])
    assert gw.shape == ow.shape == (groups, 8) and types[4:] == [F64] * 4
    if nk:
        assert np.array_equal(gk, ok)
    assert int(ow[:, 1].sum()) == 784 - 28
    assert np.isposinf(ow[:, 7].view(np.float64)).any() and (ow[:, 4].view(np.float64) < 0).any()
    assert np.array_equal(gw, ow), np.argwhere(gw != ow)[:5]


@pytest.mark.parametrize("name", sorted(X.KEY_SPECS))
def test_computed_key_edges(ex, name):
    """key programs whose value is INT64_MIN — the hash table's empty marker — next to -1 and
    MAX: abs(MIN), 1 shl 63, MIN intdiv 1"""
    keys, where = X.KEY_SPECS[name]
    cols = list(X.EE)
    q = ProgQuery(keys=keys, cols=[dev(c, ex) for c in cols], where=where, aggs=X.KEY_AGGS)
    gk, gw = ex.groupby(q, group_hint=1024).to_host_words()
    ok, ow, _ = groupby_prog(keys, cols, where, [(OPNUM[o], v, m) for o, v, m in X.KEY_AGGS])
    for j in range(len(keys)):
        assert MIN in ok[:, j] and (MAX in ok[:, j] or name == "abs_shl")
    assert -1 in ok[:, -1] and len(ok) > 100 and int(ow[:, 0].sum()) == (784 if where is None else 756)
    assert gk.shape == ok.shape and np.array_equal(gk, ok)
    assert np.array_equal(gw, ow), np.argwhere(gw != ow)[:5]
    if where is not None:  # without its WHERE the key program meets the zero divisors
        with pytest.raises(NutError, match="division by zero"):
            ex.groupby(ProgQuery(keys=keys, cols=[dev(c, ex) for c in cols], aggs=X.KEY_AGGS), group_hint=1024)


# ------------------------------------------------------------------ g. SQL
def test_sql_edges(ex):
    n = len(X.DAYS)
    a, f, d = np.resize(X.i64(E), n), np.resize(X.f64(X.F), n), X.i64(X.DAYS)
    got = ex.sql(X.SQL_EDGES, {"a": dev(a, ex), "f": dev(f, ex), "d": dev(d, ex)})
    assert list(got) == [nm for nm, _, _ in X.SQL_ITEMS] + [f"fold{j}" for j in range(len(X.FOLD_DAYS))]
    cells = 0
    for name, sql, prog in X.SQL_ITEMS:
        v, t, e = eval_prog(prog, [a, f, d])
        assert not e.any() and not np.ma.isMaskedArray(got[name])
        assert got[name].dtype == (np.float64 if t == F64 else np.int64), sql
        assert np.array_equal(bits(got[name]), bits(v)), (sql, np.flatnonzero(bits(got[name]) != bits(v))[:5])
        cells += len(v)
    assert cells == len(X.SQL_ITEMS) * n == 20 * 122
    assert int(got["fe"].sum()) == int((f == 2.0**53).sum()) > 0
    # the host twin (sql_lower.cpp date_part) folds a literal as the device computes a column
    for j, day in enumerate(X.FOLD_DAYS):
        assert got[f"fold{j}"].tolist() == [int(date_part(X.i64([day]), 7)[0])] * n
    fold = ex.sql("select a, " + ", ".join(f"toYYYYMMDD({day}) as f{j}" for j, day in enumerate(X.DAYS)) + " from t",
                  {"a": dev(a[:1], ex)})
    assert [int(fold[f"f{j}"][0]) for j in range(n)] == got["dp7"].tolist() and len(fold["a"]) == 1
    with pytest.raises(NutError, match="outside int64"):
        ex.sql("select a + 9223372036854775808 as x from t", {"a": dev(a, ex)})


# ------------------------------------------------------------------ h. WHERE constants
def test_fused_where_constants_exact(ex):
    """`col <cmp> k` on the fused filter: resolve_i64 (sql_exec_scan.cpp) turns a fractional,
    negative-fractional or out-of-range constant into an int64 predicate, all rows or none.
    Reference: exact rational comparison (fractions.Fraction of the literal's text)."""
    col = X.where_column()
    ints = [int(v) for v in col]
    t = {"col": dev(col, ex)}
    runs = 0
    for k in X.WHERE_CONSTS:
        for op in X.SQL_CMP:
            want = col[np.array([X.exact_compare(v, op, k) for v in ints])]
            for sql in (f"col {op} {k}", f"{k} {X.MIRROR[op]} col"):
                got = ex.sql(f"select col from t where {sql}", t)["col"]
                assert np.array_equal(got, want), (sql, len(got), len(want))
                runs += 1
    assert runs == 17 * 6 * 2
    kept = []
    for lo, hi in X.BETWEENS:  # fused group-by predicates: two resolve_i64 bounds
        keep = np.array([X.exact_compare(v, ">=", lo) and X.exact_compare(v, "<=", hi) for v in ints])
        got = ex.sql(f"select count(*) as c, min(col) as mn, max(col) as mx from t where col between {lo} and {hi}", t)
        assert int(got["c"][0]) == int(keep.sum()), (lo, hi)
        if keep.any():
            assert (int(got["mn"][0]), int(got["mx"][0])) == (int(col[keep].min()), int(col[keep].max())), (lo, hi)
        kept.append(int(keep.sum()))
    assert kept[5] == 0 and kept[6] == 4099 and all(0 < c < 4099 for c in kept[:5])


@pytest.mark.parametrize("op", sorted(X.COMPILED_CONSTS))
def test_compiled_where_constants(ex, op):
    """The same comparison with `and col % 1 = 0` is compiled (plan lowering): the
    constant becomes a program node — a decimal literal the nearest f64, an integer literal
    an int64 — and an int compared with an f64 converts to f64.  So:
      * full column: the compiled rows are the oracle's under that rule;
      * a column within +-2^53 (every value converts exactly): compiled = fused = exact,
        unless rounding the LITERAL to f64 moved it onto or across a value of the column
        — of these constants only 9007199254740992.5 -> 2^53, which differs at col = 2^53
        and nowhere else."""
    from fractions import Fraction
    col = X.where_column()
    small = np.where((col >= -2**53) & (col <= 2**53), col, col >> 11)
    assert {2**53, -2**53, 0, -1} <= set(small.tolist()) and int(np.abs(small).max()) == 2**53
    for k in X.COMPILED_CONSTS[op]:
        decimal = "." in k
        node = [("f64", 0, float(Fraction(k)))] if decimal else X.K(int(k))
        for c, within in ((col, False), (small, True)):
            t = {"col": dev(c, ex)}
            comp = ex.sql(f"select col from t where col {op} {k} and col % 1 = 0", t)["col"]
            w, _, e = eval_prog(X.C0 + node + [(X.SQL_CMP[op],)], [c])
            assert not e.any() and np.array_equal(comp, c[w != 0]), (op, k, within)
            if not within:
                continue
            fused = ex.sql(f"select col from t where col {op} {k}", t)["col"]
            exact = np.array([X.exact_compare(int(v), op, k) for v in c])
            assert np.array_equal(fused, c[exact]), (op, k)
            moved = Fraction(float(Fraction(k))) != Fraction(k) and abs(Fraction(k)) <= 2**53 + 1
            if moved:
                assert k == "9007199254740992.5" and (w != 0).tolist() != exact.tolist()
                assert set(c[(w != 0) != exact].tolist()) == {2**53}
            else:
                assert np.array_equal(comp, fused), (op, k)
