"""GPU: the ordered group-by's kernels on inputs built around its sample (tests/gorder_shapes.py;
DESIGN.md §4.2f has the branch-to-case table).  Every test runs one case through
nut_groupby_to_host with page-locked outputs and asserts
  - keys and every aggregate word equal oracle.groupby, bit for bit;
  - the path and the decline reason equal the case's note;
  - groupby_heavy() equals the note exactly, in keys and in rows (a lookup that misses a heavy key
    changes no result: its rows travel through the levels instead);
  - groupby_overflow_rows() == 0 under the exact layout and where every cell fits its capped region,
    > 0 where the note says arenas.
tests/test_gorder_shapes_cpu.py proves the notes.  Columns are built and uploaded once per module
(a small cache: a case is 128 MB per column), and the oracle's result once per (case, aggregates)."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest
import torch

import gorder_shapes as S

pytestmark = pytest.mark.gpu

OP_NAMES = {0: "sum", 1: "count", 2: "min", 3: "max"}
_cases = OrderedDict()    # (builder, args) -> (case, device key column)
_values = {}              # (kind, slot, n) -> (host column, device column)
_oracle = OrderedDict()   # (case name, shape) -> (keys, words)


def get_case(ex, builder, *args):
    key = (builder.__name__, args)
    if key not in _cases:
        while len(_cases) >= 2:
            _cases.popitem(last=False)
        case = builder(*args)
        _cases[key] = (case, torch.from_numpy(case.keys).to(ex.device))
    _cases.move_to_end(key)
    return _cases[key]


def get_values(ex, shape, case, kd):
    """-> (host columns, device columns) of an aggregate shape; "k": the key column itself"""
    n = len(case.keys)
    if shape in S.IDENTITY_SHAPES:
        host = S.identity_columns(shape, case)
        return host, [torch.from_numpy(v).to(ex.device) for v in host]
    host, devc = [], []
    for i, kind in enumerate(S.SHAPES[shape][0]):
        if kind == "k":
            host.append(case.keys)
            devc.append(kd)
            continue
        if (kind, i, n) not in _values:
            for old in [k for k in _values if k[2] != S.N0 and k[2] != n]:
                del _values[old]
            v = S.value_column(kind, n, 0x60 + i)
            _values[(kind, i, n)] = (v, torch.from_numpy(v).to(ex.device))
        host.append(_values[(kind, i, n)][0])
        devc.append(_values[(kind, i, n)][1])
    return host, devc


def aggs_of(shape):
    return S.identity_aggs(shape) if shape in S.IDENTITY_SHAPES else S.oracle_aggs(shape)


def query_of(shape, kd, devc):
    from nutdb_amd import Agg, AggQuery
    aggs = [Agg("count") if op == 1 else Agg(OP_NAMES[op], "col", tuple(args)) for op, _, args in aggs_of(shape)]
    return AggQuery(keys=[kd], values=list(devc), aggs=aggs)


def oracle_of(orc, case, shape, host):
    key = (case.name, shape)
    if key not in _oracle:
        while len(_oracle) >= 6:
            _oracle.popitem(last=False)
        _oracle[key] = orc.groupby([case.keys], aggs_of(shape), values=host)
    return _oracle[key]


def pinned(rows, cols):
    return torch.empty((rows, cols), dtype=torch.int64, pin_memory=True).numpy()


def run_case(ex, orc, case, kd, shape, hint=None, keys_dev=None):
    """one nut_groupby_to_host of the case; asserts result, path, decline, heavy counts, overflow"""
    host, devc = get_values(ex, shape, case, kd)
    q = query_of(shape, kd if keys_dev is None else keys_dev, devc)
    ok, ow = oracle_of(orc, case, shape, host)
    note = case.note
    assert len(ok) == note["groups"]
    na = len(aggs_of(shape))
    out = (pinned(len(ok) + 64, 1), pinned(len(ok) + 64, na))
    k, w = ex.groupby_to_host(q, group_hint=case.hint if hint is None else hint, out=out)
    path, why = ex.groupby_stats()["path"], ex.groupby_declined()
    assert np.array_equal(k, ok)
    assert np.array_equal(w.view(np.uint64), ow)
    return path, why


def check_ordered(ex, case, path, why, heavy_opt=1):
    note = case.note
    assert (path, why) == (S.ORDERED, "none")
    assert ex.groupby_heavy() == ((len(note["heavy"]), note["heavy_rows"]) if heavy_opt else (0, 0))
    arenas = note["arenas"] if heavy_opt == 1 else note["arenas_capped"] if heavy_opt == 2 else None
    if arenas is not None:
        assert (ex.groupby_overflow_rows() > 0) == arenas


# ----------------------------------------------------------------------------- the heavy pass
@pytest.mark.parametrize("shape,heavy_opt", [("count", 1), ("one", 1), ("four", 1), ("one", 2)])
def test_sampled_heavy(ex, orc, opts, shape, heavy_opt):
    """the full heavy set at its cut (2048 / 512 / 409 keys, spare candidates beyond it), every key on
    a handful of sampled rows; COUNT alone is hk_split_kernel<0>, five aggregates over four columns <4>"""
    opts(gb_heavy=heavy_opt)
    case, kd = get_case(ex, S.sampled_heavy, S.shape_na(shape))
    path, why = run_case(ex, orc, case, kd, shape)
    check_ordered(ex, case, path, why, heavy_opt)
    assert len(case.note["heavy"]) == min(2048, 2048 // S.shape_na(shape))


@pytest.mark.parametrize("shape,heavy_opt", [("count", 1), ("one", 1), ("one", 2)])
def test_cuckoo_neighbours(ex, orc, opts, shape, heavy_opt):
    """kept keys whose two slots both name heavy keys stay kept; heavy keys in their second slot are
    found (the heavy rows are exact)"""
    opts(gb_heavy=heavy_opt)
    case, kd = get_case(ex, S.cuckoo_neighbours, S.shape_na(shape))
    path, why = run_case(ex, orc, case, kd, shape)
    check_ordered(ex, case, path, why, heavy_opt)


TAIL_SHAPES = [(0, False, "count"), (0, True, "one"), (1, True, "keyval"), (1, False, "three"), (2047, True, "four"),
               (2049, False, "one"), (4099, True, "count")]


@pytest.mark.parametrize("tail,last_heavy,shape", TAIL_SHAPES)
def test_heavy_blocks(ex, orc, tail, last_heavy, shape):
    """tiles and workgroups that keep nothing, one row, every other row; block edges in mid-tile; a
    last tile of 1, 2047, 2049 (+ 2048) rows whose last row is heavy or kept"""
    case, kd = get_case(ex, S.heavy_blocks, tail, last_heavy)
    path, why = run_case(ex, orc, case, kd, shape)
    check_ordered(ex, case, path, why)


@pytest.mark.parametrize("tail,last_heavy,shape", [(0, False, "one"), (1, True, "three"), (2049, False, "count"),
                                                   (4099, True, "four")])
def test_heavy_blocks_capped(ex, orc, opts, tail, last_heavy, shape):
    """the same placements with the capped layout behind the heavy pass (gb_heavy = 2)"""
    opts(gb_heavy=2)
    case, kd = get_case(ex, S.heavy_blocks, tail, last_heavy)
    path, why = run_case(ex, orc, case, kd, shape)
    check_ordered(ex, case, path, why, 2)


@pytest.mark.parametrize("shape,option", [("count", {}), ("one", {}), ("keyval", {}), ("three", {}), ("four", {}),
                                          ("one", dict(gb_heavy=2)), ("one", dict(gb_l0_bits=6)),
                                          ("three", dict(gb_l0_bits=8)), ("one", dict(gb_l1_threads=512))])
def test_gap(ex, orc, opts, shape, option):
    """heavy keys the host folds (hq = -1) beside heavy keys inserted below, above, alone and in pairs
    in their partitions"""
    opts(**option)
    case, kd = get_case(ex, S.gap)
    path, why = run_case(ex, orc, case, kd, shape)
    check_ordered(ex, case, path, why, option.get("gb_heavy", 1))


@pytest.mark.parametrize("shape", ["id_i64", "id_f64"])
@pytest.mark.parametrize("heavy_opt", [1, 2])
def test_identity_values(ex, orc, opts, shape, heavy_opt):
    """a heavy key whose every accumulator ends equal to its initial word (the merge skips those)"""
    opts(gb_heavy=heavy_opt)
    case, kd = get_case(ex, S.identity_keys)
    path, why = run_case(ex, orc, case, kd, shape)
    check_ordered(ex, case, path, why, heavy_opt)


# ----------------------------------------------------------------------------- keys the sample never saw
@pytest.mark.parametrize("with_heavy,shape,heavy_opt", [(False, "one", 1), (False, "three", 1), (True, "one", 1),
                                                        (True, "one", 2)])
def test_hidden_key(ex, orc, opts, with_heavy, shape, heavy_opt):
    """3 % of the rows on a key the sample missed: the arenas under the capped layout, one huge cell
    under the exact one"""
    opts(gb_heavy=heavy_opt)
    case, kd = get_case(ex, S.hidden_key, 8, with_heavy)
    path, why = run_case(ex, orc, case, kd, shape)
    check_ordered(ex, case, path, why, heavy_opt)


@pytest.mark.parametrize("geom", ["full", "dense", "negative", "straddle", "tiny"])
def test_outliers(ex, orc, geom):
    """keys outside [lo, lo + span] clamp to cells 0 and 16383 (INT64_MIN and INT64_MAX among them);
    dense ids order with sh = 0"""
    case, kd = get_case(ex, *((S.tiny_span,) if geom == "tiny" else (S.outliers, geom)))
    path, why = run_case(ex, orc, case, kd, "keyval" if geom == "dense" else "one")
    check_ordered(ex, case, path, why)


# ----------------------------------------------------------------------------- declines
@pytest.mark.parametrize("which", ["arena_level0", "arena_level1", "table", "capacity", "capacity_neighbour", "span",
                                   "clustered"])
def test_declines(ex, orc, which):
    """the reasons after work has started — "arena" (either level), "table", "capacity" beside its
    neighbour that fits (the digit counts come from nut_groupby_layout: fewest_digits) — and before
    it: a sampled span below 2^16 ("shape"), "clustered".  The hashed path gives the oracle's result."""
    if which.startswith("capacity"):
        d = S.fewest_digits(S.shape_na("one"))
        fits = which == "capacity_neighbour"
        builder, args = S.few_digits, (d if fits else d - 1, fits)
    else:
        builder, args = {"arena_level0": (S.arena_level0, ()), "arena_level1": (S.arena_level1, ()),
                         "table": (S.table_overflow, ()), "span": (S.tiny_span, (False,)),
                         "clustered": (S.clustered, ())}[which]
    case, kd = get_case(ex, builder, *args)
    path, why = run_case(ex, orc, case, kd, "one")
    if case.note["decline"] == "none":
        check_ordered(ex, case, path, why)
    else:
        assert path != S.ORDERED and why == case.note["decline"]


def test_admission_edges(ex, orc):
    """n = 2^24 - 1 / 2^24, group_hint = 100 x 16384 - 1 / 100 x 16384, n = 4 hint - 1 / 4 hint, and a
    key column sliced by one row (8-byte aligned only)"""
    case, kd = get_case(ex, S.plain)
    host, devc = get_values(ex, "one", case, kd)
    ok, ow = oracle_of(orc, case, "one", host)
    out = (pinned(len(ok) + 64, 1), pinned(len(ok) + 64, 4))

    def run(q, hint):
        k, w = ex.groupby_to_host(q, group_hint=hint, out=out)
        return k.copy(), w.copy().view(np.uint64), ex.groupby_stats()["path"], ex.groupby_declined()
    for hint, want in ((S.HINT, "none"), (S.HINT - 1, "shape"), (S.N0 // 4, "none"), (S.N0 // 4 + 1, "shape")):
        k, w, path, why = run(query_of("one", kd, devc), hint)
        assert why == want and (path == S.ORDERED) == (want == "none"), hint
        assert np.array_equal(k, ok) and np.array_equal(w, ow)
    # one row fewer
    k, w, path, why = run(query_of("one", kd[:-1], [devc[0][:-1]]), S.HINT)
    assert why == "shape" and path != S.ORDERED
    sk, sw = orc.groupby([case.keys[:-1]], S.oracle_aggs("one"), values=[host[0][:-1]])
    assert np.array_equal(k, sk) and np.array_equal(w, sw)
    # 2^24 rows from row 1 of a longer column: the key column is 8-byte aligned only
    keys1 = np.concatenate([case.keys[-1:], case.keys])
    kd1 = torch.from_numpy(keys1).to(ex.device)
    assert kd1.data_ptr() % 16 == 0
    k, w, path, why = run(query_of("one", kd1[1:], devc), S.HINT)
    assert why == "shape" and path != S.ORDERED
    assert np.array_equal(k, ok) and np.array_equal(w, ow)


# ----------------------------------------------------------------------------- the capacity contract
def to_host_raw(ex, q, hint, keys, aggs, cap):
    """nut_groupby_to_host with `cap` below the arrays' rows -> (status, *n_out)"""
    from nutdb_amd._lib import lib
    spec = q.to_spec(ex.device)
    ex._bind_stream()
    n = C.c_uint64()
    st = lib.nut_groupby_to_host(ex.ctx, C.byref(spec), hint, keys.ctypes.data, aggs.ctypes.data, cap, C.byref(n))
    return st, n.value


PATTERN = 0x5A5A5A5A5A5A5A5A


@pytest.mark.parametrize("which", ["gap", "arenas", "gap_arenas"])
def test_capacity_contract(ex, orc, opts, which):
    """nutexec.h: on NUT_ERR_CAPACITY *n_out is the room needed.  cap = G succeeds; every smaller cap
    reports G, whichever stage overflows first — the device-ordered part (cap = G / 2), the arena
    fold, or the heavy keys' fold (cap = G - 1 overflows in the last stage that adds a group; with
    four fold-only heavy keys, G - 5 overflows before their fold) — leaves the rows from cap on
    untouched, and a retry with exactly *n_out rows succeeds."""
    from nutdb_amd._lib import NUT_ERR_CAPACITY
    if which == "gap":              # exact layout: four heavy keys that only the host's fold adds
        case, kd = get_case(ex, S.gap)
    elif which == "arenas":         # capped layout, no heavy pass: the arena fold
        case, kd = get_case(ex, S.hidden_key, 8, False)
    else:                           # capped layout behind the heavy pass: both folds
        opts(gb_heavy=2)
        case, kd = get_case(ex, S.gap, 18, 6, True)
    host, devc = get_values(ex, "one", case, kd)
    q = query_of("one", kd, devc)
    ok, ow = oracle_of(orc, case, "one", host)
    G = len(ok)
    keys, aggs = pinned(G + 64, 1), pinned(G + 64, 4)

    def fill():
        keys[:] = PATTERN
        aggs[:] = PATTERN
    fill()
    st, n = to_host_raw(ex, q, case.hint, keys, aggs, G)
    assert (st, n) == (0, G) and ex.groupby_stats()["path"] == S.ORDERED
    assert np.array_equal(keys[:G], ok) and np.array_equal(aggs[:G].view(np.uint64), ow)
    assert np.all(keys[G:] == PATTERN) and np.all(aggs[G:] == PATTERN)
    if which != "gap":
        assert ex.groupby_overflow_rows() > 0
    for cap in (G - 1, G - 5, G // 2):
        fill()
        st, n = to_host_raw(ex, q, case.hint, keys, aggs, cap)
        print(f"{case.name}: cap {cap} of {G} groups -> status {st}, n_out {n}")
        assert st == NUT_ERR_CAPACITY and ex.groupby_stats()["path"] == S.ORDERED, cap
        assert n == G, (cap, n, G)
        assert np.all(keys[cap:] == PATTERN) and np.all(aggs[cap:] == PATTERN), cap
        k2, a2 = pinned(n, 1), pinned(n, 4)
        st2, n2 = to_host_raw(ex, q, case.hint, k2, a2, n)
        assert (st2, n2) == (0, G) and np.array_equal(k2, ok) and np.array_equal(a2.view(np.uint64), ow), cap


def test_auto_size_beyond_first_arrays(ex, orc):
    """groupby_to_host(out=None): 3.67 M groups under the smallest hint, whose first arrays (2 x hint
    rows) are too small — the device-ordered part overflows with four fold-only heavy keys still to
    come; the second arrays, sized from *n_out, must hold the oracle's result"""
    case, kd = get_case(ex, S.gap, 22, 7, False)
    assert case.note["groups"] > 2 * case.hint
    host, devc = get_values(ex, "one", case, kd)
    ok, ow = oracle_of(orc, case, "one", host)
    k, w = ex.groupby_to_host(query_of("one", kd, devc), group_hint=case.hint)
    assert ex.groupby_stats()["path"] == S.ORDERED
    assert ex.groupby_heavy() == (12, case.note["heavy_rows"])
    assert np.array_equal(k, ok) and np.array_equal(w, ow)
