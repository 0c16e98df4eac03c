"""Every branch of the group-by tables (csrc/agg_kernel.hpp, csrc/gtable.hpp) on directed
inputs, bit-exact against the oracle (oracle.groupby): keys, counts, MIN, MAX and the f64
sums (dyadic values: every sum is exact in any order) compared with np.array_equal — there
is no tolerance in this file.

tests/groupby_shapes.py builds the inputs — keys with a chosen home bucket, slot word, slot,
tag, shard, owner or partition digit, since every hash of the tables is invertible — and
tests/test_groupby_shapes_cpu.py proves, against the library's own layout arithmetic
(nut_groupby_layout), that they hold what they claim.  DESIGN.md §4.2e maps each kernel
branch to its case.  Rows come round-robin over the keys (every wave meets every new key at
once: claim contention) and blocked (a wave's lanes carry one key: same-address fold
atomics), at 1..5 and 4099 rows (each lane at most its guarded last step) and, for the
on-chip cases, at a row count taken from the exported launch arithmetic at which every lane
runs three or four full steps of the main loop (groupby_shapes.loop_rows).

Kernels: the compiled SUM/COUNT/MIN/MAX shape with vector loads ("all4"), the generic kernel
on columns sliced by one row ("generic": 8-byte aligned, scalar loads), a run-time compiled
kernel with a computed key k + 0 ("expr"), and on A2, A3 and A5 the compiled SUM and
SUM/COUNT shapes; two keys: the generic kernel, the Q1 shape, and a private run-time
compiled kernel.  The oracle's result is computed once per input."""
import numpy as np
import pytest
import torch

import groupby_shapes as S
from test_gpu_exec import dev

pytestmark = pytest.mark.gpu

I64_MIN = S.I64_MIN
AGGS4 = [(0, 0, (0,)), (1, 0, ()), (2, 0, (0,)), (3, 0, (0,))]         # oracle: SUM, COUNT, MIN, MAX of v0
Q1_AGGS = [(0, 0, (0,)), (0, 0, (1,)), (0, 4, (1, 2)), (1, 0, ())]     # SUM v0, SUM v1, SUM v1 (1 - v2), COUNT
Q1_K = 10471
KEY_PLUS_0 = lambda c: [("col", c), ("i64", 0, 0), ("add",)]           # noqa: E731
FORMS1 = ("all4", "generic", "expr")
FORMS2 = ("generic2", "q1")


def sliced(x, ex):
    """The column at an 8-byte aligned, not 16-byte aligned address."""
    t = torch.empty(len(x) + 1, dtype=torch.from_numpy(x[:0]).dtype, device=ex.device)
    t[1:] = torch.from_numpy(np.ascontiguousarray(x))
    assert t[1:].data_ptr() % 16 == 8
    return t[1:]


class Inputs:
    """Rows of (case, n, order): host and device columns and the oracle's results, made once."""

    def __init__(self, ex, orc):
        self.ex, self.orc, self.seen = ex, orc, {}

    def get(self, case, n, order):
        k = (id(case), n, order)
        if k not in self.seen:
            keys, v = S.rows(case, n, order)
            self.seen[k] = {"case": case, "keys": keys, "v": v, "n": n}
        return self.seen[k]

    def oracle(self, inp, what):
        if what not in inp:
            if what == "aggs4":
                inp[what] = self.orc.groupby(inp["keys"], AGGS4, values=[inp["v"]])
            elif what == "q1":
                inp[what] = self.orc.groupby(inp["keys"], Q1_AGGS, values=inp["q1_vals"], preds=[(inp["q1_date"], 1, Q1_K)])
            elif what == "ints":
                inp[what] = self.orc.groupby(inp["keys"], [(0, 0, (0,)), (2, 0, (0,)), (3, 0, (0,)), (1, 0, ())],
                                             values=[inp["iv"]])
        return inp[what]

    def device(self, inp, name, make):
        if name not in inp:
            inp[name] = make()
        return inp[name]


@pytest.fixture(scope="module")
def inputs(ex, orc):
    return Inputs(ex, orc)


def same(got, want, what):
    gk, gw = got
    wk, ww = want
    assert gk.shape == wk.shape and np.array_equal(gk, wk), (what, "keys", gk.shape, wk.shape)
    assert np.array_equal(np.asarray(gw).view(np.uint64), np.asarray(ww).view(np.uint64)), (what, "aggregates")


def query(ex, inputs, inp, form):
    """(query, oracle result) of one kernel form over an input."""
    from nutdb_amd import Agg, AggQuery, ProgQuery
    a4 = [Agg("sum", "col", (0,)), Agg("count"), Agg("min", "col", (0,)), Agg("max", "col", (0,))]
    d = lambda name, x: inputs.device(inp, "dev_" + name, lambda: dev(x, ex))       # noqa: E731
    keys = [d(f"k{i}", k) for i, k in enumerate(inp["keys"])]
    if form in ("all4", "generic2"):
        return AggQuery(keys=keys, values=[d("v", inp["v"])], aggs=a4), inputs.oracle(inp, "aggs4")
    if form in ("sum", "sumcount"):
        ok, ow = inputs.oracle(inp, "aggs4")
        m = 1 if form == "sum" else 2
        return AggQuery(keys=keys, values=[d("v", inp["v"])], aggs=a4[:m]), (ok, ow[:, :m])
    if form == "generic":
        ks = [inputs.device(inp, f"ks{i}", lambda k=k: sliced(k, ex)) for i, k in enumerate(inp["keys"])]
        vs = inputs.device(inp, "vs", lambda: sliced(inp["v"], ex))
        return AggQuery(keys=ks, values=[vs], aggs=a4), inputs.oracle(inp, "aggs4")
    if form in ("expr", "expr2"):
        nk = len(keys)
        v = ("col", nk)
        aggs = [("sum", [v], None), ("count", None, None), ("min", [v], None), ("max", [v], None)]
        q = ProgQuery(keys=[KEY_PLUS_0(0)] + keys[1:], cols=[keys[0]] + keys[1:] + [d("v", inp["v"])], aggs=aggs)
        return q, inputs.oracle(inp, "aggs4")
    if form == "ints":
        if "iv" not in inp:
            inp["iv"] = S.wrapping(inp["n"], 3)
        q = AggQuery(keys=keys, values=[d("div", inp["iv"])],
                     aggs=[Agg("sum", "col", (0,)), Agg("min", "col", (0,)), Agg("max", "col", (0,)), Agg("count")])
        return q, inputs.oracle(inp, "ints")
    assert form == "q1"
    if "q1_vals" not in inp:
        rng = np.random.default_rng([inp["n"], 17])
        n = inp["n"]
        # quantity: dyadic; price: multiples of 2^-5 below 2^10; discount: multiples of 2^-5 in [0, 1) — the product
        # price x (1 - discount) is an exact multiple of 2^-10 and every sum is exact
        inp["q1_vals"] = [inp["v"], rng.integers(0, 1 << 15, n) / 32.0, rng.integers(0, 32, n) / 32.0]
        inp["q1_date"] = rng.integers(Q1_K - 50, Q1_K + 10, n).astype(np.int64)
    vals = [d(f"q1v{i}", x) for i, x in enumerate(inp["q1_vals"])]
    q = AggQuery(keys=keys, values=vals, preds=[(d("q1d", inp["q1_date"]), "<=", Q1_K)],
                 aggs=[Agg("sum", "col", (0,)), Agg("sum", "col", (1,)), Agg("sum", "mul_1m", (1, 2)), Agg("count")])
    return q, inputs.oracle(inp, "q1")


def run(ex, inputs, case, hint, forms, sizes, orders=S.ORDERS):
    """Every form over every (rows, order) of a case, each against the oracle; len() too."""
    for n in sizes:
        for order in (orders if n > 5 else orders[:1]):
            inp = inputs.get(case, n, order)
            for form in forms:
                q, want = query(ex, inputs, inp, form)
                g = ex.groupby(q, group_hint=hint)
                what = f"{case.name} ({case.note}): hint {hint}, {n} rows {order}, {form}"
                assert len(g) == len(want[0]), what
                same(g.to_host_words(), want, what)
                g.free()
            if n > 10000:          # a loop-size input is used by one run: free its columns
                del inputs.seen[(id(case), n, order)]


def loop_rows(ex, nk, na, hint, expr=0, agg_blocks=1):
    """The row count at which every lane of this launch runs at least three full steps
    (proven from the same figures in tests/test_groupby_shapes_cpu.py)."""
    o = S.library_layout(nk, na, hint, num_cus=ex.info()["num_cus"], agg_blocks=agg_blocks, expr=expr, n=1 << 40)
    return S.loop_rows(o["blocks"], o["threads"])


def lds(nk, na, hint):
    return S.library_layout(nk, na, hint)["lds_cap"]


# ----------------------------------------------------------------------------- A: single-key on-chip table
TABLE_HINTS = (9, 0, 4096)      # 64 slots (limit 48); no hint; the largest table the aggregates allow


@pytest.mark.parametrize("hi", S.HIS, ids=["hi0", "hineg"])
@pytest.mark.parametrize("hint", TABLE_HINTS)
@pytest.mark.parametrize("builder", [S.a1_bucket, S.a2_chain, S.a3_wrap, S.a4_behind], ids=["A1", "A2", "A3", "A4"])
def test_single_key_buckets_and_chains(ex, inputs, builder, hint, hi):
    """A1 a hit at each slot of the home bucket; A2 the inline probe past the bucket, l_walk
    and the CAS claim walking through other keys of the chain; A3 the wrap at the table's
    end; A4 a key behind two full buckets."""
    run(ex, inputs, builder(lds(1, 4, hint), hi), hint, FORMS1, S.TAIL_ROWS)


@pytest.mark.parametrize("hint", TABLE_HINTS)
@pytest.mark.parametrize("builder", [S.a2_chain, S.a3_wrap], ids=["A2", "A3"])
def test_single_key_chains_sum_shapes(ex, inputs, builder, hint):
    """The compiled SUM and SUM/COUNT shapes (their own tables: one or two aggregates)."""
    for form, na in (("sum", 1), ("sumcount", 2)):
        run(ex, inputs, builder(lds(1, na, hint)), hint, (form,), S.TAIL_ROWS)


@pytest.mark.parametrize("builder", [S.a1_bucket, S.a2_chain, S.a3_wrap, S.a4_behind], ids=["A1", "A2", "A3", "A4"])
def test_single_key_chains_main_loop(ex, inputs, opts, builder):
    """The same chains with every lane in the main loop (TAIL = false loads and folds)."""
    opts(agg_blocks=1)
    run(ex, inputs, builder(64), 9, FORMS1, [loop_rows(ex, 1, 4, 9)], orders=S.ORDERS if builder is S.a2_chain else S.ORDERS[:1])
    if builder is S.a3_wrap:
        run(ex, inputs, builder(lds(1, 4, 4096)), 4096, ("all4",), [loop_rows(ex, 1, 4, 4096)], orders=S.ORDERS[:1])
        run(ex, inputs, builder(lds(1, 1, 4096)), 4096, ("sum",), [loop_rows(ex, 1, 1, 4096)], orders=S.ORDERS[:1])
        run(ex, inputs, builder(64), 9, ("sumcount",), [loop_rows(ex, 1, 2, 9)], orders=S.ORDERS[:1])


@pytest.mark.parametrize("K", [48, 49, 64, 200])
def test_single_key_admission_limit(ex, inputs, opts, K):
    """A5: 48 keys are admitted, the 49th is not (CTL_CLAIMED >= limit), 64 and 200 exceed
    the slots: the rest of the rows fold into the global table (g_row)."""
    run(ex, inputs, S.a5_count(K), 9, FORMS1 + ("sum", "sumcount", "ints"), S.TAIL_ROWS[-1:])
    if K in (49, 200):
        opts(agg_blocks=1)
        run(ex, inputs, S.a5_count(K), 9, ("all4", "sum"), [loop_rows(ex, 1, 4, 9)], orders=S.ORDERS[:1])


@pytest.mark.parametrize("hint", TABLE_HINTS)
def test_single_key_extremes_and_equal_folds(ex, inputs, opts, hint):
    """A6: the empty-marker key (the special slot), INT64_MAX, -1 and 0 beside a chain;
    A7: keys with swapped halves (equal fold, equal home, different keys)."""
    run(ex, inputs, S.a6_extremes(lds(1, 4, hint)), hint, FORMS1 + ("ints",), S.TAIL_ROWS)
    run(ex, inputs, S.a7_swapped_halves(), hint, FORMS1, S.TAIL_ROWS[-1:])
    if hint == 9:
        opts(agg_blocks=1)
        n = loop_rows(ex, 1, 4, 9)
        run(ex, inputs, S.a6_extremes(64), 9, FORMS1, [n], orders=S.ORDERS[:1])     # the marker key in the main loop
        run(ex, inputs, S.a7_swapped_halves(), 9, ("all4",), [n], orders=S.ORDERS[:1])


def test_no_on_chip_table(ex, inputs):
    """A8: a hint above 8 x the largest table: no LDS table, every row through g_row."""
    c = S.a8_no_table(4)
    run(ex, inputs, c, c.hint, FORMS1, S.TAIL_ROWS)
    assert ex.groupby_stats()["path"] == "onchip"


# ----------------------------------------------------------------------------- B: two-key on-chip table
TABLE_HINTS2 = (9, 0, 8)        # 64 slots shared; no hint; 32 slots with private accumulators


def forms2(hint):
    return FORMS2 + (("expr2",) if hint == 8 else ())


@pytest.mark.parametrize("hint", TABLE_HINTS2)
@pytest.mark.parametrize("across", [False, True], ids=["bucket", "across"])
@pytest.mark.parametrize("m", [2, 3])
def test_two_key_equal_slot_words(ex, inputs, m, across, hint):
    """B1: unequal tuples with one slot word: keys_match misses in the home bucket (s = -1,
    end = false), in the inline probe and in l_walk."""
    run(ex, inputs, S.b1_same_word(lds(2, 4, hint), m, across), hint, forms2(hint), S.TAIL_ROWS)


@pytest.mark.parametrize("hint", TABLE_HINTS2)
def test_two_key_nudge_limit_and_chains(ex, inputs, hint):
    """B2: the tuple whose hash is the empty marker (nudged) beside the tuple that hashes to
    the nudged word; B3: more tuples than the limit; B4: a chain and a wrapped chain."""
    run(ex, inputs, S.b2_nudged(), hint, forms2(hint), S.TAIL_ROWS)
    cap = lds(2, 4, hint)
    for wrap in (False, True):
        run(ex, inputs, S.b4_chain(cap, wrap), hint, forms2(hint), S.TAIL_ROWS[-1:])
    for K in (cap - cap // 4, cap - cap // 4 + 1, 200):
        run(ex, inputs, S.b3_count(K), hint, forms2(hint), S.TAIL_ROWS[-1:])


def test_two_key_main_loop(ex, inputs, opts):
    """B1, B2 and the wrapped B4 with every lane in the main loop: shared tables (generic and
    Q1 shape) and private ones (generic, compiled Q1, run-time compiled)."""
    opts(agg_blocks=1)
    n = loop_rows(ex, 2, 4, 9)
    for c in (S.b1_same_word(64, 3, True), S.b2_nudged(), S.b4_chain(64, True)):
        run(ex, inputs, c, 9, FORMS2, [n], orders=S.ORDERS[:1])
    # at the tail sizes nearly every lane loads its bucket before anything is inserted and goes through
    # l_find_slow; the home-bucket miss on an equal word needs rows that come after the insert
    for c in (S.b1_same_word(64, 2, False), S.b1_same_word(64, 3, False), S.b1_same_word(64, 2, True)):
        run(ex, inputs, c, 9, ("generic2",), [n], orders=S.ORDERS[1:])
    run(ex, inputs, S.b1_same_word(32, 3, True), 8, ("generic2",), [loop_rows(ex, 2, 4, 8, agg_blocks=0)], orders=S.ORDERS[:1])
    run(ex, inputs, S.b1_same_word(32, 3, True), 8, ("q1", "expr2"), [loop_rows(ex, 2, 4, 8, expr=1, agg_blocks=0)],
        orders=S.ORDERS[:1])


# ----------------------------------------------------------------------------- C: private accumulators, direct map
def test_private_direct_map_edges(ex, inputs):
    """C1 / C2: keys on both sides of the direct map's range."""
    run(ex, inputs, S.c1_direct_edge(), 8, ("all4", "generic", "ints"), S.TAIL_ROWS)
    run(ex, inputs, S.c2_direct_edge(), 8, FORMS2 + ("expr2",), S.TAIL_ROWS)
    run(ex, inputs, S.c1_direct_edge(), 8, ("all4", "generic"), [loop_rows(ex, 1, 4, 8, agg_blocks=0)], orders=S.ORDERS[:1])
    run(ex, inputs, S.c2_direct_edge(), 8, ("generic2",), [loop_rows(ex, 2, 4, 8, agg_blocks=0)], orders=S.ORDERS[:1])
    run(ex, inputs, S.c2_direct_edge(), 8, ("q1", "expr2"), [loop_rows(ex, 2, 4, 8, expr=1, agg_blocks=0)], orders=S.ORDERS[:1])


def test_private_ids_run_out(ex, inputs):
    """C3: hint 3 with 6 groups: three take private ids, the others fold in the table (and
    must not be given a direct-map entry)."""
    c = S.c3_ids_run_out()
    run(ex, inputs, c, 3, ("all4", "generic", "ints"), S.TAIL_ROWS)
    run(ex, inputs, c, 3, ("all4",), [loop_rows(ex, 1, 4, 3, agg_blocks=0)], orders=S.ORDERS[1:])


def test_private_cut_off(ex, inputs):
    """C4: hint 8 with four aggregates runs private accumulators, with five the shared table
    (the private layout would take more than half the LDS budget)."""
    from nutdb_amd import Agg, AggQuery
    c = S.c4_cutoff()
    assert S.library_layout(1, 4, 8)["priv"] == 8 and S.library_layout(1, 5, 8)["priv"] == 0
    run(ex, inputs, c, 8, ("all4", "generic"), S.TAIL_ROWS)
    for n in S.TAIL_ROWS:
        inp = inputs.get(c, n, "round_robin")
        iv = S.wrapping(n, 5)
        q = AggQuery(keys=[dev(inp["keys"][0], ex)], values=[dev(inp["v"], ex), dev(iv, ex)],
                     aggs=[Agg("sum", "col", (0,)), Agg("count"), Agg("min", "col", (0,)), Agg("max", "col", (0,)),
                           Agg("sum", "col", (1,))])
        want = inputs.orc.groupby(inp["keys"], AGGS4 + [(0, 0, (1,))], values=[inp["v"], iv])
        same(ex.groupby(q, group_hint=8).to_host_words(), want, f"C4, five aggregates, {n} rows")


# ----------------------------------------------------------------------------- D: global table
def test_global_run_across_the_table_end(ex, inputs):
    """D1: 100 keys homed at slot 1020 of 1024: g_find wraps and walks more than 63 occupied
    slots (the overflow-flag check on the way, with the flag clear)."""
    c = S.d1_long_run()
    run(ex, inputs, c, c.hint, FORMS1 + ("ints",), S.TAIL_ROWS)


@pytest.mark.parametrize("K", [768, 769, 3073])
def test_global_regrow(ex, inputs, K):
    """D2: hint 1 (1024 slots): 768 keys fit, the 769th claim flags overflow (one regrow),
    3073 keys flag it again at 4096 slots (two regrows)."""
    run(ex, inputs, S.d2_regrow(K), 1, FORMS1, S.TAIL_ROWS[-1:])


@pytest.mark.parametrize("K", [816, 817])
def test_global_claim_shard_limit(ex, inputs, K):
    """D3: a 2^18-slot table (sharded counters, no on-chip table, too few rows to partition):
    816 claims in one shard fit, the 817th flags overflow in a nearly empty table."""
    c = S.d3_claim_shard(K)
    run(ex, inputs, c, c.hint, FORMS1, S.TAIL_ROWS[-1:])
    assert ex.groupby_stats()["path"] == "onchip"


@pytest.mark.parametrize("hint", [16, 8])
def test_global_two_key_collisions(ex, inputs, hint):
    """D4: tuples with one 64-bit hash (same slot, same tag: only the arena compare tells
    them apart); D5: one tag and two slots, one slot and two tags."""
    for c in (S.d4_same_hash(2), S.d4_same_hash(3), S.d5_tag_and_slot(1024)):
        run(ex, inputs, c, hint, forms2(hint), S.TAIL_ROWS)


@pytest.mark.parametrize("K", [1280, 1281])
def test_global_arena_shard_limit(ex, inputs, K):
    """D6: 1280 tuples in one arena shard of a 2^18-slot table, and one more (the shard's
    arena runs out: overflow, a larger table)."""
    c = S.d6_arena_shard(K)
    run(ex, inputs, c, c.hint, ("generic2", "q1"), S.TAIL_ROWS[-1:])


# ----------------------------------------------------------------------------- E: compaction, owner partition
def check_partition(ex, g, nk, P, want, what):
    """nut_groups_partition: every group in its owner's segment, the segments together the
    oracle's result."""
    buf, counts = g.partition(P)
    w = nk + 4
    assert sum(counts) == len(want[0]), what
    rows, off = [], 0
    for p in range(P):
        if counts[p]:
            seg = buf[w * off: w * (off + counts[p])].view(w, counts[p]).cpu().numpy()
            own = S.owner_hash(nk, seg[0], seg[1] if nk == 2 else 0) % np.uint64(P)
            assert np.all(own == np.uint64(p)), (what, p)
            rows.append(seg.T)
        off += counts[p]
    t = np.concatenate(rows)
    t = t[np.lexsort([t[:, i] for i in range(nk - 1, -1, -1)])]
    same((t[:, :nk], np.ascontiguousarray(t[:, nk:])), want, what)
    return counts


@pytest.mark.parametrize("cap", [2048, 4096])
def test_compaction_special_slot_chunk(ex, inputs, cap):
    """E1: the empty-marker key's slot (index cap) is the first of a compaction chunk."""
    c = S.e1_special_chunk(cap)
    run(ex, inputs, c, c.hint, ("all4",), S.TAIL_ROWS[-1:], orders=S.ORDERS[:1])
    inp = inputs.get(c, S.TAIL_ROWS[-1], "round_robin")
    q, want = query(ex, inputs, inp, "all4")
    g = ex.groupby(q, group_hint=c.hint)
    for P in (1, 2):
        check_partition(ex, g, 1, P, want, f"E1 cap {cap}, {P} parts")


@pytest.mark.parametrize("nk", [1, 2])
@pytest.mark.parametrize("P", [1, 2, 64])
def test_owner_partition(ex, inputs, nk, P):
    """E2: every group owned by one part (the others empty), and one group per part."""
    for spread in (False, True):
        c = S.e2_owners(nk, P, spread)
        inp = inputs.get(c, 1001, "round_robin")
        q, want = query(ex, inputs, inp, "all4" if nk == 1 else "generic2")
        g = ex.groupby(q, group_hint=c.hint)
        counts = check_partition(ex, g, nk, P, want, f"{c.name} ({c.note})")
        assert counts == ([1] * P if spread else [0] * (P - 1) + [40])


# ----------------------------------------------------------------------------- F: accumulate
def accumulate(ex, g, keys, v):
    """Raw rows as partials: COUNT partials merge as sums of ones."""
    from nutdb_amd import Agg, AggQuery
    ones = np.ones(len(v), dtype=np.int64)
    ex.accumulate(AggQuery(keys=[dev(k, ex) for k in keys], values=[dev(v, ex), dev(ones, ex)],
                           aggs=[Agg("sum", "col", (0,)), Agg("sum", "col", (1,)), Agg("min", "col", (0,)),
                                 Agg("max", "col", (0,))]), g)


def test_accumulate_across_the_limit(ex, inputs, orc):
    """F1: new keys accumulated past the table's limit: ensure_room rehashes D1's run, the
    special slot and (two keys) D4's collided tuples into a larger table (rehash_kernel)."""
    from nutdb_amd import Agg, AggQuery
    a4 = [Agg("sum", "col", (0,)), Agg("count"), Agg("min", "col", (0,)), Agg("max", "col", (0,))]
    first = S.case_of("F1", [np.concatenate([S.d1_long_run().keys[0], [I64_MIN]])], S.D1_HINT, "D1's run and the special key")
    new = S.d2_regrow(769)
    k0, v0 = S.rows(first, 4099, "round_robin")
    k1, v1 = S.rows(new, 4099, "blocked", seed=1)
    assert S.library_layout(1, 4, S.D1_HINT)["limit"] == 768 < len(first.keys[0]) + 4099      # ensure_room must grow
    g = ex.groupby(AggQuery(keys=[dev(k0[0], ex)], values=[dev(v0, ex)], aggs=a4), group_hint=S.D1_HINT)
    assert len(g) == 101
    accumulate(ex, g, k1, v1)
    accumulate(ex, g, k0, v0)                      # and the old keys again, found in the new table
    want = orc.groupby([np.concatenate([k0[0], k1[0], k0[0]])], AGGS4, values=[np.concatenate([v0, v1, v0])])
    assert len(g) == 101 + 769
    same(g.to_host_words(), want, "F1, one key")
    # two keys: D4's equal-hash tuples move through the rehash
    first = S.d4_same_hash(3)
    new = S.b3_count(200)
    k0, v0 = S.rows(first, 1001, "round_robin")
    k1, v1 = S.rows(new, 4099, "round_robin", seed=2)
    g = ex.groupby(AggQuery(keys=[dev(k, ex) for k in k0], values=[dev(v0, ex)], aggs=a4), group_hint=16)
    accumulate(ex, g, k1, v1)
    accumulate(ex, g, k0, v0)
    want = orc.groupby([np.concatenate([a, b, a]) for a, b in zip(k0, k1)], AGGS4, values=[np.concatenate([v0, v1, v0])])
    same(g.to_host_words(), want, "F1, two keys")


# ----------------------------------------------------------------------------- G: segment mode
def segment_opts(ex, opts):
    """One level of 256 partitions, one workgroup each: their groups are final in the block
    (the dense append) — as long as the device has no more than 256 compute units."""
    opts(gb_partition=1, gb_levels=1, gb_chunks=1, gb_l0_bits=S.SEG_BITS)
    assert ex.info()["num_cus"] <= 256


@pytest.mark.parametrize("K", [S.seg_limit(), S.seg_limit() + 1, 200])
def test_segment_partition_at_its_limit(ex, inputs, opts, K):
    """G2: a partition holding exactly its block table's limit (96 groups): the dense append.
    G1: one more, and 200 (more than the table's 128 slots): the block cannot hold its
    partition, flags it, and the launch reruns with the hashed merge.  F2: accumulating
    into the (dense) result rehashes it first."""
    segment_opts(ex, opts)
    c = S.g_partition(K)
    inp = inputs.get(c, 4099, "round_robin")
    q, want = query(ex, inputs, inp, "all4")
    g = ex.groupby(q, group_hint=c.hint)
    st = ex.groupby_stats()
    assert (st["path"], st["levels"]) == ("partitioned_direct", 1)
    assert len(g) == K + 255
    same(g.to_host_words(), want, f"G, {K} groups in one partition")
    k1, v1 = S.rows(S.d1_long_run(), 1001, "round_robin", seed=4)
    accumulate(ex, g, k1, v1)
    accumulate(ex, g, inp["keys"], inp["v"])
    want = inputs.orc.groupby([np.concatenate([inp["keys"][0], k1[0], inp["keys"][0]])], AGGS4,
                              values=[np.concatenate([inp["v"], v1, inp["v"]])])
    same(g.to_host_words(), want, f"F2, accumulate into the result of {K} groups in one partition")


# ----------------------------------------------------------------------------- results and their executor
def test_result_outlives_its_executor(orc):
    """A result still alive when its executor closes (a failed assertion's traceback keeps one
    until the interpreter exits) is freed by close(): freeing or collecting it afterwards
    must not hand its table to a context that is gone."""
    from nutdb_amd import Agg, AggQuery, Executor
    e2 = Executor(0)
    keys, v = S.rows(S.c1_direct_edge(), 101, "round_robin")
    g = e2.groupby(AggQuery(keys=[dev(keys[0], e2)], values=[dev(v, e2)],
                            aggs=[Agg("sum", "col", (0,)), Agg("count"), Agg("min", "col", (0,)), Agg("max", "col", (0,))]),
                   group_hint=8)
    same(g.to_host_words(), orc.groupby(keys, AGGS4, values=[v]), "before close")
    e2.close()
    assert not g.h
    g.free()
    del g
