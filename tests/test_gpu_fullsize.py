"""GPU parity at the BASELINE.json sizes (VERDICT r1 "What's weak" 1): the benchmarked
shapes themselves, not scaled-down stand-ins, checked against the C oracle.

- config 5: one full 1.25e9-key sort shard (the per-GPU share of 1e10 keys on 8 GPUs).
  At this size the hybrid MSD sort takes two scatter levels and its ~19 K-key segments
  run through the largest local-sort class — a segment mix no smaller test drives.
  Checked by sortedness + count + order-independent multiset hash against the oracle's
  hash of the same generated column (a full element compare would need a 10 GB CPU sort).
- config 3: GROUP BY key SUM(val) over 1e9 rows, G = 1000, dyadic values -> the f64 sums
  are exact, so the comparison is bit-exact.
- config 4: the TPC-H Q1 shape over 1e9 rows (keys / counts exact, f64 sums <= 1e-12), at
  the launch shape the probe keeps and at the two 128-thread shapes it chooses among.
- config 3 at large G (1e5 and 1e7 groups over 1e9 rows): the partitioned path the bench
  times (direct key-hash partitioning, one level at 1e5 and two at 1e7, optimistic level
  0), checked bit-exact against the indexed dense-array oracle (oracle.h
  orc_groupby_pool_dyadic), which takes seconds at this size.

Host memory: at most ~50 GB at a time (the Q1 columns), freed between tests.
"""
import gc

import numpy as np
import pytest

from helpers import F64_SUM_RTOL, OPCODE, rel_err

pytestmark = pytest.mark.gpu


def test_sort_full_config5_shard(ex, orc):
    from nutdb_amd.workloads import SORT_COL, gen
    n = 1_250_000_000
    keys = gen(ex, SORT_COL, n)
    out = ex.sort_i64(keys)
    nbytes, levels = ex.sort_stats()
    assert levels == 2 and nbytes >= 16 * n
    del keys
    o = out.cpu().numpy()
    del out
    assert len(o) == n
    assert bool(np.all(o[1:] >= o[:-1])), "not sorted"
    h = orc.multiset_hash(o)
    del o
    gc.collect()
    want = orc.gen(SORT_COL, n)
    assert h == orc.multiset_hash(want), "multiset hash differs from the generated column's"


def test_groupby_full_config3(ex, orc):
    from nutdb_amd import Agg, AggQuery
    from nutdb_amd.workloads import gen, groupby_cols
    n, G = 1_000_000_000, 1000
    specs = groupby_cols(G, dyadic=True)
    key, val = [gen(ex, s, n) for s in specs]
    g = ex.groupby(AggQuery(keys=[key], values=[val], aggs=[Agg("sum", "col", (0,)), Agg("count")]),
                   group_hint=G)
    gk, gw = g.to_host_words()
    g.free()
    del key, val
    hk, hv = [orc.gen(s, n) for s in specs]
    ok, ow = orc.groupby([hk], [(0, 0, (0,)), (1, 0, ())], values=[hv], cap=G)
    del hk, hv
    gc.collect()
    assert len(ok) == G
    assert np.array_equal(gk, ok)
    assert np.array_equal(gw, ow), "dyadic sums / counts must be bit-exact"
    assert int(gw[:, 1].sum()) == n


def test_q1_full_config4(ex, orc, opts):
    from nutdb_amd.workloads import Q1_COLS, Q1_DATE_K, gen
    n = 1_000_000_000
    cols = [gen(ex, spec, n) for spec in Q1_COLS]
    g = ex.q1(*cols, date_k=Q1_DATE_K)
    gk, gw = g.to_host_words()
    g.free()
    # the launch above ran the launch-shape probe (NUT_OPT_PRIV_PROBE) and the shape it kept
    # for this device; the two 128-thread candidates it chooses among, on the same columns
    forced = {}
    for blocks in (3, 4):
        opts(priv_bd=128, priv_blocks=blocks)
        shape = ex.priv_shape()
        assert (shape["threads"], shape["blocks_per_cu"]) == (128, blocks), shape
        g = ex.q1(*cols, date_k=Q1_DATE_K)
        forced[blocks] = g.to_host_words()
        g.free()
    del cols
    sd, rf, ls, qty, price, disc = [orc.gen(spec, n) for spec in Q1_COLS]
    ok, ow = orc.groupby([rf, ls], [(0, 0, (0,)), (0, 0, (1,)), (0, 4, (1, 2)), (1, 0, ())],
                         values=[qty, price, disc], preds=[(sd, OPCODE["<="], Q1_DATE_K)], cap=64)
    del sd, rf, ls, qty, price, disc
    gc.collect()
    assert np.array_equal(gk, ok)
    assert np.array_equal(gw[:, 3], ow[:, 3])
    for j in range(3):
        assert rel_err(gw[:, j].view(np.float64), ow[:, j].view(np.float64)) <= F64_SUM_RTOL
    for blocks, (fk, fw) in forced.items():
        assert np.array_equal(fk, ok), blocks
        assert np.array_equal(fw[:, 3], ow[:, 3]), blocks
        for j in range(3):
            assert rel_err(fw[:, j].view(np.float64), ow[:, j].view(np.float64)) <= F64_SUM_RTOL, (blocks, j)


@pytest.mark.parametrize("G,levels", [(100_000, 1), (10_000_000, 2)])
def test_groupby_full_config3_large_groups(ex, orc, G, levels):
    from nutdb_amd import Agg, AggQuery
    from nutdb_amd.workloads import gen, groupby_cols
    n = 1_000_000_000
    ks, vs = groupby_cols(G, dyadic=True)
    key, val = gen(ex, ks, n), gen(ex, vs, n)
    g = ex.groupby(AggQuery(keys=[key], values=[val], aggs=[Agg("sum", "col", (0,)), Agg("count"),
                                                             Agg("min", "col", (0,)), Agg("max", "col", (0,))]),
                   group_hint=G)
    st = ex.groupby_stats()
    gk, gw = g.to_host_words()
    g.free()
    del key, val
    # every level without a histogram pass (the capped layout held for these uniform keys)
    assert st == {"path": "partitioned_direct", "levels": levels, "optimistic": True, "capped_levels": levels}, st
    ok, ow = orc.groupby_pool_dyadic(G, n, key_seed=ks[2], val_seed=vs[2])
    gc.collect()
    assert len(ok) == G
    assert np.array_equal(gk, ok)
    assert np.array_equal(gw, ow), "dyadic sums / counts / min / max must be bit-exact"
    assert int(gw[:, 1].sum()) == n


@pytest.mark.parametrize("skew", [False, True])
def test_groupby_full_config3_ordered_to_host(ex, orc, skew):
    """Config 3 at G = 1e7 as the bench runs it (nut_groupby_to_host, the key-range ordered
    path) on 1e9 rows: uniform pool keys, and Zipf-like keys (GEN_SKEW_KEY: pool index i on
    ~1/i of the rows, the top key ~6 %) whose frequent keys go through the heavy-key pass
    before the partition levels (heavy.hpp) — both bit-exact against the indexed oracle,
    both on the ordered path."""
    import torch
    from nutdb_amd import Agg, AggQuery
    from nutdb_amd import _lib as L
    from nutdb_amd.workloads import GB_KEY_SEED, GB_VAL_SEED, gen, groupby_cols
    n, G = 1_000_000_000, 10_000_000
    ks, vs = groupby_cols(G, dyadic=True, skew=skew)
    key, val = gen(ex, ks, n), gen(ex, vs, n)
    out = tuple(torch.empty((G, w), dtype=torch.int64, pin_memory=True).numpy() for w in (1, 4))
    q = AggQuery(keys=[key], values=[val], aggs=[Agg("sum", "col", (0,)), Agg("count"), Agg("min", "col", (0,)),
                                                   Agg("max", "col", (0,))])
    gk, gw = ex.groupby_to_host(q, group_hint=G, out=out)
    st, hv, ovf = ex.groupby_stats(), ex.groupby_heavy(), ex.groupby_overflow_rows()
    gk, gw = gk.copy(), gw.copy()
    del key, val, out
    assert st["path"] == "partitioned_ordered", st
    assert (hv[1] > n // 4) == skew and (hv[0] > 0) == skew, hv
    assert not skew or ovf == 0, ovf  # (behind the heavy pass the levels' regions are exact)
    ok, ow = orc.groupby_pool_dyadic(G, n, key_seed=GB_KEY_SEED, val_seed=GB_VAL_SEED,
                                     kind=L.GEN_SKEW_KEY if skew else L.GEN_POOL_KEY)
    gc.collect()
    assert np.array_equal(gk, ok)
    assert np.array_equal(gw.view(np.uint64), ow), "dyadic sums / counts / min / max must be bit-exact"
    assert int(gw[:, 1].sum()) == n
