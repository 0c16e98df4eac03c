"""Narrow against widened columns, same process.

The TPC-H Q1 shape in expression mode over the columns as a user would declare them —
l_shipdate Int32, two Int8 flags, three Float32 measures: 18 B/row — against the same values
as 8-byte columns (48 B/row), and `select ... where x < k` (select_rows) over an Int32
against an Int64 column.  The two sides alternate for --rounds rounds after a warm-up; times
are the kernels' own (nut_ctx_kernel_time, hipEvents around each launch).  Prints one JSON
line per measurement: ms (median, min, max per side), bytes/s against the algorithmic bytes,
and the widened / narrow ratio.

  python scripts/narrow_q1.py [--rows 1e9] [--select-rows 1e8] [--rounds 5] [--attribute]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from nutdb_amd import Executor, ProgQuery  # noqa: E402
from nutdb_amd import _lib as L  # noqa: E402
from nutdb_amd.workloads import FILTER_COL, Q1_COLS, Q1_DATE_K, gen  # noqa: E402

NARROW = [torch.int32, torch.int8, torch.int8, torch.float32, torch.float32, torch.float32]


def q1_query(cols):
    c = lambda i: ("col", i)
    disc_price = [c(4), ("f64", 0, 1.0), c(5), ("sub",), ("mul",)]
    return ProgQuery(keys=[[c(1)], [c(2)]], cols=cols, where=[c(0), ("i64", 0, Q1_DATE_K), ("le",)],
                     aggs=[("sum", [c(3)], None), ("sum", [c(4)], None), ("sum", disc_price, None), ("count", None, None)])


def timed(ex, kind, fn):
    ex.kernel_time(kind)  # reset
    out = fn()
    ex.sync()
    ms, _ = ex.kernel_time(kind)
    return ms, out


def report(name, rows, sides, bytes_per_row):
    rec = {"measurement": name, "rows": rows}
    for side, ms in sides.items():
        med = statistics.median(ms)
        rec[side] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                     "bytes_per_row": bytes_per_row[side],
                     "tb_per_s": round(rows * bytes_per_row[side] / (med * 1e-3) / 1e12, 3)}
    rec["widened_over_narrow"] = round(rec["widened"]["ms_median"] / rec["narrow"]["ms_median"], 3)
    rec["byte_ratio"] = round(bytes_per_row["widened"] / bytes_per_row["narrow"], 3)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e9)
    ap.add_argument("--select-rows", type=float, default=1e8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--attribute", action="store_true",
                    help="also time Q1 with only the integer / only the Float32 columns narrow")
    args = ap.parse_args()
    ex = Executor(0)
    ex.enable_timing(True)

    n = int(args.rows)
    narrow, wide = [], []
    for spec, dt in zip(Q1_COLS, NARROW):
        full = gen(ex, spec, n)
        nar = full.to(dt)  # l_extendedprice and l_discount round to Float32 here ...
        narrow.append(nar)
        wide.append(nar.to(full.dtype))  # ... and the widened side holds exactly those values
        del full
    qs = {"narrow": q1_query(narrow), "widened": q1_query(wide)}
    bpr = {"narrow": 18, "widened": 48}
    if args.attribute:  # which columns' width costs what: only the integers, only the measures narrow
        qs["narrow_ints"] = q1_query(narrow[:3] + wide[3:])
        qs["narrow_floats"] = q1_query(wide[:3] + narrow[3:])
        bpr.update(narrow_ints=30, narrow_floats=36)
    res = {}
    sides = {k: [] for k in qs}
    for rnd in range(-1, args.rounds):  # round -1: warm-up (the run-time compile)
        for side, q in qs.items():
            ms, g = timed(ex, L.KERNEL_AGGREGATE, lambda: ex.groupby(q, group_hint=8))
            res[side] = g.to_host_words()
            g.free()
            if rnd >= 0:
                sides[side].append(ms)
    assert np.array_equal(res["narrow"][0], res["widened"][0])
    assert np.array_equal(res["narrow"][1][:, 3], res["widened"][1][:, 3])
    a, b = (res[s][1][:, :3].view(np.float64) for s in ("narrow", "widened"))
    assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), (a, b)
    report("q1_expression_mode", n, sides, bpr)
    del narrow, wide, qs

    m = int(args.select_rows)
    col = gen(ex, FILTER_COL, m) >> 32  # uniform [0, 2^30): fits Int32
    cols = {"narrow": col.to(torch.int32), "widened": col}
    where = [("col", 0), ("i64", 0, 2**29), ("lt",)]  # selectivity 0.5
    sides = {"narrow": [], "widened": []}
    ids = {}
    for rnd in range(-1, args.rounds):
        for side, t in cols.items():
            ms, out = timed(ex, L.KERNEL_FILTER, lambda: ex.select_rows([t], where))
            ids[side] = out
            if rnd >= 0:
                sides[side].append(ms)
    assert torch.equal(ids["narrow"], ids["widened"])
    sel = ids["narrow"].numel() / m
    # algorithmic bytes: the column once + 8 B per selected row id
    report("select_rows_where", m, sides, {"narrow": round(4 + 8 * sel, 3), "widened": round(8 + 8 * sel, 3)})
    ex.close()


if __name__ == "__main__":
    main()
