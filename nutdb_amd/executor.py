"""Host-side executor API over the nutexec C ABI.

Mirrors what the reference's AST hands an executor:
  WhereClause      (src/parser/ast/query.rs:68-72)  -> predicates  [(column, op, literal)]
  GroupByClause    (src/parser/ast/query.rs:74-78)  -> keys        [column, column]
  SELECT FnCall    (src/parser/ast/expr.rs:32-36)   -> aggregates  [(op, expr, args)]
  OrderByClause    (src/parser/ast/query.rs:86-90)  -> sort_i64
Columns are torch tensors resident on the GPU (HBM); torch is only the allocator and
stream provider.  Every operator runs a hand-written HIP kernel in libnutexec.so.
"""
from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from ._lib import check, lib

CMP = {"<": L.LT, "<=": L.LE, ">": L.GT, ">=": L.GE, "=": L.EQ, "==": L.EQ, "!=": L.NE, "<>": L.NE,
       "in": L.IN, "not in": L.NOT_IN}
AGG = {"sum": L.AGG_SUM, "count": L.AGG_COUNT, "min": L.AGG_MIN, "max": L.AGG_MAX}
EXPR = {"col": L.EX_COL, "mul": L.EX_MUL, "add": L.EX_ADD, "sub": L.EX_SUB,
        "mul_1m": L.EX_MUL_1M, "mul_1m_1p": L.EX_MUL_1M_1P}


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.int64:
        return L.T_I64
    if t.dtype == torch.float64:
        return L.T_F64
    raise TypeError(f"nutexec columns are int64 or float64, got {t.dtype}")


# narrow torch dtypes -> physical nut_type codes (uint16 / uint32 where this torch has them)
_NARROW = {torch.int32: L.T_I32, torch.int16: L.T_I16, torch.int8: L.T_I8, torch.uint8: L.T_U8,
           torch.float32: L.T_F32}
for _name, _code in (("uint16", L.T_U16), ("uint32", L.T_U32)):
    if hasattr(torch, _name):
        _NARROW[getattr(torch, _name)] = _code


def _phys_code(t) -> int:
    """nut_type of a column the generated kernels and gather read at its stored width:
    int64 / float64 as _dtype_code, narrow dtypes as their physical code."""
    code = _NARROW.get(t.dtype)
    return _dtype_code(t) if code is None else code


def _col(t: torch.Tensor, dev: torch.device) -> int:
    if t.device != dev:
        raise ValueError(f"column on {t.device}, executor on {dev}")
    if not t.is_contiguous() or t.dim() != 1:
        raise ValueError("columns must be contiguous 1-D tensors")
    return t.data_ptr()


@dataclass
class Agg:
    op: str                      # sum | count | min | max
    expr: str = "col"            # col | mul | add | sub | mul_1m | mul_1m_1p
    args: Sequence[int] = ()     # indices into AggQuery.values


@dataclass
class AggQuery:
    """SELECT keys..., aggs... FROM t WHERE preds... GROUP BY keys...  (no keys: a global
    aggregate, one group with key 0)"""
    keys: list
    aggs: list
    values: list = field(default_factory=list)
    preds: list = field(default_factory=list)   # (column, op, literal)
    rows: int | None = None                     # row count when there is no column at all

    def to_spec(self, dev: torch.device) -> L.NutAggSpec:
        # built once per device and column set: a query run step after step (the bench,
        # a prepared statement) pays the ctypes marshalling once
        cols = list(self.keys) + list(self.values) + [c for c, _, _ in self.preds]
        lits = tuple((op, tuple(lit) if isinstance(lit, (list, tuple)) else lit) for _, op, lit in self.preds)
        tag = (str(dev), tuple((t.data_ptr(), t.numel(), t.dtype) for t in cols), len(self.keys), len(self.values),
               tuple((a.op, a.expr, tuple(a.args)) for a in self.aggs), lits, self.rows)
        cached = self.__dict__.get("_spec")
        if cached is not None and cached[0] == tag:
            return cached[1]
        s = self._build_spec(dev)
        self.__dict__["_spec"] = (tag, s)
        return s

    def _build_spec(self, dev: torch.device) -> L.NutAggSpec:
        s = L.NutAggSpec()
        cols = list(self.keys) + list(self.values) + [c for c, _, _ in self.preds]
        n = int(cols[0].numel()) if cols else int(self.rows or 0)
        s.n = n
        if not 0 <= len(self.keys) <= L.NUT_MAX_KEYS:
            raise ValueError("0, 1 or 2 group keys")
        s.nkeys = len(self.keys)
        for i, k in enumerate(self.keys):
            if k.dtype != torch.int64:
                raise TypeError("group keys are int64 columns")
            if k.numel() != n:
                raise ValueError("ragged columns")
            s.keys[i] = _col(k, dev)
        if len(self.preds) > L.NUT_MAX_PRED:
            raise ValueError("too many predicate terms")
        s.npred = len(self.preds)
        for i, (col, op, lit) in enumerate(self.preds):
            if col.numel() != n:
                raise ValueError("ragged columns")
            s.pred_col[i] = _col(col, dev)
            s.pred_type[i] = _dtype_code(col)
            s.pred_op[i] = CMP[op] if isinstance(op, str) else int(op)
            if s.pred_op[i] in (L.IN, L.NOT_IN):  # lit: a sequence of 1..16 values
                vals = list(lit)
                if not 1 <= len(vals) <= L.NUT_MAX_SET:
                    raise ValueError("IN sets hold 1..16 values")
                s.pred_nset[i] = len(vals)
                for j, v in enumerate(vals):
                    if s.pred_type[i] == L.T_I64:
                        s.pred_set[i][j] = int(v)
                    else:
                        s.pred_set[i][j] = int(np.array([float(v)], dtype=np.float64).view(np.int64)[0])
            elif s.pred_type[i] == L.T_I64:
                s.pred_i64[i] = int(lit)
            else:
                s.pred_f64[i] = float(lit)
        if len(self.values) > L.NUT_MAX_VALS:
            raise ValueError("too many value columns")
        s.nvals = len(self.values)
        for i, v in enumerate(self.values):
            if v.numel() != n:
                raise ValueError("ragged columns")
            s.val_col[i] = _col(v, dev)
            s.val_type[i] = _dtype_code(v)
        if len(self.aggs) > L.NUT_MAX_AGGS:
            raise ValueError("too many aggregates")
        s.naggs = len(self.aggs)
        for i, a in enumerate(self.aggs):
            s.agg_op[i] = AGG[a.op]
            s.agg_expr[i] = EXPR[a.expr]
            for j, x in enumerate(a.args):
                s.agg_arg[i][j] = int(x)
        return s

    def result_types(self) -> list:
        """numpy dtype of each aggregate word (matches nutexec.h result words)."""
        out = []
        for a in self.aggs:
            if a.op == "count":
                out.append(np.int64)
            elif a.expr == "col" and self.values[a.args[0]].dtype == torch.int64:
                out.append(np.int64)
            else:
                out.append(np.float64)
        return out


def _node(nd) -> tuple:
    """(op, arg, v): op = nut_prog_op index or name (_lib.PROG_OPS); an "f64" constant
    may be given as a Python float (stored as the double's bits)."""
    op, arg, v = (tuple(nd) + (0, 0))[:3]
    op = L.P[op] if isinstance(op, str) else int(op)
    if op == L.P["f64"] and isinstance(v, float):
        v = int(np.array([v], dtype=np.float64).view(np.int64)[0])
    return op, int(arg), int(v)


def _prog(nodes, keep: list) -> L.NutProg:
    pr = L.NutProg()
    if not nodes:
        return pr
    if len(nodes) > L.NUT_MAX_PROG_NODES:
        raise ValueError("expression programs hold at most 256 nodes")
    arr = (L.NutProgNode * len(nodes))()
    for i, nd in enumerate(nodes):
        arr[i].op, arr[i].arg, arr[i].v = _node(nd)
    keep.append(arr)
    pr.n = len(nodes)
    pr.node = C.cast(arr, C.POINTER(L.NutProgNode))
    return pr


@dataclass
class ProgQuery:
    """Expression mode of nut_groupby (include/nutexec.h nut_prog): WHERE and every
    aggregate argument are RPN programs over `cols`, compiled for the query at run time
    (csrc/jit.cpp).  aggs = [(op, value program or None, mask program or None)]: the
    mask keeps only rows where it is true (CASE without ELSE).  A key is an int64 column
    or an int64 / bool program over `cols` (a computed key: nut_agg_spec.key_prog).
    `cols` may be narrow (int8 / 16 / 32, uint8 / 16 / 32, float32): the kernel reads them at
    their stored width and computes on int64 / float64; a narrow key is the program
    [("col", c)].  Narrow columns save HBM, not yet time: measured at 1e9 rows (DESIGN.md
    4.2d) int32 / float32 columns run up to 1.12x faster than widened ones, int8 / int16
    columns slower (a Q1 with two int8 keys 1.3x) until the kernel holds more rows per lane
    for them; widen those first (Executor.gather(col, None)) where time matters more."""
    keys: list
    cols: list
    aggs: list
    where: list | None = None
    rows: int | None = None

    def to_spec(self, dev: torch.device) -> L.NutAggSpec:
        s = L.NutAggSpec()
        keep = []
        s._keep = keep  # node arrays live as long as the spec
        cols = [k for k in self.keys if isinstance(k, torch.Tensor)] + list(self.cols)
        n = int(cols[0].numel()) if cols else int(self.rows or 0)
        s.n = n
        if not 0 <= len(self.keys) <= L.NUT_MAX_KEYS:
            raise ValueError("0, 1 or 2 group keys")
        s.nkeys = len(self.keys)
        for i, k in enumerate(self.keys):
            if not isinstance(k, torch.Tensor):
                s.key_prog[i] = _prog(k, keep)
                continue
            if k.dtype != torch.int64 or k.numel() != n:
                raise ValueError("group keys are int64 columns of equal length")
            s.keys[i] = _col(k, dev)
        if len(self.cols) > L.NUT_MAX_PROG_COLS:
            raise ValueError("programs read at most 16 columns")
        s.prog_mode = 1
        s.nprog_cols = len(self.cols)
        for i, c in enumerate(self.cols):
            if c.numel() != n:
                raise ValueError("ragged columns")
            s.prog_col[i] = _col(c, dev)
            s.prog_col_type[i] = _phys_code(c)
        s.where = _prog(self.where, keep)
        if len(self.aggs) > L.NUT_MAX_AGGS:
            raise ValueError("too many aggregates")
        s.naggs = len(self.aggs)
        for i, (op, val, mask) in enumerate(self.aggs):
            s.agg_op[i] = AGG[op] if isinstance(op, str) else int(op)
            s.agg_val[i] = _prog(val, keep)
            s.agg_mask[i] = _prog(mask, keep)
        return s

    def result_types(self) -> list:
        types = (C.c_int32 * max(len(self.cols), 1))(*[_phys_code(c) for c in self.cols])
        out = []
        for op, val, _ in self.aggs:
            if (AGG[op] if isinstance(op, str) else int(op)) == L.AGG_COUNT:
                out.append(np.int64)
                continue
            keep = []
            t = C.c_int32()
            check(lib.nut_prog_type(C.byref(_prog(val, keep)), types, len(self.cols), C.byref(t)), "nut_prog_type")
            out.append(np.float64 if t.value == L.PT_F64 else np.int64)
        return out


class Groups:
    """Library-owned group-by result (nut_groups*)."""

    def __init__(self, ex: "Executor", handle: int, nkeys: int, types: list):
        self.ex = ex
        self.h = C.c_void_p(handle)
        self.nkeys = nkeys
        self.types = types

    @property
    def naggs(self) -> int:
        return len(self.types)

    def __len__(self) -> int:
        n = C.c_uint64()
        check(lib.nut_groups_size(self.h, C.byref(n)), "nut_groups_size")
        return n.value

    def to_host_words(self, out=None):
        """(keys int64 [n, nkeys], aggs uint64 [n, naggs]) sorted by key tuple.  out: a
        (keys, aggs) pair of C-contiguous host arrays with room for n rows to fill instead
        (a caller's reused result buffers; page-locked ones are written by the copy engine
        directly)."""
        n = len(self)
        if out is not None:
            ko, ao = out
            if (ko.dtype != np.int64 or ao.dtype.itemsize != 8 or ko.shape[0] < n or ao.shape[0] < n
                    or ko.shape[1:] != (self.nkeys,) or ao.shape[1:] != (max(self.naggs, 1),)
                    or not ko.flags.c_contiguous or not ao.flags.c_contiguous):
                raise ValueError("to_host_words: out arrays must be C-contiguous int64 [>=n, nkeys] / "
                                 "8-byte [>=n, max(naggs, 1)]")
            check(lib.nut_groups_to_host(self.h, ko.ctypes.data, ao.ctypes.data, n), "nut_groups_to_host")
            return ko[:n], ao[:n, : self.naggs].view(np.uint64)
        # np.empty: the library writes every word; np.zeros spent ~10 ms zeroing 1e7 groups
        keys = np.empty((n, self.nkeys), dtype=np.int64)
        aggs = np.empty((n, max(self.naggs, 1)), dtype=np.uint64)
        check(lib.nut_groups_to_host(self.h, keys.ctypes.data, aggs.ctypes.data, n), "nut_groups_to_host")
        return keys, aggs[:, : self.naggs]

    def to_host(self):
        """(keys int64 [n, nkeys], [per-aggregate numpy column with its natural dtype])."""
        keys, words = self.to_host_words()
        cols = [np.ascontiguousarray(words[:, i]).view(t) for i, t in enumerate(self.types)]
        return keys, cols

    def to_device(self) -> torch.Tensor:
        """uint64-as-int64 tensor [nkeys+naggs, n] on the device, unordered."""
        n = len(self)
        w = self.nkeys + self.naggs
        out = torch.empty((w, max(n, 1)), dtype=torch.int64, device=self.ex.device)
        check(lib.nut_groups_to_device(self.h, out.data_ptr(), max(n, 1)), "nut_groups_to_device")
        return out[:, :n] if n else out[:, :0]

    def partition(self, nparts: int):
        """Device buffer of nparts column-major segments + per-part group counts."""
        n = len(self)
        w = self.nkeys + self.naggs
        buf = torch.empty(max(w * n, 1), dtype=torch.int64, device=self.ex.device)
        counts = (C.c_uint64 * nparts)()
        check(lib.nut_groups_partition(self.h, nparts, buf.data_ptr(), max(n, 1), counts), "nut_groups_partition")
        return buf[: w * n], [int(x) for x in counts]

    def free(self) -> None:
        if self.h:
            # nut_groups_free hands the table's allocation back to its context, which must
            # still be there (Executor.close frees the results it still owns first)
            if self.ex.ctx:
                lib.nut_groups_free(self.h)
            self.h = C.c_void_p(None)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Executor:
    """One nut_ctx bound to a GPU and to torch's current stream on it."""

    def __init__(self, device: int | torch.device = 0):
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("nutexec runs on a GPU device (torch 'cuda' = HIP)")
        if not torch.cuda.is_available():
            raise RuntimeError("nutdb_amd: no GPU visible — the executor has no CPU fallback")
        self.device = dev
        h = C.c_void_p()
        check(lib.nut_ctx_create(dev.index or 0, C.byref(h)), "nut_ctx_create")
        self.ctx = h
        self._groups = weakref.WeakSet()  # results not yet freed: their tables go back to this context
        self._bind_stream()

    def _bind_stream(self):
        s = torch.cuda.current_stream(self.device)
        check(lib.nut_ctx_set_stream(self.ctx, C.c_void_p(s.cuda_stream)), "nut_ctx_set_stream")

    def close(self):
        if self.ctx:
            for g in list(self._groups):  # a result freed after its context would touch freed memory
                g.free()
            lib.nut_ctx_destroy(self.ctx)
            self.ctx = None

    def _own(self, g: Groups) -> Groups:
        self._groups.add(g)
        return g

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        ncu = C.c_int()
        name = C.create_string_buffer(64)
        check(lib.nut_ctx_info(self.ctx, C.byref(ncu), name, 64), "nut_ctx_info")
        return {"num_cus": ncu.value, "name": name.value.decode()}

    def enable_timing(self, on: bool = True) -> None:
        check(lib.nut_ctx_enable_timing(self.ctx, int(on)), "nut_ctx_enable_timing")

    def kernel_time(self, kind: int):
        """(total_ms, launches) of one hot-kernel kind since the last call (device events)."""
        ms = C.c_double()
        cnt = C.c_uint64()
        check(lib.nut_ctx_kernel_time(self.ctx, kind, C.byref(ms), C.byref(cnt)), "nut_ctx_kernel_time")
        return ms.value, cnt.value

    def priv_shape(self) -> dict:
        """The compiled Q1 kernel's launch shape on this device (nut_ctx_priv_shape): threads
        per workgroup, workgroups per CU, and the shape probe's kernel ms per candidate
        (None where the probe has not run in this process)."""
        t, b = C.c_int(), C.c_int()
        ms = (C.c_double * 3)()
        check(lib.nut_ctx_priv_shape(self.ctx, C.byref(t), C.byref(b), ms), "nut_ctx_priv_shape")
        cost = C.c_double()
        check(lib.nut_ctx_priv_probe_cost(self.ctx, C.byref(cost)), "nut_ctx_priv_probe_cost")
        return {"threads": t.value, "blocks_per_cu": b.value,
                "probe_ms": {f"{a}x{c}": (round(m, 4) if m >= 0 else None)
                             for (a, c), m in zip(((192, 2), (128, 3), (128, 4)), ms)},
                "probe_first_call_cost_ms": round(cost.value, 3)}

    def sort_stats(self):
        """(algorithmic HBM bytes, scatter levels) of the last sort on this context."""
        b = C.c_uint64()
        lv = C.c_uint32()
        check(lib.nut_ctx_sort_stats(self.ctx, C.byref(b), C.byref(lv)), "nut_ctx_sort_stats")
        return b.value, lv.value

    GROUPBY_PATHS = ("onchip", "partitioned_direct", "partitioned_spill", "partitioned_ordered")
    OPTIONS = {"gb_partition": 0, "gb_levels": 1, "gb_optimistic": 2, "gb_direct": 3, "gb_chunks": 4,
               "join_region": 5, "join_probe_cfg": 6, "join_any_cfg": 7, "gb_seg_slots": 8,
               "gb_dense": 9, "gb_l1_bits": 10,
               "topk": 11, "gb_l0_bits": 12, "stream_blocks": 13,
               "priv_bd": 14, "priv_blocks": 15, "agg_blocks": 16, "sel_blocks": 17, "sort_bd": 18,
               "gb_ordered": 19, "priv_probe": 20, "gb_heavy": 21,
               "join_match": 22, "gb_l1_threads": 23, "agg_slots": 24, "gb_l1_spare": 25}

    def groupby_stats(self) -> dict:
        """The algorithm the last group-by on this context took (nut_ctx_groupby_stats)."""
        p, lv, opt = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib.nut_ctx_groupby_stats(self.ctx, C.byref(p), C.byref(lv), C.byref(opt)), "nut_ctx_groupby_stats")
        return {"path": self.GROUPBY_PATHS[p.value], "levels": lv.value, "optimistic": bool(opt.value),
                "capped_levels": opt.value}

    GB_DECLINES = ("none", "shape", "clustered", "arena", "capacity", "table")

    def groupby_overflow_rows(self) -> int:
        """Rows of the last ordered group-by (groupby_to_host) aggregated from its overflow
        arenas — a heavy key's excess past its capped partition (nut_ctx_groupby_overflow)."""
        r, d = C.c_uint64(), C.c_uint32()
        check(lib.nut_ctx_groupby_overflow(self.ctx, C.byref(r), C.byref(d)), "nut_ctx_groupby_overflow")
        return r.value

    def groupby_heavy(self) -> tuple:
        """(keys, rows) the last ordered groupby_to_host aggregated in its heavy-key pass
        before the partition levels (nut_ctx_groupby_heavy)."""
        k, r = C.c_uint32(), C.c_uint64()
        check(lib.nut_ctx_groupby_heavy(self.ctx, C.byref(k), C.byref(r)), "nut_ctx_groupby_heavy")
        return k.value, r.value

    def groupby_declined(self) -> str:
        """Why the last groupby_to_host left the ordered path ("none" if it did not)."""
        r, d = C.c_uint64(), C.c_uint32()
        check(lib.nut_ctx_groupby_overflow(self.ctx, C.byref(r), C.byref(d)), "nut_ctx_groupby_overflow")
        return self.GB_DECLINES[d.value] if d.value < len(self.GB_DECLINES) else str(d.value)

    def set_option(self, name: str, value: int) -> int:
        """nut_ctx_set_option (tuning / tests); returns the previous value."""
        key = self.OPTIONS[name]
        old = C.c_int64()
        check(lib.nut_ctx_get_option(self.ctx, key, C.byref(old)), "nut_ctx_get_option")
        check(lib.nut_ctx_set_option(self.ctx, key, int(value)), "nut_ctx_set_option")
        return old.value

    def sync(self):
        check(lib.nut_ctx_sync(self.ctx), "nut_ctx_sync")

    def stream_probe(self, read_bytes: int, write_bytes: int, reps: int = 5) -> float:
        """Device ms of the fastest of `reps` copy-floor launches (nut_stream_probe) that read
        read_bytes and write write_bytes of them; the buffers are allocated here and freed."""
        read_bytes -= read_bytes % 16
        write_bytes -= write_bytes % 16
        src = torch.empty(read_bytes, dtype=torch.uint8, device=self.device)
        dst = torch.empty(write_bytes + 1024 if write_bytes else 16, dtype=torch.uint8, device=self.device)
        self._bind_stream()
        ms = C.c_double()
        check(lib.nut_stream_probe(self.ctx, C.c_void_p(src.data_ptr()), read_bytes, C.c_void_p(dst.data_ptr()),
                                   write_bytes, reps, C.byref(ms)), "nut_stream_probe")
        del src, dst
        return ms.value

    # ---------------------------------------------------------------- data
    def gen_column(self, kind: int, seed: int, n: int, row0: int = 0, a: int = 0, b: int = 0,
                   c: float = 1.0, out: torch.Tensor | None = None) -> torch.Tensor:
        dt = torch.float64 if kind in (L.GEN_DYADIC, L.GEN_UNIT_F64, L.GEN_RANGE_F64) else torch.int64
        if out is None:
            out = torch.empty(n, dtype=dt, device=self.device)
        self._bind_stream()
        check(lib.nut_gen_column(self.ctx, kind, seed & (2**64 - 1), a, b, c, row0, n,
                                 C.c_void_p(out.data_ptr() if n else None)), "nut_gen_column")
        return out

    # ---------------------------------------------------------------- filter
    def filter_i64(self, col: torch.Tensor, op: str | int, k: int, out: torch.Tensor | None = None) -> torch.Tensor:
        if col.dtype != torch.int64:
            raise TypeError("filter_i64 takes an int64 column")
        n = col.numel()
        if out is None:
            out = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        self._bind_stream()
        cnt = C.c_uint64()
        check(lib.nut_filter_i64(self.ctx, C.c_void_p(_col(col, self.device) if n else None), n,
                                 CMP[op] if isinstance(op, str) else int(op), int(k),
                                 C.c_void_p(out.data_ptr()), C.byref(cnt)), "nut_filter_i64")
        return out[: cnt.value]

    def filter_i64_async(self, col: torch.Tensor, op, k: int, out: torch.Tensor, out_n: torch.Tensor) -> None:
        self._bind_stream()
        check(lib.nut_filter_i64_async(self.ctx, C.c_void_p(col.data_ptr()), col.numel(),
                                       CMP[op] if isinstance(op, str) else int(op), int(k),
                                       C.c_void_p(out.data_ptr()), C.c_void_p(out_n.data_ptr())),
              "nut_filter_i64_async")

    def lookback_probe(self, status, tile: int, total: int) -> tuple:
        """nut_lookback_probe (a test hook): the look-back of `tile` over the constructed
        granules `status` (uint64, {flag:2 | value:62}).  Returns (the exclusive prefix,
        status[tile] as published afterwards).  A predecessor without a flag is refused."""
        s = np.ascontiguousarray(np.asarray(status, dtype=np.uint64))
        excl, gran = C.c_uint64(), C.c_uint64()
        self._bind_stream()
        check(lib.nut_lookback_probe(self.ctx, s.ctypes.data_as(C.c_void_p), len(s), int(tile), int(total),
                                     C.byref(excl), C.byref(gran)), "nut_lookback_probe")
        return excl.value, gran.value

    # ---------------------------------------------------------------- group-by
    def groupby(self, q: "AggQuery | ProgQuery", group_hint: int = 0) -> Groups:
        spec = q.to_spec(self.device)
        self._bind_stream()
        h = C.c_void_p()
        check(lib.nut_groupby(self.ctx, C.byref(spec), group_hint, C.byref(h)), "nut_groupby")
        return self._own(Groups(self, h.value, max(spec.nkeys, 1), q.result_types()))

    def groupby_to_host(self, q: "AggQuery | ProgQuery", group_hint: int = 0, out=None):
        """nut_groupby_to_host: (keys int64 [n, nkeys], aggs uint64 [n, naggs]) sorted by key
        tuple, as groupby(q).to_host_words() — for one plain key column at large G the
        range-partitioned path that needs no sort and overlaps the transfer (page-locked
        `out` arrays: a (keys, aggs) pair with room for the groups; without `out` page-locked
        arrays of max(2 * group_hint, 1024) rows are made, and again at the size the library
        reports if that was too small)."""
        spec = q.to_spec(self.device)
        nk, na = max(spec.nkeys, 1), len(q.result_types())
        self._bind_stream()
        n = C.c_uint64()
        rows = max(2 * int(group_hint), 1024)
        for _ in range(2):
            if out is None:
                ko = torch.empty((rows, nk), dtype=torch.int64, pin_memory=True).numpy()
                ao = torch.empty((rows, max(na, 1)), dtype=torch.int64, pin_memory=True).numpy().view(np.uint64)
            else:
                ko, ao = out
                if (ko.dtype != np.int64 or ao.dtype.itemsize != 8 or ko.shape[1:] != (nk,) or ko.shape[0] != ao.shape[0]
                        or ao.shape[1:] != (max(na, 1),) or not ko.flags.c_contiguous or not ao.flags.c_contiguous):
                    raise ValueError("groupby_to_host: out arrays must be C-contiguous int64 [cap, nkeys] / "
                                     "8-byte [cap, max(naggs, 1)]")
            st = lib.nut_groupby_to_host(self.ctx, C.byref(spec), group_hint, ko.ctypes.data, ao.ctypes.data,
                                         ko.shape[0], C.byref(n))
            if st == L.NUT_ERR_CAPACITY and out is None:
                rows = n.value
                continue
            check(st, "nut_groupby_to_host")
            m = n.value
            return ko[:m], ao[:m, :na].view(np.uint64)
        raise RuntimeError("nut_groupby_to_host: result size changed between two runs")

    def accumulate(self, q: AggQuery, acc: Groups) -> None:
        spec = q.to_spec(self.device)
        self._bind_stream()
        check(lib.nut_groupby_accumulate(self.ctx, C.byref(spec), acc.h), "nut_groupby_accumulate")

    def q1(self, shipdate, returnflag, linestatus, qty, price, disc, date_k: int = 10471) -> Groups:
        n = shipdate.numel()
        for t in (returnflag, linestatus, qty, price, disc):
            if t.numel() != n:
                raise ValueError("ragged columns")
        self._bind_stream()
        h = C.c_void_p()
        ptrs = [C.c_void_p(_col(t, self.device)) for t in (shipdate, returnflag, linestatus, qty, price, disc)]
        check(lib.nut_q1(self.ctx, *ptrs, n, int(date_k), C.byref(h)), "nut_q1")
        return self._own(Groups(self, h.value, 2, [np.float64, np.float64, np.float64, np.int64]))

    # ---------------------------------------------------------------- sort
    def sort_i64(self, col: torch.Tensor, out: torch.Tensor | None = None, descending: bool = False) -> torch.Tensor:
        if col.dtype != torch.int64:
            raise TypeError("sort_i64 takes an int64 column")
        n = col.numel()
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=self.device)
        self._bind_stream()
        fn = lib.nut_sort_i64_desc if descending else lib.nut_sort_i64
        check(fn(self.ctx, C.c_void_p(_col(col, self.device) if n else None),
                 C.c_void_p(out.data_ptr() if n else None), n), fn.__name__)
        return out

    # ---------------------------------------------------------------- join
    JOIN_TYPES = {"inner": 0, "left": 1, "semi": 2, "anti": 3}

    def join_i64(self, build: torch.Tensor, probe: torch.Tensor, how: str = "inner", passes: int = 1,
                 any_order: bool = False):
        """Hash equi-join (nut_join_i64): (probe_idx, build_idx) int64 tensors, ordered by
        probe row (any_order: in unspecified order, NUT_JOIN_ANY_ORDER — the unordered
        probe); build_idx = -1 for LEFT rows without a match and for SEMI /
        ANTI rows.
        Lowered from JoinClause (src/parser/ast/query.rs:55-66, 100-117).  passes=1:
        nut_join_i64_into (one probe pass into arrays of len(probe) pairs, again with the
        exact size if the build keys repeat); passes=2: nut_join_i64 (count) +
        nut_join_write."""
        for t in (build, probe):
            if t.dtype != torch.int64:
                raise TypeError("join_i64 takes int64 key columns")
        if how not in self.JOIN_TYPES:
            raise ValueError(f"join type {how!r} (inner, left, semi, anti)")
        self._bind_stream()
        n = C.c_uint64()
        nb, np_ = build.numel(), probe.numel()
        bp = C.c_void_p(_col(build, self.device) if nb else None)
        pp = C.c_void_p(_col(probe, self.device) if np_ else None)
        if passes == 2:
            h = C.c_void_p()
            check(lib.nut_join_i64(self.ctx, bp, nb, pp, np_,
                                   self.JOIN_TYPES[how] | (L.NUT_JOIN_ANY_ORDER if any_order else 0), C.byref(h),
                                   C.byref(n)),
                  "nut_join_i64")
            try:
                pi = torch.empty(n.value, dtype=torch.int64, device=self.device)
                bi = torch.empty(n.value, dtype=torch.int64, device=self.device)
                check(lib.nut_join_write(h, C.c_void_p(pi.data_ptr() if n.value else None),
                                         C.c_void_p(bi.data_ptr() if n.value else None)), "nut_join_write")
                self.sync()
            finally:
                lib.nut_join_free(h)
            return pi, bi
        cap = np_  # enough unless build keys repeat (INNER / LEFT): then one more pass
        while True:
            pi = torch.empty(cap, dtype=torch.int64, device=self.device)
            bi = torch.empty(cap, dtype=torch.int64, device=self.device)
            st = lib.nut_join_i64_into(self.ctx, bp, nb, pp, np_,
                                       self.JOIN_TYPES[how] | (L.NUT_JOIN_ANY_ORDER if any_order else 0),
                                       C.c_void_p(pi.data_ptr() if cap else None),
                                       C.c_void_p(bi.data_ptr() if cap else None), cap, C.byref(n))
            if st == L.NUT_ERR_CAPACITY and n.value > cap:
                cap = n.value
                continue
            check(st, "nut_join_i64_into")
            break
        self.sync()
        pi, bi = pi[:n.value], bi[:n.value]
        return pi, bi

    def gather(self, col: torch.Tensor, idx: torch.Tensor, null=0) -> torch.Tensor:
        """col[idx] for an int64 / float64 column, `null` where idx < 0 (nut_gather_u64).  A
        narrow column (int8 / 16 / 32, uint8 / 16 / 32, float32) comes back widened to int64 /
        float64 (nut_gather_typed); idx None: every row, a pure widening pass."""
        if col.dtype in _NARROW:
            return self._gather_typed(col, idx, null)
        if idx is None:
            raise TypeError("gather without an index widens a narrow column")
        if col.element_size() != 8 or idx.dtype != torch.int64:
            raise TypeError("gather takes an 8-byte column and an int64 index")
        n = idx.numel()
        out = torch.empty(n, dtype=col.dtype, device=self.device)
        nb = torch.tensor([null], dtype=col.dtype).view(torch.int64).item() & 0xFFFFFFFFFFFFFFFF
        self._bind_stream()
        check(lib.nut_gather_u64(self.ctx, C.c_void_p(_col(col, self.device) if col.numel() else None),
                                 C.c_void_p(idx.data_ptr() if n else None), n, nb,
                                 C.c_void_p(out.data_ptr() if n else None)), "nut_gather_u64")
        return out

    def _gather_typed(self, col: torch.Tensor, idx, null) -> torch.Tensor:
        if idx is not None and idx.dtype != torch.int64:
            raise TypeError("gather takes an int64 index")
        code = _NARROW[col.dtype]
        odt = torch.float64 if code == L.T_F32 else torch.int64
        n = col.numel() if idx is None else idx.numel()
        out = torch.empty(n, dtype=odt, device=self.device)
        nb = torch.tensor([null], dtype=odt).view(torch.int64).item() & 0xFFFFFFFFFFFFFFFF
        self._bind_stream()
        check(lib.nut_gather_typed(self.ctx, C.c_void_p(_col(col, self.device) if col.numel() else None), code,
                                   C.c_void_p(idx.data_ptr() if idx is not None and n else None), n, nb,
                                   C.c_void_p(out.data_ptr() if n else None)), "nut_gather_typed")
        return out

    def eval_rows(self, cols: list, progs: list, rows: torch.Tensor | None = None):
        """Computed projections (nut_eval_rows): progs = [(value program, mask program or
        None)] over `cols`, evaluated at the row ids `rows` (None: every row).  Returns
        ([8-byte words as int64 tensors], [uint8 validity tensors])."""
        q = ProgQuery(keys=[], cols=list(cols), aggs=[("sum", v, m) for v, m in progs])
        spec = q.to_spec(self.device)
        if rows is not None and rows.dtype != torch.int64:
            raise TypeError("eval_rows takes int64 row ids")
        m = int(spec.n) if rows is None else rows.numel()
        outs = [torch.empty(max(m, 1), dtype=torch.int64, device=self.device) for _ in progs]
        valid = [torch.empty(max(m, 1), dtype=torch.uint8, device=self.device) for _ in progs]
        po = (C.c_void_p * len(progs))(*[o.data_ptr() for o in outs])
        pv = (C.c_void_p * len(progs))(*[v.data_ptr() for v in valid])
        self._bind_stream()
        check(lib.nut_eval_rows(self.ctx, C.byref(spec), C.c_void_p(rows.data_ptr() if rows is not None and m else None),
                                m, po, pv), "nut_eval_rows")
        return [o[:m] for o in outs], [v[:m] for v in valid]

    # the launch shape of nut_group_pick's kernels (csrc/pick.hpp): threads per workgroup,
    # rows a workgroup takes per step
    PICK_THREADS, PICK_TILE = 256, 1024

    def group_pick(self, row_keys: list, order: torch.Tensor | None, group_keys: list,
                   want_max: bool = False, nrows: int | None = None) -> torch.Tensor:
        """The per-group row pick behind any / anyLast / argMin / argMax (nut_group_pick):
        row_keys = 0..2 int64 key-word columns of the m rows, group_keys = as many columns of
        the ng group tuples (strictly ascending, signed, word 0 first; no keys: one group),
        order = m int64 / float64 order values or None (the position is the order).  Returns
        an int64 tensor of ng positions: the row of the least (want_max: greatest) order per
        group, ties to the lowest position, -1 for a group without rows.  nrows: the row count
        when neither a key nor an order column gives it."""
        nk = len(row_keys)
        if len(group_keys) != nk:
            raise ValueError("group_pick takes as many group key columns as row key columns")
        cols = list(row_keys) + list(group_keys) + ([order] if order is not None else [])
        if any(t.dtype != torch.int64 for t in cols[:2 * nk]):
            raise TypeError("group_pick takes int64 key words")
        if order is not None and order.dtype not in (torch.int64, torch.float64):
            raise TypeError("group_pick orders by an int64 or float64 column")
        if nk:
            m, ng = row_keys[0].numel(), group_keys[0].numel()
        else:
            if order is None and nrows is None:
                raise ValueError("group_pick without keys and order needs nrows")
            m, ng = order.numel() if order is not None else int(nrows), 1
        if any(t.numel() != m for t in row_keys) or any(t.numel() != ng for t in group_keys) or \
                (order is not None and order.numel() != m):
            raise ValueError("group_pick: columns of different lengths")
        ptrs = [_col(t, self.device) if t.numel() else None for t in cols]
        rk = (C.c_void_p * max(nk, 1))(*ptrs[:nk])
        gk = (C.c_void_p * max(nk, 1))(*ptrs[nk:2 * nk])
        out = torch.empty(max(ng, 1), dtype=torch.int64, device=self.device)
        self._bind_stream()
        check(lib.nut_group_pick(self.ctx, rk, nk, m, C.c_void_p(ptrs[2 * nk] if order is not None else None),
                                 L.T_F64 if order is not None and order.dtype == torch.float64 else L.T_I64,
                                 int(bool(want_max)), gk, ng, C.c_void_p(out.data_ptr())), "nut_group_pick")
        return out[:ng]

    def partition_i64(self, col: torch.Tensor, splitters, out: torch.Tensor | None = None):
        """Stable partition by bucket(k) = #{splitters <= k} (nut_partition_i64).  Returns
        (partitioned tensor, per-bucket counts)."""
        if col.dtype != torch.int64:
            raise TypeError("partition_i64 takes an int64 column")
        spl = np.ascontiguousarray(np.asarray(splitters, dtype=np.int64))
        n = col.numel()
        if out is None:
            out = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        counts = (C.c_uint64 * (len(spl) + 1))()
        self._bind_stream()
        check(lib.nut_partition_i64(self.ctx, C.c_void_p(_col(col, self.device) if n else None), n,
                                    spl.ctypes.data_as(C.c_void_p) if len(spl) else None, len(spl),
                                    C.c_void_p(out.data_ptr()), counts), "nut_partition_i64")
        return out[:n], [int(c) for c in counts]

    def select_rows(self, cols: list, where: list | None) -> torch.Tensor:
        """Expression-mode scan (nut_select_rows): ascending int64 row ids of the rows where
        the RPN program `where` (ProgQuery node syntax, over `cols`) holds."""
        q = ProgQuery(keys=[], cols=list(cols), aggs=[], where=where)
        spec = q.to_spec(self.device)
        n = int(spec.n)
        out = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        cnt = C.c_uint64()
        self._bind_stream()
        check(lib.nut_select_rows(self.ctx, C.byref(spec), C.c_void_p(out.data_ptr()), C.byref(cnt)),
              "nut_select_rows")
        return out[:cnt.value]

    def hash_partition_i64(self, keys: torch.Tensor, row0: int, nparts: int):
        """The multi-GPU join's exchange step (nut_hash_partition_i64): keys and their row
        ids (row0 + index) grouped by part = dist.join_owner(key, nparts).  Returns
        (keys, rows, per-part counts)."""
        if keys.dtype != torch.int64:
            raise TypeError("hash_partition_i64 takes an int64 column")
        n = keys.numel()
        ok = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        orow = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        counts = (C.c_uint64 * nparts)()
        self._bind_stream()
        check(lib.nut_hash_partition_i64(self.ctx, C.c_void_p(_col(keys, self.device) if n else None), n, nparts,
                                         row0, C.c_void_p(ok.data_ptr()), C.c_void_p(orow.data_ptr()), counts),
              "nut_hash_partition_i64")
        return ok[:n], orow[:n], [int(c) for c in counts]

    # ---------------------------------------------------------------- SQL
    def sql(self, query: str, columns: dict, group_hint: int = 0, right: Optional[dict] = None) -> dict:
        """Parse + lower `query` (nut_sql_plan) and run it on `columns` = {name: CUDA
        tensor}.  Returns {output name: numpy array} in SELECT-list order.  A query with
        a JOIN takes the JOIN source's columns as `right` (`columns` = the FROM table)."""
        from .sql import Plan
        p = Plan(query)
        if isinstance(right, (list, tuple)):  # several JOINs: one dict per JOIN source, in order
            return p.execute_tables(self, [columns] + list(right), group_hint=group_hint)
        if right is not None or "join" in p.describe():
            return p.execute_join(self, columns, right or {}, group_hint=group_hint)
        return p.execute(self, columns, group_hint=group_hint)
