// sql_plan.cpp — the SQL C ABI: parse / tokenize / unescape, plan,
// describe, route, prepare and execute, results.  The six execute entry points (raw columns
// or typed tables; one, two or n tables) check their arguments, wrap their tables as
// TableViews and call one driver, run_plan, which does UNION ALL, derived tables, scalar
// subqueries, `SELECT *`, host staging and the dispatch to the executors once; route,
// prepare and the driver bind plan columns through one bind_columns.  Lowering lives in
// sql_lower.cpp, execution in sql_exec_{scan,groupby,join}.cpp (sql_plan.hpp).
#include "sql_plan.hpp"

namespace {

// a typed table's Date / Datetime column tells the calendar functions its kind
int table_kind_flag(const TCol &c) {
  return c.kind == NUT_COL_DATE ? NUT_COL_AS_DATE : c.kind == NUT_COL_DATETIME ? NUT_COL_AS_DATETIME : 0;
}

// Scalar subqueries (nut_plan.subs): run each (run(sub) executes it over the caller's
// binding), check it returned one value, and copy the plan with every placeholder constant
// replaced by that value.  A global aggregate over no rows is one row of defaults
// (ClickHouse: count / sum / min / max 0, avg NaN); a NaN (or no row) is treated as SQL
// NULL: a WHERE term comparing with it is never true; anywhere else it is rejected.
nut_status resolve_subqueries(const nut_plan &p, nut_plan &q,
                              const std::function<nut_status(const nut_plan *, nut_result **)> &run) {
  std::vector<CVal> vals(p.subs.size());
  std::vector<bool> null(p.subs.size(), false);
  for (size_t i = 0; i < p.subs.size(); ++i) {
    nut_result *r = nullptr;
    nut_status st = run(p.subs[i].get(), &r);
    if (st) return st;
    std::unique_ptr<nut_result, void (*)(nut_result *)> hold(r, nut_result_free);
    if (r->nrows > 1)
      return fail(NUT_ERR_PLAN, "scalar subquery returned " + std::to_string(r->nrows) + " rows (one expected)");
    if (r->nrows == 0 || r->host.empty() || r->host[0].empty()) {
      null[i] = true;
      continue;
    }
    const uint64_t w = r->host[0][0];
    if (r->types[0] != NUT_T_F64 && r->types[0] != NUT_T_I64)  // a dictionary code is no number
      return fail(NUT_ERR_PLAN, "scalar subquery returned a non-numeric value (type " +
                                    std::to_string(r->types[0]) + "); only int64 / float64 results compare");
    if (r->types[0] == NUT_T_F64) {
      double d;
      memcpy(&d, &w, 8);
      if (std::isnan(d)) {  // avg over no rows: comparisons with NaN are never true, as with NULL
        null[i] = true;
        continue;
      }
      if (!std::isfinite(d)) return fail(NUT_ERR_UNSUPPORTED, "scalar subquery returned an infinite value");
      vals[i].is_int = false;
      vals[i].dec = decimal_of(d);
    } else {
      vals[i].is_int = true;
      vals[i].v = (int64_t)w;
    }
  }
  q = p;
  q.subs.clear();
  bool bad_null = false;
  auto put = [&](CVal &c) {
    if (c.param < 0) return;
    if (null[c.param]) bad_null = true;
    c = vals[c.param];
  };
  for (PlanPred &pr : q.preds) {
    if ((pr.c.param >= 0 && null[pr.c.param])) {
      q.never = true;  // col <cmp> NULL: never true (the terms are ANDed)
      pr.c = CVal{};
      continue;
    }
    put(pr.c);
    for (CVal &v : pr.set) put(v);
  }
  auto prog = [&](PProg &pp) {
    for (PNode &n : pp)
      if (n.c.param >= 0) {
        put(n.c);
        n.op = n.c.is_int ? NUT_P_I64 : NUT_P_F64;
      }
  };
  prog(q.where);
  for (PProg &pp : q.proj_val) prog(pp);
  for (PProg &pp : q.proj_mask) prog(pp);
  for (PProg &pp : q.key_progs) prog(pp);
  for (PlanAgg &a : q.aggs) prog(a.val), prog(a.mask), prog(a.ord);
  for (nut_plan::JoinStep &js : q.jn) prog(js.cond);
  std::function<void(HNode &)> hv = [&](HNode &h) {
    if (h.k == H_CONST && h.param >= 0) {
      if (null[h.param]) bad_null = true;
      const CVal &v = vals[h.param];
      h.param = -1;
      if (v.is_int && v.v <= INT64_MAX && v.v >= INT64_MIN) {
        h.is_int = true;
        h.i = (int64_t)v.v;
      } else {
        h.is_int = false;
        h.f = v.is_int ? (double)v.v : v.dec.to_f64();
      }
    }
    for (HNode &k : h.kids) hv(k);
  };
  hv(q.having);
  if (bad_null) return fail(NUT_ERR_UNSUPPORTED, "a scalar subquery returned no row (NULL) where only a WHERE comparison can take it");
  return NUT_OK;
}

// UNION ALL: the branches' results in branch order as one result — device
// columns copied after each other (scans), host columns appended (aggregates), decoded
// strings appended, NULL flags kept per column.  Column names are branch 0's; each
// column's type must agree across the branches.  Frees the parts.
nut_status concat_results(nut_ctx *c, std::vector<nut_result *> &parts, nut_result **out) {
  struct Free {
    std::vector<nut_result *> &v;
    ~Free() {
      for (nut_result *r : v) nut_result_free(r);
    }
  } f{parts};
  const nut_result &r0 = *parts[0];
  const size_t nc = r0.names.size();
  uint64_t total = 0;
  for (size_t k = 0; k < parts.size(); ++k) {
    const nut_result &r = *parts[k];
    if (r.names.size() != nc)
      return fail(NUT_ERR_PLAN, "UNION ALL: branch " + std::to_string(k + 1) + " outputs " + std::to_string(r.names.size()) +
                                    " columns, branch 1 " + std::to_string(nc));
    for (size_t j = 0; j < nc; ++j)
      if (r.types[j] != r0.types[j])
        return fail(NUT_ERR_PLAN, "UNION ALL: column " + std::to_string(j + 1) + " ('" + r0.names[j] +
                                      "') has another type in branch " + std::to_string(k + 1));
    total += r.nrows;
  }
  nut_result *u = new (std::nothrow) nut_result;
  if (!u) return fail(NUT_ERR_OOM, "UNION ALL: out of host memory");
  std::unique_ptr<nut_result, void (*)(nut_result *)> keep(u, nut_result_free);
  u->kind = r0.kind;
  u->device = c->device;
  u->nrows = total;
  u->names = r0.names;
  u->types = r0.types;
  bool any_str = false;
  for (int t : r0.types) any_str |= t == NUT_T_STR;
  if (any_str) {
    u->strs.assign(nc, {});
    for (size_t j = 0; j < nc; ++j)
      if (r0.types[j] == NUT_T_STR)
        for (const nut_result *r : parts)
          if (j < r->strs.size()) u->strs[j].insert(u->strs[j].end(), r->strs[j].begin(), r->strs[j].end());
  }
  if (r0.kind == NUT_PLAN_GROUPBY) {
    u->host.assign(nc, {});
    for (size_t j = 0; j < nc; ++j)
      for (const nut_result *r : parts)
        if (j < r->host.size()) u->host[j].insert(u->host[j].end(), r->host[j].begin(), r->host[j].end());
    *out = keep.release();
    return NUT_OK;
  }
  DeviceGuard g(c->device);
  u->dev_stride = total;
  if (total) NUT_HIP(hipMalloc(&u->dev, total * nc * 8));
  std::vector<int> vcols;  // columns with NULL flags in any branch
  for (size_t j = 0; j < nc; ++j) {
    bool v = false;
    for (const nut_result *r : parts) v |= j < r->valid_of.size() && r->valid_of[j] >= 0 && r->valid;
    u->valid_of.push_back(v ? (int)vcols.size() : -1);
    if (v) vcols.push_back((int)j);
  }
  if (!vcols.empty() && total) NUT_HIP(hipMalloc((void **)&u->valid, total * vcols.size()));
  uint64_t row = 0;
  for (const nut_result *r : parts) {
    if (r->nrows) {
      for (size_t j = 0; j < nc; ++j) {
        NUT_HIP(hipMemcpyAsync((int64_t *)u->dev + j * total + row, (const int64_t *)r->dev + j * r->dev_stride + r->dev_off,
                               r->nrows * 8, hipMemcpyDeviceToDevice, c->stream));
        if (u->valid_of[j] < 0) continue;
        uint8_t *dv = u->valid + (size_t)u->valid_of[j] * total + row;
        if (j < r->valid_of.size() && r->valid_of[j] >= 0 && r->valid)
          NUT_HIP(hipMemcpyAsync(dv, r->valid + (size_t)r->valid_of[j] * r->dev_stride + r->dev_off, r->nrows,
                                 hipMemcpyDeviceToDevice, c->stream));
        else
          NUT_HIP(hipMemsetAsync(dv, 1, r->nrows, c->stream));
      }
    }
    row += r->nrows;
  }
  NUT_HIP(hipStreamSynchronize(c->stream));  // the parts' buffers are freed on return
  *out = keep.release();
  return NUT_OK;
}

// One table as run_plan sees it: the raw nut_column arrays of nut_plan_execute*, or a typed
// table's columns (nut_table_execute*, typed_views).
struct TableView {
  const nut_column *cols = nullptr;
  int ncols = 0;
  uint64_t nrows = 0;
  const Dict *const *dicts = nullptr;  // per column (typed tables); null: raw columns carry no strings
  const char *table = "";  // a typed table's name; empty: raw columns (the text and status of an unbound column)
};

// The exported function a call came through: its name begins the messages, and `tables` is
// how many tables its signature takes (0: any number).
struct Entry {
  const char *name;
  int tables;
};

// NUT_ERR_INVALID_ARG with the message "<who>: <what>"
nut_status bad(const char *who, const std::string &what) { return fail(NUT_ERR_INVALID_ARG, std::string(who) + ": " + what); }
nut_status bad(const Entry &e, const std::string &what) { return bad(e.name, what); }

// Every plan column bound to a column of v (bind()): `SELECT *` is expanded over v's columns
// first (into sq, and p then points at it); each column's type must be known.  An execution
// also needs `*` to stand for something and every column to have data.  dicts (if given):
// the bound columns' dictionaries.
nut_status bind_columns(const char *who, const nut_plan *&p, nut_plan &sq, const TableView &v, bool executing,
                        std::vector<const nut_column *> &bound, std::vector<const Dict *> *dicts = nullptr) {
  if (p->star) {
    std::vector<std::string> names;
    for (int i = 0; i < v.ncols; ++i)
      if (v.cols[i].name) names.push_back(v.cols[i].name);
    if (executing && names.empty()) return bad(who, "SELECT * over no columns");
    p = expand_star(*p, names, sq);
  }
  bound.assign(p->cols.size(), nullptr);
  if (dicts) dicts->assign(p->cols.size(), nullptr);
  for (size_t i = 0; i < p->cols.size(); ++i) {
    const nut_column *b = bound[i] = bind(*p, (int)i, v.cols, v.ncols);
    const std::string &name = p->cols[i];
    if (!b)
      return *v.table ? fail(NUT_ERR_PLAN, std::string("table '") + v.table + "' has no column '" + name + "'")
                      : bad(who, "column '" + name + "' is not bound");
    if (!type_known(col_type(b))) return bad(who, "column '" + name + "' has an unknown type");
    if (executing && v.nrows && !b->data) return bad(who, "column '" + name + "' is NULL");
    if (dicts && v.dicts) (*dicts)[i] = v.dicts[b - v.cols];
  }
  return NUT_OK;
}

nut_status run_plan(nut_ctx *c, const Entry &e, const nut_plan *p, const TableView *v, int nv, uint64_t hint,
                    nut_result **out);

// The rest of a plan over its materialized derived table: the body's result (a group-by:
// host columns) bound by output name as the outer plan's one table (copied into HBM by the
// run, NUT_COL_HOST).  Takes r1.
nut_status run_over_derived(nut_ctx *c, const Entry &e, const nut_plan &p, nut_result *r1, nut_result **out) {
  std::unique_ptr<nut_result, void (*)(nut_result *)> hold(r1, nut_result_free);
  if (r1->kind != NUT_PLAN_GROUPBY || r1->host.size() != r1->names.size())
    return fail(NUT_ERR_UNSUPPORTED, "derived table: its body did not produce a group-by result");
  std::vector<nut_column> cols;
  for (size_t j = 0; j < r1->names.size(); ++j) {
    if (r1->types[j] != NUT_T_I64 && r1->types[j] != NUT_T_F64) continue;  // (string outputs are not read back)
    cols.push_back(nut_column{r1->names[j].c_str(), r1->host[j].data(), r1->types[j] | NUT_COL_HOST});
  }
  nut_plan o = p;
  o.inner.reset();
  const TableView d{cols.data(), (int)cols.size(), r1->nrows, nullptr, ""};
  return run_plan(c, Entry{e.name, 1}, &o, &d, 1, 0, out);
}

// Runs plan p over the tables v[0 .. nv) for entry point e: the one driver behind the six
// nut_plan_execute* / nut_table_execute* functions.  In this order:
//   1. UNION ALL: branch k over table k (one table: every branch over it), concatenated
//   2. a materialized derived table / CTE: its body over the same tables (with the caller's
//      group hint), then the rest over the body's result (hint 0)
//   3. scalar subqueries: each over table 0 (group hint 1), then the plan with their values
//   4. one table: `SELECT *` expanded and every plan column bound (bind_columns)
//   5. host columns staged into HBM (they and the result of 4 live until the run returns)
//   6. the run: exec_scan / exec_groupby over one table, exec_join for a plain two-table
//      JOIN, exec_joinn for a chain (p->jn; one step too: ON filters, EXISTS / IN)
// A plan without a JOIN runs over table 0 whatever nv is (up to two tables).
nut_status run_plan(nut_ctx *c, const Entry &e, const nut_plan *p, const TableView *v, int nv, uint64_t hint,
                    nut_result **out) {
  const Entry one{e.name, 1};
  *out = nullptr;
  if (!p->uni.empty()) {
    if (nv != 1 && (size_t)nv != p->uni.size())
      return bad(e, "a UNION ALL of " + std::to_string(p->uni.size()) +
                                           " branches takes one table per branch (or one for all)");
    std::vector<nut_result *> parts;
    for (size_t k = 0; k < p->uni.size(); ++k) {
      nut_result *r = nullptr;
      nut_status st = run_plan(c, one, p->uni[k].get(), &v[nv == 1 ? 0 : k], 1, hint, &r);
      if (st) {
        for (nut_result *x : parts) nut_result_free(x);
        return st;
      }
      parts.push_back(r);
    }
    return concat_results(c, parts, out);
  }
  if (p->inner) {
    if (e.tables == 1 && p->inner->join >= 0)
      return bad(e, std::string("the derived table has a JOIN (") + e.name + "2)");
    nut_result *r1 = nullptr;
    nut_status st = run_plan(c, e, p->inner.get(), v, nv, hint, &r1);
    return st ? st : run_over_derived(c, e, *p, r1, out);
  }
  // How many tables the plan takes against how many the call gave.  The raw-column entry
  // points refuse a JOIN plan over one table and a chain through the two-table call; the
  // typed-table ones never did: there a JOIN plan over one table fails to bind ("has no
  // column") and a chain is counted by exec_joinn.
  const bool raw = !*v[0].table;
  if (p->jn.empty() && nv > 2) return bad(e, "the plan joins fewer tables");
  const bool single = e.tables == 1 || p->join < 0 || (nv == 1 && p->jn.empty());
  if (single && p->join >= 0 && raw) return bad(e, "the plan has a JOIN (nut_plan_execute2)");
  if (e.tables == 2 && p->jn.size() > 1 && raw)
    return bad(e, "the plan joins several tables (nut_plan_executen)");
  if (!p->subs.empty()) {
    nut_plan q;
    nut_status st = resolve_subqueries(*p, q, [&](const nut_plan *sp, nut_result **r) {
      return run_plan(c, one, sp, v, 1, 1, r);
    });
    return st ? st : run_plan(c, e, &q, v, nv, hint, out);
  }
  DeviceGuard g(c->device);
  const int nt = single ? 1 : nv;
  std::deque<HostStage> hs(nt);
  std::vector<TableView> t(v, v + nt);
  for (int k = 0; k < nt; ++k) {
    nut_status st = stage_host(c, v[k].cols, v[k].ncols, v[k].nrows, hs[k], &t[k].cols);
    if (st) return st;
  }
  nut_plan sq;
  std::vector<const nut_column *> bound;
  std::vector<const Dict *> dicts;
  if (single) {
    nut_status st = bind_columns(e.name, p, sq, t[0], true, bound, &dicts);
    if (st) return st;
  }
  nut_result *r = new (std::nothrow) nut_result;
  if (!r) return fail(NUT_ERR_OOM, std::string(e.name) + ": out of host memory");
  r->kind = p->kind;
  r->device = c->device;
  nut_status st;
  if (single) {
    st = p->kind == NUT_PLAN_GROUPBY ? exec_groupby(c, *p, bound.data(), dicts.data(), t[0].nrows, hint, r)
                                     : exec_scan(c, *p, bound.data(), dicts.data(), t[0].nrows, r);
  } else if (p->jn.empty()) {
    st = exec_join(c, *p, t[0].cols, t[0].ncols, t[0].nrows, t[1].cols, t[1].ncols, t[1].nrows, hint, r, t[0].dicts,
                   t[1].dicts);
  } else {
    std::vector<const nut_column *> cols(nt);
    std::vector<int> ncols(nt);
    std::vector<uint64_t> nrows(nt);
    std::vector<const Dict *const *> tdicts(nt);
    for (int k = 0; k < nt; ++k) cols[k] = t[k].cols, ncols[k] = t[k].ncols, nrows[k] = t[k].nrows, tdicts[k] = t[k].dicts;
    st = exec_joinn(c, *p, cols.data(), ncols.data(), nrows.data(), nt, hint, r, tdicts.data());
  }
  if (st) {
    nut_result_free(r);
    return st;
  }
  *out = r;
  return NUT_OK;
}

// The views of typed tables: every column as a nut_column in its executed type (a Date /
// Datetime column tells the calendar functions its kind) with its dictionary, through one
// DictOverlays for the whole call — the query's own view of the tables' dictionaries
// (substring results).  The tables must be whole (no ragged columns) and on c's device.
struct TypedViews {
  std::vector<std::vector<nut_column>> cols;
  std::vector<std::vector<const Dict *>> dicts;
  DictOverlays ov;
  std::vector<TableView> views;
};
nut_status typed_views(const char *who, nut_ctx *c, nut_table *const *tables, int n, TypedViews &tv) {
  tv.cols.resize(n);
  tv.dicts.resize(n);
  for (int k = 0; k < n; ++k) {
    const nut_table *t = tables[k];
    if (!t) return bad(who, "NULL table");
    if (t->ragged()) return bad(who, "table '" + t->name + "' has ragged columns");
    if (t->device >= 0 && t->device != c->device) return bad(who, "table '" + t->name + "' lives on another device");
    for (const TCol &x : t->cols) {
      tv.cols[k].push_back(nut_column{x.name.c_str(), x.dev, x.exec_type | table_kind_flag(x)});
      tv.dicts[k].push_back(tv.ov.of(x.dict));
    }
    tv.views.push_back(TableView{tv.cols[k].data(), (int)tv.cols[k].size(), t->rows(), tv.dicts[k].data(), t->name.c_str()});
  }
  return NUT_OK;
}

}  // namespace

extern "C" {

nut_status nut_sql_parse(const char *sql, size_t len, nut_stmt **out) {
  if (!out || (!sql && len)) return fail(NUT_ERR_INVALID_ARG, "nut_sql_parse: NULL argument");
  *out = nullptr;
  nut_stmt *s = new (std::nothrow) nut_stmt;
  if (!s) return fail(NUT_ERR_OOM, "nut_sql_parse: out of host memory");
  nut_status st = parse_into(sql ? sql : "", len, s);
  if (st) {
    delete s;
    return st;
  }
  *out = s;
  return NUT_OK;
}

int nut_stmt_kind_of(const nut_stmt *s) { return s ? (int)s->st.k : -1; }

nut_status nut_stmt_dump(const nut_stmt *s, char *buf, size_t cap, size_t *len) {
  if (!s) return fail(NUT_ERR_INVALID_ARG, "nut_stmt_dump: NULL statement");
  return put_text(dump(s->st), buf, cap, len);
}

void nut_stmt_free(nut_stmt *s) { delete s; }

nut_status nut_sql_tokenize(const char *sql, size_t len, int32_t *types, uint64_t *spans, size_t cap, size_t *ntok) {
  if (!ntok || (!sql && len) || (cap && (!types || !spans)))
    return fail(NUT_ERR_INVALID_ARG, "nut_sql_tokenize: NULL argument");
  size_t bad = 0;
  if (!valid_utf8(sql, len, &bad))
    return fail(NUT_ERR_INVALID_ARG, "sql is not valid UTF-8 (byte " + std::to_string(bad) + ")");
  Tokenizer tz(sql ? sql : "", len);
  size_t n = 0;
  for (;;) {
    Token t;
    LexError le;
    if (!tz.next_token(t, le)) {
      *ntok = n;
      return fail(NUT_ERR_PARSE, le.str());
    }
    if (n >= cap) {
      *ntok = n;
      return fail(NUT_ERR_CAPACITY, "nut_sql_tokenize: more than " + std::to_string(cap) + " tokens");
    }
    types[n] = (int32_t)t.t;
    spans[2 * n] = t.span.start;
    spans[2 * n + 1] = t.span.end;
    ++n;
    if (t.t == Tok::Eof) break;
  }
  *ntok = n;
  return NUT_OK;
}

nut_status nut_sql_unescape(const char *s, size_t len, int quote, char *out, size_t cap, size_t *out_len) {
  if (!out_len || (!s && len) || (quote != '\'' && quote != '"'))
    return fail(NUT_ERR_INVALID_ARG, "nut_sql_unescape: bad argument");
  size_t bad = 0;
  if (!valid_utf8(s, len, &bad)) return fail(NUT_ERR_INVALID_ARG, "nut_sql_unescape: input is not valid UTF-8");
  std::string r;
  ParseError pe;
  if (!unescape(sv(s ? s : "", len), (char)quote, r, pe)) return fail(NUT_ERR_PARSE, pe.msg);  // SyntaxError Display
  *out_len = r.size();
  if (r.size() > cap) return fail(NUT_ERR_CAPACITY, "nut_sql_unescape: output needs " + std::to_string(r.size()) + " bytes");
  if (!r.empty()) memcpy(out, r.data(), r.size());
  return NUT_OK;
}

nut_status nut_sql_plan(const char *sql, size_t len, nut_plan **out) {
  if (!out || (!sql && len)) return fail(NUT_ERR_INVALID_ARG, "nut_sql_plan: NULL argument");
  *out = nullptr;
  nut_stmt s;
  nut_status st = parse_into(sql ? sql : "", len, &s);
  if (st) return st;
  nut_plan *p = new (std::nothrow) nut_plan;
  if (!p) return fail(NUT_ERR_OOM, "nut_sql_plan: out of host memory");
  Lowering L;
  if (!lower(s.st, *p, L)) {
    delete p;
    return fail(NUT_ERR_PLAN, "cannot lower to an executor plan: " + L.err);
  }
  *out = p;
  return NUT_OK;
}

int nut_plan_kind_of(const nut_plan *p) { return p ? p->kind : -1; }

nut_status nut_plan_describe(const nut_plan *p, char *buf, size_t cap, size_t *len) {
  if (!p) return fail(NUT_ERR_INVALID_ARG, "nut_plan_describe: NULL plan");
  return put_text(describe(*p), buf, cap, len);
}

nut_status nut_plan_route(const nut_plan *p, const nut_column *cols, int ncols, char *buf, size_t cap, size_t *len) {
  if (!p || (ncols && !cols) || ncols < 0) return fail(NUT_ERR_INVALID_ARG, "nut_plan_route: NULL argument");
  if (p->join >= 0 || p->inner || !p->uni.empty() || !p->subs.empty())
    return fail(NUT_ERR_INVALID_ARG, "nut_plan_route: single-table plans without subqueries or UNION only");
  nut_plan sq;
  std::vector<const nut_column *> bound;
  nut_status bst = bind_columns("nut_plan_route", p, sq, TableView{cols, ncols, 0, nullptr, ""}, false, bound);
  if (bst) return bst;
  std::string route;
  if (p->kind == NUT_PLAN_GROUPBY) {
    nut_agg_spec s;
    ProgStore store;
    std::vector<int> agg_f64;
    GbExtra gx;
    nut_plan nq;  // narrow columns: the expression-mode plan exec_groupby runs
    if (narrow_groupby_plan(*p, bound.data(), nq)) p = &nq;
    // float64 key columns (a Float32 one: widened first) are grouped on int64 key words (exec_groupby)
    std::deque<nut_column> words;
    int nf = 0;
    for (int k : p->keys)
      if (k >= 0 && type_is_float(col_type(bound[k]))) {
        words.push_back(nut_column{bound[k]->name, nullptr, NUT_T_I64});
        bound[k] = &words.back();
        ++nf;
      }
    nut_status st = build_spec(*p, bound.data(), nullptr, 0, s, store, agg_f64, &gx);
    if (st) return st;
    route = gx.active ? "packed-groupby" : p->compiled ? "expr-groupby" : "fused-groupby";
    if (nf) route += " (float64 key words)";
  } else {
    ScanRoute r;
    nut_status st = scan_route(*p, bound.data(), nullptr, &r);
    if (st) return st;
    route = scan_route_name(r);
    if (r == S_RERUN_EXPR) {  // and where the rerun lands
      nut_plan q = *p;
      std::vector<PProg> cs;
      for (const PlanPred &pr : p->preds) cs.push_back(pred_prog(pr));
      q.compiled = true;
      q.preds.clear();
      q.where = and_all(cs);
      st = scan_route(q, bound.data(), nullptr, &r);
      if (st) return st;
      route += std::string(" -> ") + scan_route_name(r);
    }
  }
  return put_text(route, buf, cap, len);
}

void nut_plan_free(nut_plan *p) { delete p; }

// The six execute entry points: argument checks, the tables as views, run_plan.

nut_status nut_plan_execute(nut_ctx *c, const nut_plan *p, const nut_column *cols, int ncols, uint64_t nrows,
                            uint64_t group_hint, nut_result **out) {
  if (!c || !p || !out || (ncols && !cols) || ncols < 0) return fail(NUT_ERR_INVALID_ARG, "nut_plan_execute: NULL argument");
  const TableView v{cols, ncols, nrows, nullptr, ""};
  return run_plan(c, Entry{"nut_plan_execute", 1}, p, &v, 1, group_hint, out);
}

nut_status nut_plan_execute2(nut_ctx *c, const nut_plan *p, const nut_column *left, int nleft, uint64_t lrows,
                             const nut_column *right, int nright, uint64_t rrows, uint64_t group_hint,
                             nut_result **out) {
  if (!c || !p || !out || (nleft && !left) || (nright && !right) || nleft < 0 || nright < 0)
    return fail(NUT_ERR_INVALID_ARG, "nut_plan_execute2: NULL argument");
  const TableView v[2] = {{left, nleft, lrows, nullptr, ""}, {right, nright, rrows, nullptr, ""}};
  return run_plan(c, Entry{"nut_plan_execute2", 2}, p, v, 2, group_hint, out);
}

nut_status nut_plan_executen(nut_ctx *c, const nut_plan *p, const nut_column *const *tables, const int *ncols,
                             const uint64_t *nrows, int ntables, uint64_t group_hint, nut_result **out) {
  if (!c || !p || !out || !tables || !ncols || !nrows || ntables < 1)
    return fail(NUT_ERR_INVALID_ARG, "nut_plan_executen: NULL argument");
  std::vector<TableView> v(ntables);
  for (int k = 0; k < ntables; ++k) {
    if (ncols[k] && !tables[k]) return fail(NUT_ERR_INVALID_ARG, "nut_plan_executen: NULL table");
    v[k] = TableView{tables[k], ncols[k], nrows[k], nullptr, ""};
  }
  return run_plan(c, Entry{"nut_plan_executen", 0}, p, v.data(), ntables, group_hint, out);
}

nut_status nut_plan_prepare(const nut_plan *p, const nut_column *cols, int ncols) {
  if (!p || (ncols && !cols) || ncols < 0) return fail(NUT_ERR_INVALID_ARG, "nut_plan_prepare: NULL argument");
  if (p->inner) return nut_plan_prepare(p->inner.get(), cols, ncols);  // (the rest compiles when it runs)
  for (const auto &b : p->uni) {  // UNION ALL: every branch whose columns are all given
    bool all = true;
    for (const std::string &n : b->cols) {
      bool found = false;
      for (int i = 0; i < ncols && !found; ++i) found = cols[i].name && n == cols[i].name;
      all = all && found;
    }
    if (all) {
      nut_status st = nut_plan_prepare(b.get(), cols, ncols);
      if (st) return st;
    }
  }
  if (!p->uni.empty()) return NUT_OK;
  bool any_narrow = false;
  for (int i = 0; i < ncols; ++i) {
    const int t = col_type(&cols[i]) & ~NUT_COL_HOST;
    any_narrow = any_narrow || (type_known(t) && type_width(t) < 8);
  }
  if (!p->compiled && !(any_narrow && p->kind == NUT_PLAN_GROUPBY)) return NUT_OK;  // precompiled kernels only
  // scalar subqueries: their values (int64 or f64 constants) decide the program types, so
  // the shape is compiled when the plan executes with the values in place
  if (!p->subs.empty()) return NUT_OK;
  std::vector<nut_column> typed(cols, cols + ncols);
  for (nut_column &col : typed) col.type &= ~NUT_COL_HOST;  // only the type matters here
  nut_plan sq;
  std::vector<const nut_column *> bound;
  nut_status bst = bind_columns("nut_plan_prepare", p, sq, TableView{typed.data(), ncols, 0, nullptr, ""}, false, bound);
  if (bst) return bst;
  nut_plan nq;  // narrow columns: the expression-mode plan that executes (a Float32 key is widened there)
  if (p->kind == NUT_PLAN_GROUPBY && narrow_groupby_plan(*p, bound.data(), nq)) {
    for (int k : nq.keys)  // (a Float32 key groups on key words made at execution: compiled then)
      if (k >= 0 && col_narrow(bound[k])) return NUT_OK;
    p = &nq;
  }
  nut_agg_spec s;
  ProgStore store;
  std::vector<int> agg_f64;
  nut_status st = build_spec(*p, bound.data(), nullptr, 0, s, store, agg_f64);
  if (st) return st;
  st = p->kind == NUT_PLAN_GROUPBY ? nut_groupby_jit_compile(&s) : nut_select_jit_compile(&s);
  // computed projections: their evaluation kernels (groups of NUT_MAX_AGGS, as executed)
  std::vector<size_t> comp;
  for (size_t j = 0; j < p->projs.size(); ++j)
    if (computed_proj(*p, j)) comp.push_back(j);
  for (size_t g0 = 0; g0 < comp.size() && !st; g0 += NUT_MAX_AGGS) {
    nut_plan q;
    q.compiled = true;
    q.cols = p->cols;
    for (size_t t = g0; t < comp.size() && t < g0 + NUT_MAX_AGGS; ++t) {
      PlanAgg a{};
      a.op = NUT_AGG_SUM;
      a.val = p->proj_val[comp[t]];
      a.mask = p->proj_mask[comp[t]];
      q.aggs.push_back(std::move(a));
    }
    nut_agg_spec es;
    ProgStore estore;
    std::vector<int> f64;
    st = build_spec(q, bound.data(), nullptr, 0, es, estore, f64);
    if (!st) st = nut_eval_jit_compile(&es);
  }
  return st;
}

nut_status nut_table_execute(nut_ctx *c, nut_table *t, const nut_plan *p, uint64_t group_hint, nut_result **out) {
  if (!c || !t || !p || !out) return fail(NUT_ERR_INVALID_ARG, "nut_table_execute: NULL argument");
  TypedViews tv;
  nut_status st = typed_views("nut_table_execute", c, &t, 1, tv);
  return st ? st : run_plan(c, Entry{"nut_table_execute", 1}, p, tv.views.data(), 1, group_hint, out);
}

nut_status nut_table_execute2(nut_ctx *c, nut_table *left, nut_table *right, const nut_plan *p, uint64_t group_hint,
                              nut_result **out) {
  if (!c || !left || !right || !p || !out) return fail(NUT_ERR_INVALID_ARG, "nut_table_execute2: NULL argument");
  nut_table *const tables[2] = {left, right};
  TypedViews tv;
  nut_status st = typed_views("nut_table_execute2", c, tables, 2, tv);
  return st ? st : run_plan(c, Entry{"nut_table_execute2", 2}, p, tv.views.data(), 2, group_hint, out);
}

nut_status nut_table_executen(nut_ctx *c, nut_table *const *tables, int ntables, const nut_plan *p,
                              uint64_t group_hint, nut_result **out) {
  if (!c || !tables || ntables < 1 || !p || !out) return fail(NUT_ERR_INVALID_ARG, "nut_table_executen: NULL argument");
  TypedViews tv;
  nut_status st = typed_views("nut_table_executen", c, tables, ntables, tv);
  return st ? st : run_plan(c, Entry{"nut_table_executen", 0}, p, tv.views.data(), ntables, group_hint, out);
}

nut_status nut_result_string(const nut_result *r, int j, uint64_t row, const char **str, size_t *len) {
  if (!r || j < 0 || j >= (int)r->names.size() || !str || !len)
    return fail(NUT_ERR_INVALID_ARG, "nut_result_string: bad argument");
  if (r->types[j] != NUT_T_STR || (size_t)j >= r->strs.size())
    return fail(NUT_ERR_INVALID_ARG, "nut_result_string: column is not a string column");
  if (row >= r->nrows) return fail(NUT_ERR_INVALID_ARG, "nut_result_string: row out of range");
  const std::string &v = r->strs[j][row];
  *str = v.data();
  *len = v.size();
  return NUT_OK;
}

nut_status nut_result_shape(const nut_result *r, uint64_t *nrows, int *ncols) {
  if (!r) return fail(NUT_ERR_INVALID_ARG, "nut_result_shape: NULL result");
  if (nrows) *nrows = r->nrows;
  if (ncols) *ncols = (int)r->names.size();
  return NUT_OK;
}

nut_status nut_result_column(const nut_result *r, int j, int *type, const char **name) {
  if (!r || j < 0 || j >= (int)r->names.size()) return fail(NUT_ERR_INVALID_ARG, "nut_result_column: bad column");
  if (type) *type = r->types[j];
  if (name) *name = r->names[j].c_str();
  return NUT_OK;
}

nut_status nut_result_to_host(const nut_result *r, int j, void *dst, uint64_t cap) {
  if (!r || j < 0 || j >= (int)r->names.size()) return fail(NUT_ERR_INVALID_ARG, "nut_result_to_host: bad column");
  if (r->nrows > cap) return fail(NUT_ERR_CAPACITY, "nut_result_to_host: capacity < " + std::to_string(r->nrows));
  if (r->nrows == 0) return NUT_OK;
  if (!dst) return fail(NUT_ERR_INVALID_ARG, "nut_result_to_host: NULL dst");
  if (r->kind == NUT_PLAN_GROUPBY) {
    if (r->types[j] == NUT_T_STR)
      return fail(NUT_ERR_INVALID_ARG, "nut_result_to_host: string column (use nut_result_string)");
    memcpy(dst, r->host[j].data(), r->nrows * 8);
    return NUT_OK;
  }
  if (r->types[j] == NUT_T_STR) return fail(NUT_ERR_INVALID_ARG, "nut_result_to_host: string column (use nut_result_string)");
  DeviceGuard g(r->device);
  NUT_HIP(hipMemcpy(dst, (const int64_t *)r->dev + (uint64_t)j * r->dev_stride + r->dev_off, r->nrows * 8,
                    hipMemcpyDeviceToHost));
  return NUT_OK;
}

nut_status nut_result_device_column(const nut_result *r, int j, const void **dev) {
  if (!r || !dev || j < 0 || j >= (int)r->names.size())
    return fail(NUT_ERR_INVALID_ARG, "nut_result_device_column: bad argument");
  if (r->kind == NUT_PLAN_GROUPBY)
    return fail(NUT_ERR_UNSUPPORTED, "nut_result_device_column: group results live on the host");
  *dev = r->dev ? (const void *)((const int64_t *)r->dev + (uint64_t)j * r->dev_stride + r->dev_off) : nullptr;
  return NUT_OK;
}

nut_status nut_result_device(const nut_result *r, const void **dev) {
  if (!r || !dev) return fail(NUT_ERR_INVALID_ARG, "nut_result_device: NULL argument");
  if (r->kind == NUT_PLAN_GROUPBY) return fail(NUT_ERR_UNSUPPORTED, "nut_result_device: group results live on the host");
  *dev = r->dev ? (const void *)((const int64_t *)r->dev + r->dev_off) : nullptr;
  return NUT_OK;
}

void nut_result_free(nut_result *r) {
  if (!r) return;
  if (r->dev) {
    DeviceGuard g(r->device);
    (void)hipFree(r->dev);
  }
  if (r->valid) {
    DeviceGuard g(r->device);
    (void)hipFree(r->valid);
  }
  delete r;
}

nut_status nut_result_validity(const nut_result *r, int j, const uint8_t **dev) {
  if (!r || !dev || j < 0 || j >= (int)r->names.size()) return fail(NUT_ERR_INVALID_ARG, "nut_result_validity: bad argument");
  const int v = j < (int)r->valid_of.size() ? r->valid_of[j] : -1;
  *dev = v >= 0 && r->valid ? r->valid + (uint64_t)v * r->dev_stride + r->dev_off : nullptr;
  return NUT_OK;
}

nut_status nut_result_validity_to_host(const nut_result *r, int j, uint8_t *dst, uint64_t cap) {
  const uint8_t *dev = nullptr;
  nut_status s = nut_result_validity(r, j, &dev);
  if (s) return s;
  if (r->nrows > cap) return fail(NUT_ERR_CAPACITY, "nut_result_validity_to_host: capacity < " + std::to_string(r->nrows));
  if (r->nrows == 0) return NUT_OK;
  if (!dst) return fail(NUT_ERR_INVALID_ARG, "nut_result_validity_to_host: NULL dst");
  if (!dev) {
    memset(dst, 1, r->nrows);
    return NUT_OK;
  }
  DeviceGuard g(r->device);
  NUT_HIP(hipMemcpy(dst, dev, r->nrows, hipMemcpyDeviceToHost));
  return NUT_OK;
}

}  // extern "C"

