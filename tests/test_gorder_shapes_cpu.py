"""CPU: every note of tests/gorder_shapes.py proven without a GPU.  Each case's modelled sample
(keys[::n // 65536][:65536]) and its whole key column go to the stand-alone plan driver
(tests/c/test_go_plan.cpp: csrc/go_plan.hpp itself, built as test_go_plan_cpu.py builds it), and
the notes are asserted from the driver's output: the heavy set as keys, the range and t, the
admission, exact or capped, the cell counts a case states, hq, the cuckoo slots, and the decline
reason where the plan's own arithmetic decides it (an exhausted arena, a region larger than the
ordering pass holds, more distinct keys in a region than a table admits).  The oracle alone must
give the group count and the heavy rows each note claims, so that no GPU assertion of
test_gpu_gorder_paths.py rests on something unchecked."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gorder_shapes as S
from groupby_shapes import library_layout

ROOT = Path(__file__).resolve().parent.parent
SHAPE, CLUSTERED = 1, 2  # nutexec.h NUT_GB_DECLINE_*
NAS = (1, 4, 5)  # the aggregate counts of the GPU tests' shapes


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("go_shapes") / "test_go_plan"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "nutdb_amd" / "csrc"),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "c" / "test_go_plan.cpp"), "-o", str(out)], check=True)
    return out


def run(exe, lines):
    r = subprocess.run([str(exe)], input="".join(x + "\n" for x in lines), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = []
    for ln in r.stdout.splitlines():
        w = ln.split()
        out.append((w[0], [float(x) if "." in x or "e" in x else int(x) for x in w[1:]]))
    return out


class Plan:
    """what the driver says about a case at `na` aggregates (default options, gb_l0_bits = 7)"""

    def __init__(self, exe, case, na, tmp, nstore=2, columns=True, keep_capped=0):
        keys, n = case.keys, len(case.keys)
        self.exe, self.n = exe, n
        sf, kf = tmp / "sample.bin", tmp / "keys.bin"
        S.sample_of(keys).tofile(sf)
        out = run(exe, [f"samplef {sf}"])
        assert out[0][1][:2] == [0, S.SAMPLE]
        self.smin, self.smax = out[0][1][2:]
        lam = case.hint / S.CELLS
        self.head = [f"samplef {sf}", f"range {self.smin} {self.smax}"]
        out = run(exe, self.head + ["admit 7", f"heavy {na}"])
        self.range_why, *rg = out[1][1]
        self.rg = tuple(rg[:2]) + (rg[2], rg[3])
        self.admit = out[2][1][0]
        self.heavy = np.array([x[1][0] for x in out[4:]], dtype=np.int64)
        self.hk = {x[1][0]: x[1][1:] for x in out[4:]}  # key -> a, slot[a], b, slot[b]
        self.head.append(f"heavy {na}")
        self.why = self.range_why or self.admit
        if self.why or not columns:
            return
        nh = len(self.heavy)
        out = run(exe, self.head + [f"sizes {n} 7 {nstore} {lam!r} {int(nh > 0)} {keep_capped}"])
        (self.exact, self.slack1, self.rows, self.arena1, self.b2rows, self.ocap, self.abase0, self.acap0,
         _) = out[-1][1][1:]
        keys.tofile(kf)
        out = run(exe, self.head + [f"hist {kf} {n}"])
        _, self.kept, self.heavy_rows, _ = out[-2][1]
        c = np.array(out[-1][1], dtype=np.int64).reshape(-1, 2)
        self.cells = np.zeros(S.CELLS, np.int64)
        self.cells[c[:, 0]] = c[:, 1]
        self.digit_rows = self.cells.reshape(128, 128).sum(axis=1)
        kf.unlink()
        # (later commands get the same counts without the column's file)
        self.head.append(f"counts {len(c)} " + " ".join(f"{q} {r}" for q, r in c.tolist()))

    def cell(self, keys):
        keys = np.atleast_1d(np.asarray(keys, dtype=np.int64))
        out = run(self.exe, self.head[:2] + [f"cell {len(keys)}"] + [str(int(k)) for k in keys])
        return np.array(out[-1][1][1:], dtype=np.int64)

    def slots(self, keys):
        out = run(self.exe, self.head[:3] + [f"slots {len(keys)}"] + [str(int(k)) for k in keys])
        return {x[1][0]: x[1][1:] for x in out if x[0] == "sl"}

    def level1_exact(self):
        """-> (l0 why, dig0, l1 why, hq) of the exact layout from the kept rows' cell counts"""
        out = run(self.exe, self.head + [f"hcount 1 {self.n} {self.kept}", f"l0 1 {self.n} 7 {self.rows} 0",
                                         f"l1 1 7 1.0 {self.b2rows} 1024"])
        d = {}
        for name, v in out:
            d.setdefault(name, v)
        return d["l0"][0], d["dig0"], d["l1"][0], np.array(d["hq"], dtype=np.int64)

    def level1_capped(self):
        """the capped layout, level 0's regions holding min(rows, ocap) each -> (level-1 region rows
        per cell [128 x 128], acap1)"""
        took = np.minimum(self.digit_rows, self.ocap)
        ne = np.flatnonzero(took)
        pairs = " ".join(f"{d * self.ocap} {d * self.ocap + took[d]}" for d in ne)
        out = run(self.exe, self.head + ["hcount 0 0", f"l0 0 {self.n} 7 {self.rows} {self.ocap} {len(ne)} {pairs}",
                                         f"l1 0 7 {self.slack1!r} {self.b2rows} 1024"])
        d = {}
        for name, v in out:
            d.setdefault(name, v)
        assert d["l0"][0] == 0 and d["l1"][0] == 0 and d["dig0"] == ne.tolist()
        cap1 = np.zeros((128, 128), np.int64)
        cap1[ne] = np.array(d["s2"], dtype=np.int64).reshape(-1, 5)[:, 4][:, None]
        return cap1, d["l1"][2]


def oracle_counts(orc, case):
    k, w = orc.groupby([case.keys], [(1, 0, ())])
    return k[:, 0], w[:, 0].astype(np.int64)


def check_common(case, plan, orc):
    """the heavy set (as keys), the verdict before any work, exact or capped, heavy rows and group
    count (driver and oracle)"""
    note = case.note
    assert np.array_equal(plan.heavy, note["heavy"])
    if note["decline"] == "shape":
        assert plan.why == SHAPE
        return None, None
    assert plan.why == 0
    assert bool(plan.exact) == bool(note["exact"])
    assert plan.heavy_rows == note["heavy_rows"] and plan.kept == len(case.keys) - note["heavy_rows"]
    gk, gc = oracle_counts(orc, case)
    assert len(gk) == note["groups"]
    assert int(gc[np.isin(gk, note["heavy"])].sum()) == note["heavy_rows"]
    assert np.isin(note["heavy"], gk).all()
    return gk, gc


def check_capped_fits(plan):
    """no row can reach an arena: every level-0 digit within its region, every cell within its
    level-1 region"""
    assert plan.digit_rows.max() <= plan.ocap
    cap1, _ = plan.level1_capped()
    assert np.all(plan.cells.reshape(128, 128) <= cap1)


def check_exact(case, plan):
    l0why, dig0, l1why, hq = plan.level1_exact()
    assert l0why == 0
    note = case.note
    if note["digits"] is not None:
        assert len(dig0) == note["digits"]
    assert np.array_equal(plan.heavy[hq < 0], note["hq_missing"])
    return dig0, l1why, hq


# ----------------------------------------------------------------------------- the model
def test_model_matches_driver(exe, tmp_path):
    rng = np.random.default_rng(3)
    for case in (S.gap(), S.outliers("dense"), S.outliers("negative"), S.tiny_span()):
        plan = Plan(exe, case, 4, tmp_path, columns=False)
        rg = S.range_of(case.keys)
        assert plan.rg == rg
        lo_s, hi_s = S.signed(rg[0]), S.signed(rg[0] + rg[1])
        probe = np.concatenate([rng.integers(S.I64_MIN, S.I64_MAX, 2000, dtype=np.int64),
                                rng.integers(lo_s, hi_s, 20000, dtype=np.int64, endpoint=True),
                                np.array([S.I64_MIN, S.I64_MAX, lo_s, hi_s, lo_s - 1, hi_s + 1])])
        assert np.array_equal(S.cell(rg, probe), plan.cell(probe))
    for na in (1, 4):
        case = S.sampled_heavy(na)
        plan = Plan(exe, case, na, tmp_path, columns=False)
        assert np.array_equal(S.heavy_model(S.sample_of(case.keys), na), plan.heavy)
        slot = S.cuckoo(plan.heavy)
        for j, k in enumerate(plan.heavy.tolist()):
            a, sa, b, sb = plan.hk[k]
            assert (slot[a], slot[b]) == (sa, sb) and j + 1 in (sa, sb)


def test_value_columns():
    n = 1 << 16
    f = S.value_column("f", n, 1)
    assert np.all(f * 1024 == np.round(f * 1024)) and np.abs(f).max() < 2**19
    assert np.signbit(f[::97]).all() and np.all(f[::97] == 0)
    assert np.abs(S.value_column("i", n, 2)).max() < 2**40
    assert np.abs(S.value_column("w", n, 3)).max() > 2**62
    for shape, (kinds, aggs) in S.SHAPES.items():
        assert all(col is None or col < len(kinds) for _, col in aggs) and S.shape_na(shape) in NAS


# ----------------------------------------------------------------------------- the cases
CAPPED = [(S.sampled_heavy, (4,)), (S.heavy_blocks, (0, False)), (S.gap, ()), (S.gap, (18, 6, True)), (S.cuckoo_neighbours, (4,)),
          (S.identity_keys, ()), (S.hidden_key, (8, True))]


@pytest.mark.parametrize("builder,args", CAPPED)
def test_capped_behind_heavy_pass(exe, tmp_path, builder, args):
    """gb_heavy = 2 (capped regions of 2.5 x the even share behind the heavy pass): arenas_capped False
    means no kept row can leave its regions, True that some must"""
    case = builder(*args)
    plan = Plan(exe, case, 4, tmp_path, keep_capped=1)
    assert not plan.exact and plan.slack1 == 2.5 and len(plan.heavy) > 0
    if case.note["arenas_capped"]:
        cap1, _ = plan.level1_capped()
        assert plan.digit_rows.max() > plan.ocap or np.any(plan.cells.reshape(128, 128) > cap1)
    else:
        assert case.note["arenas_capped"] is False
        check_capped_fits(plan)


def test_plain(exe, orc, tmp_path):
    case = S.plain()
    plan = Plan(exe, case, 4, tmp_path)
    check_common(case, plan, orc)
    check_capped_fits(plan)


@pytest.mark.parametrize("na", [1, 4, 5])
def test_sampled_heavy(exe, orc, tmp_path, na):
    """the cut: heavy_max(na) keys chosen, the 64 spare candidates (sampled 3 times) dropped"""
    case = S.sampled_heavy(na)
    plan = Plan(exe, case, na, tmp_path)
    gk, gc = check_common(case, plan, orc)
    assert len(plan.heavy) == S.heavy_max(na) == min(2048, 2048 // na)
    smp = S.sample_of(case.keys)
    assert all(int((smp == k).sum()) == 3 for k in case.note["spare"]) and not np.isin(case.note["spare"], plan.heavy).any()
    assert case.note["heavy_rows"] == len(plan.heavy) * case.note["each"] < len(case.keys) // 100
    check_exact(case, plan)


@pytest.mark.parametrize("with_heavy", [False, True])
def test_hidden_key(exe, orc, tmp_path, with_heavy):
    case = S.hidden_key(8, with_heavy)
    plan = Plan(exe, case, 4, tmp_path)
    gk, gc = check_common(case, plan, orc)
    x = case.note["hidden"]
    assert int(gc[gk == x][0]) == case.note["hidden_rows"] == len(case.keys) // 32
    assert not np.isin(x, S.sample_of(case.keys))
    c = int(plan.cell(x)[0])
    if with_heavy:  # exact: one huge cell
        check_exact(case, plan)
        assert plan.cells[c] >= case.note["hidden_rows"] and plan.cells[c] > 100 * np.median(plan.cells)
    else:  # capped: its level-0 digit outgrows its region, so rows must go to level 0's arena and fit there
        assert case.note["arenas"] and plan.digit_rows[c >> 7] > plan.ocap
        assert plan.digit_rows[c >> 7] < plan.acap0


TAILS = [(0, False), (0, True), (1, True), (1, False), (2047, True), (2049, False), (4099, True)]


@pytest.mark.parametrize("tail,last_heavy", TAILS)
def test_heavy_blocks(exe, orc, tmp_path, tail, last_heavy):
    case = S.heavy_blocks(tail, last_heavy)
    plan = Plan(exe, case, 4, tmp_path)
    check_common(case, plan, orc)
    check_exact(case, plan)
    keys, n = case.keys, len(case.keys)
    assert n == S.N0 + tail and n // S.SAMPLE == S.STEP
    hv = keys == plan.heavy[0]
    assert (hv[n - 1]) == last_heavy
    assert hv[S.HB_ALL[0]:S.HB_ALL[1]].all()
    a, b = S.HB_ONE_PER_TILE
    t = (~hv[a:b]).reshape(-1, S.HK_TILE)
    assert np.all(t.sum(axis=1) == 1)
    at = t.argmax(axis=1)  # thread = at % 256 (lane = at % 64), item = at // 256
    assert len(set((at % 64).tolist())) == 64 and len(set((at // 256).tolist())) == 8
    alt = hv[S.HB_ALTERNATE[0]:S.HB_ALTERNATE[1]]
    assert alt[1::2].all() and not alt[0::2].any()
    for off, ln in S.HB_EDGE_BLOCKS:
        r0 = S.HB_EDGES + off
        assert hv[r0:r0 + ln].all() and not hv[r0 - 1] and not hv[r0 + ln]
    assert any(off % S.HK_TILE for off, _ in S.HB_EDGE_BLOCKS) and any((off + ln) % S.HK_TILE for off, ln in S.HB_EDGE_BLOCKS)
    a, b = S.HB_ONE_PER_WG
    lone = case.note["lone_row"]
    assert int((~hv[a:b]).sum()) == 1 and not hv[lone]
    # any heavy-pass grid (256 or 304 CUs, 1..8 workgroups per CU): whole workgroups keep nothing, one keeps
    # exactly one row; with a tail, trailing workgroups have no tile at all
    trailing = {256: 0, 304: 0}
    pow2 = 0
    for cus in (256, 304):
        for per_cu in range(1, 9):
            why, ntiles, hgrid, chunk = run(exe, [f"grid {n} {cus} {per_cu}"])[0][1]
            assert why == 0 and ntiles == -(-n // S.HK_TILE)
            rows = chunk * S.HK_TILE
            kept = np.add.reduceat((~hv).astype(np.int64), np.arange(0, n, rows))
            assert (kept == 0).any() and kept[lone // rows] == 1
            trailing[cus] += int((hgrid - 1) * chunk >= ntiles)
            pow2 += int((hgrid - 1) * chunk >= ntiles and cus == 256 and per_cu in (1, 2, 4, 8))
    # workgroups without a tile (count[b] = 0 without a load): some grid leaves them at every size; the
    # power-of-two grids divide the 8192 tiles of 2^24 rows evenly and leave them only with a tail
    assert trailing[256] > 0 and trailing[304] > 0 and (pow2 > 0) == (tail > 0)


@pytest.mark.parametrize("logp,s,hidden", [(18, 6, False), (18, 6, True), (22, 7, False)])
def test_gap(exe, orc, tmp_path, logp, s, hidden):
    case = S.gap(logp, s, hidden)
    plan = Plan(exe, case, 4, tmp_path)
    gk, gc = check_common(case, plan, orc)
    dig0, l1why, hq = check_exact(case, plan)
    assert l1why == 0 and len(case.note["hq_missing"]) == 4 and (hq >= 0).sum() == 8
    note = case.note
    kept = gk[~np.isin(gk, plan.heavy)]
    kc = plan.cell(kept)
    hc = dict(zip(plan.heavy.tolist(), plan.cell(plan.heavy).tolist()))
    hqd = dict(zip(plan.heavy.tolist(), hq.tolist()))
    k, k1 = note["adjacent"]
    assert k1 == k + 1 and hc[k] == hc[k1] and hqd[k] == hqd[k1] >= 0   # two heavy keys in one partition
    m = note["middle"]
    assert m[3] == m[2] + 1 and hc[m[2]] == hc[m[3]]
    own = kept[kc == hc[note["below"]]]
    assert len(own) > 0 and note["below"] < own.min()
    own = kept[kc == hc[note["above"]]]
    assert len(own) > 0 and note["above"] > own.max()
    assert not (kc == hc[note["alone"]]).any() and hqd[note["alone"]] >= 0
    assert plan.cells[hc[note["alone"]]] == 0 and list(hc.values()).count(hc[note["alone"]]) == 1  # a partition of 1 group
    p0, p1 = note["pair"]  # a partition of exactly 2 groups: no kept row in the cell, both keys (and no other) inserted there
    assert p1 == p0 + 1 and hc[p0] == hc[p1] and plan.cells[hc[p0]] == 0 and not (kc == hc[p0]).any()
    assert hqd[p0] == hqd[p1] >= 0 and list(hqd.values()).count(hqd[p0]) == 2 and hqd[p0] != hqd[note["alone"]]
    # the middle holds no kept key
    assert len(dig0) < 128 and not np.isin([hc[x] >> 7 for x in m], dig0).any()
    if logp == 22:  # more groups than a result of 2 x hint rows holds (Executor.groupby_to_host's first arrays)
        assert note["groups"] > 2 * case.hint and len(case.keys) >= 4 * case.hint
    if hidden:
        x, late = note["hidden"], note["late"]
        assert len(case.keys) // 32 - 64 <= int(gc[gk == x][0]) <= len(case.keys) // 32 and not np.isin(np.append(late, x), S.sample_of(case.keys)).any()
        assert np.all(plan.cell(late) == plan.cell(x)[0]) and np.all(gc[np.isin(gk, late)] == 4)
        assert np.flatnonzero(np.isin(case.keys, late)).min() >= 7 * (len(case.keys) // 8)


@pytest.mark.parametrize("geom", ["full", "dense", "negative", "straddle", "tiny"])
def test_outliers(exe, orc, tmp_path, geom):
    case = S.tiny_span() if geom == "tiny" else S.outliers(geom)
    plan = Plan(exe, case, 4, tmp_path)
    gk, gc = check_common(case, plan, orc)
    note = case.note
    assert plan.rg[2] == note["t"] and (note["t"] > 0) == (geom in ("full", "negative"))
    lo_s, hi_s = S.signed(plan.rg[0]), S.signed(plan.rg[0] + plan.rg[1])
    assert note["below"].max() < lo_s and note["above"].min() > hi_s
    assert note["below"][0] == S.I64_MIN and note["above"][-1] == S.I64_MAX
    assert np.all(plan.cell(note["below"]) == 0) and np.all(plan.cell(note["above"]) == plan.cell(hi_s)[0])
    out = np.concatenate([note["below"], note["above"]])
    assert len(out) == 48 and not np.isin(out, S.sample_of(case.keys)).any()
    assert np.all(gc[np.isin(gk, out)] == 8)
    if geom == "negative":
        assert hi_s < 0
    if geom in ("full", "straddle"):
        assert lo_s < 0 < hi_s
    if geom == "dense":
        kept = gk[~np.isin(gk, out)]
        assert np.array_equal(kept, np.arange(S.G0))  # ids: every partition's span is below 2^32 (sh = 0)
    if geom == "tiny":
        assert plan.rg[1] == 1 << 16  # the smallest span go_range accepts
    check_capped_fits(plan)


def test_clustered(exe, orc, tmp_path):
    case = S.clustered()
    plan = Plan(exe, case, 4, tmp_path)
    assert plan.range_why == 0 and plan.admit == CLUSTERED and len(plan.heavy) == 0
    gk, gc = oracle_counts(orc, case)
    assert len(gk) == case.note["groups"] == S.G0
    assert len(set(plan.cell(gk[(gk > S.okey(100000)) & (gk <= S.okey(100000) + S.G0 // 2)]).tolist())) == 1


def test_tiny_span_declined(exe, orc, tmp_path):
    case = S.tiny_span(False)
    plan = Plan(exe, case, 4, tmp_path)
    check_common(case, plan, orc)
    assert plan.range_why == SHAPE and case.note["top"] == S.smallest_span() - 1


@pytest.mark.parametrize("na", [1, 4])
def test_cuckoo_neighbours(exe, orc, tmp_path, na):
    case = S.cuckoo_neighbours(na)
    plan = Plan(exe, case, na, tmp_path)
    gk, gc = check_common(case, plan, orc)
    nb = case.note["neighbours"]
    assert len(nb) == 64 and not np.isin(nb, plan.heavy).any() and np.all(gc[np.isin(gk, nb)] == 4)
    assert not np.isin(nb, S.sample_of(case.keys)).any()
    for k, (a, sa, b, sb) in plan.slots(nb).items():
        assert sa != 0 and sb != 0  # both of its slots name heavy keys
    second = [k for j, k in enumerate(plan.heavy.tolist()) if plan.hk[k][1] != j + 1]
    assert second == case.note["second_slot"].tolist() and len(second) > 0
    assert all(plan.hk[k][3] == plan.heavy.tolist().index(k) + 1 for k in second)
    check_exact(case, plan)


def test_identity(exe, orc, tmp_path):
    case = S.identity_keys()
    plan = Plan(exe, case, 4, tmp_path)
    check_common(case, plan, orc)
    check_exact(case, plan)
    z = case.note["z"]
    assert z in plan.heavy
    for shape, want in S.IDENTITY_WORDS.items():
        cols = S.identity_columns(shape, case)
        k, w = orc.groupby([case.keys], S.identity_aggs(shape), values=cols)
        row = w[k[:, 0] == z][0]
        assert tuple(int(x) for x in row[:3]) == want, shape  # the oracle's aggregates ARE the initial words
        assert int(row[3]) == 512
        yrow = w[k[:, 0] == case.note["y"]][0]  # Y: the next aggregate's initial word, not its own
        for a, o in enumerate(S.OTHER_KIND_WORDS[shape]):
            nxt = S.IDENTITY_WORDS[shape][a + 1] if a + 1 < 3 else 0  # (COUNT starts at 0)
            assert o is None or (int(yrow[a]) == o == nxt and o != want[a])


def test_arena_level0(exe, orc, tmp_path):
    case = S.arena_level0()
    plan = Plan(exe, case, 4, tmp_path)
    check_common(case, plan, orc)
    d = int(plan.cell(case.note["hidden"])[0]) >> 7
    assert case.note["hidden_rows"] * 10 > len(case.keys) * 6
    assert plan.digit_rows[d] - plan.ocap > plan.acap0  # more rows past the region than the arena holds


def test_arena_level1(exe, orc, tmp_path):
    case = S.arena_level1()
    plan = Plan(exe, case, 4, tmp_path)
    check_common(case, plan, orc)
    assert plan.digit_rows.max() <= plan.ocap  # level 0 fits: its arena stays empty
    cap1, acap1 = plan.level1_capped()
    over = np.maximum(plan.cells.reshape(128, 128) - cap1, 0)
    assert (over > 0).sum() == 128 and over.sum() > acap1  # level 1's arena cannot hold the 128 cells' excess


def test_table_overflow(exe, orc, tmp_path):
    case = S.table_overflow()
    plan = Plan(exe, case, 4, tmp_path)
    gk, gc = check_common(case, plan, orc)
    c = case.note["cell"]
    mine = plan.cell(gk) == c
    assert mine.sum() == case.note["cell_keys"] == plan.cells[c] and np.all(gc[mine] == 1)  # one row per key
    assert plan.digit_rows.max() <= plan.ocap
    cap1, acap1 = plan.level1_capped()
    region = int(cap1[c >> 7, c & 127])
    assert region < plan.cells[c] and plan.cells[c] - region < acap1  # (the excess fits the arena: not "arena")
    per = max(64, 2 * -(-case.hint // S.CELLS))
    for na in NAS:  # whatever rows the region takes, they are more keys than the table's slots
        assert region > library_layout(1, na, per, segment=1)["lds_cap"] > 0


@pytest.mark.parametrize("na", NAS)
def test_few_digits(exe, orc, tmp_path, na):
    d = S.fewest_digits(na)
    assert d >= 2 and S.level1_fits(d, na) and not S.level1_fits(d - 1, na)
    if na != 4:
        return  # (the columns are built for the GPU tests' aggregate count alone)
    for dd, fits in ((d - 1, False), (d, True)):
        case = S.few_digits(dd, fits)
        plan = Plan(exe, case, na, tmp_path)
        check_common(case, plan, orc)
        assert plan.admit == 0
        dig0, l1why, hq = check_exact(case, plan)
        assert l1why == 0 and len(dig0) == dd  # (go_level1 itself accepts; level1_fits above — nut_groupby_layout's
        # table size for this many digits — is what makes go_plan_level1 decline dd = d - 1 and take dd = d)
