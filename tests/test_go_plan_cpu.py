"""CPU: the ordered group-by's host plan (csrc/go_plan.hpp) without a GPU — the
key range, the admission test, the heavy keys and their cuckoo table, the buffer sizes, both
levels' regions in their capped and exact forms, the chunks with their tile tables and the heavy
keys' partitions.  The header is built with g++ into a stand-alone program
(tests/c/test_go_plan.cpp), plain and sanitized; every check is an invariant the kernels rely on
or a value that follows from the plan's stated rules, restated here in Python."""
import math
import random
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
M64 = 2**64 - 1
I64_MIN, I64_MAX = -2**63, 2**63 - 1
GP_TILE, GP_ITEMS, CELLS, SAMPLE = 8192, 16, 1 << 14, 65536
HK_MAX, HK_WORDS, HK_SLOTS = 2048, 2048, 8192
SHAPE, CLUSTERED, CAPACITY = 1, 2, 4  # nutexec.h NUT_GB_DECLINE_*


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]],
                ids=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("go_plan") / "test_go_plan"
    subprocess.run(["g++", *request.param, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "nutdb_amd" / "csrc"),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "c" / "test_go_plan.cpp"), "-o", str(out)], check=True)
    return out


def run(exe, lines):
    """-> the output lines as (name, [numbers]), in order"""
    r = subprocess.run([str(exe)], input="".join(x + "\n" for x in lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = []
    for ln in r.stdout.splitlines():
        w = ln.split()
        out.append((w[0], [float(x) if "." in x or "e" in x else int(x) for x in w[1:]]))
    return out


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def signed(u):
    return u - 2**64 if u >> 63 else u


def biased(k):
    """a signed key as the unsigned word whose order is the keys' order"""
    return (k & M64) ^ (1 << 63)


# ---------------------------------------------------------------- range
def want_range(smin, smax):
    """the rule: 1/1024 of the sampled span on either side, saturating at 0 and ~0; a span (after
    the margin) below 2^16 declines; t shifts the span below 2^32; mul = floor(2^46 / ((span >> t) + 1))"""
    lo, hi = biased(smin), biased(smax)
    margin = (hi - lo) >> 10
    lo = lo - margin if lo > margin else 0
    hi = hi + margin if hi < M64 - margin else M64
    span = hi - lo
    if span < 2**16:
        return None
    t = span.bit_length() - 32 if span >> 32 else 0
    return lo, span, t, (1 << 46) // ((span >> t) + 1)


# (0, 2^16 - 1): its own span is below 2^16, but the check is on the span with the margin
# (65535 + 2 * 63 = 65661), so the plan ACCEPTS it; (0, 65000) widens to 65126 and declines.
RANGES = [(0, 2**16 - 1), (0, 2**20), (-2**40, 2**40), (I64_MIN, I64_MAX), (I64_MAX - 2**20, I64_MAX),
          (I64_MIN, I64_MIN + 2**20), (0, 65000)]


@pytest.mark.parametrize("smin,smax", RANGES)
def test_range(exe, smin, smax):
    want = want_range(smin, smax)
    assert (want is None) == ((smin, smax) == (0, 65000))
    rnd = random.Random(smin ^ smax)
    keys = [rnd.randint(smin, smax) for _ in range(60000)] + [rnd.randint(I64_MIN, I64_MAX) for _ in range(20000)] + \
           [min(I64_MAX, max(I64_MIN, smin + rnd.randint(-2**21, 2**21))) for _ in range(10000)] + \
           [min(I64_MAX, max(I64_MIN, smax + rnd.randint(-2**21, 2**21))) for _ in range(10000)]
    keys.sort()
    out = run(exe, [f"range {smin} {smax}", "cell 4"] + ["0"] * 4)
    why, lo, span, t, mul = out[0][1]
    if want is None:
        assert why == SHAPE
        return
    assert why == 0 and (lo, span, t, mul) == want
    assert span >> t < 2**32 and mul < 2**32
    assert lo <= biased(smin) and biased(smax) <= lo + span
    ends = [signed(lo ^ (1 << 63)), signed((lo + span) ^ (1 << 63)), I64_MIN, I64_MAX]
    out = run(exe, [f"range {smin} {smax}", f"cell {len(ends)}"] + [str(k) for k in ends] +
              [f"cell {len(keys)}"] + [str(k) for k in keys])
    ec, kc = out[1][1][1:], out[2][1][1:]
    assert all(0 <= c < CELLS for c in ec + kc)
    assert ec[0] == ec[2] == 0 and max(kc) <= ec[1] == ec[3]  # outside keys clamp to the end cells
    assert kc == sorted(kc) and len(kc) == len(keys)
    assert len(set(kc)) > CELLS // 2  # (the cells are used: the range is not degenerate)


# ---------------------------------------------------------------- admission
def sample_lines(pairs):
    assert sum(m for _, m in pairs) == SAMPLE
    return [f"sample {len(pairs)}"] + [f"{k} {m}" for k, m in pairs]


@pytest.mark.parametrize("bits0", [6, 7, 8])
def test_admission(exe, bits0):
    rng = f"range 0 {65535 << 20}"
    even = run(exe, [rng] + sample_lines([(i << 20, 1) for i in range(SAMPLE)]) + [f"admit {bits0}"])
    packed = run(exe, [rng] + sample_lines([(i << 12, 1) for i in range(SAMPLE)]) + [f"admit {bits0}"])
    repeat = run(exe, [rng] + sample_lines([(12345 << 20, SAMPLE)]) + [f"admit {bits0}"])
    assert even[-1] == ("admit", [0])
    assert packed[-1] == ("admit", [CLUSTERED])
    assert repeat[-1] == ("admit", [0])


# ---------------------------------------------------------------- heavy keys
def key_of(i):
    return signed(mix64(i + 1))


def heavy_sample(groups):
    """[(keys, multiplicity)] + single keys up to the sample's size"""
    pairs, i = [], 0
    for count, mult in groups:
        pairs += [(key_of(i + j), mult) for j in range(count)]
        i += count
    rest = SAMPLE - sum(m for _, m in pairs)
    return pairs + [(key_of(i + j), 1) for j in range(rest)]


def run_heavy(exe, pairs, na):
    out = run(exe, sample_lines(pairs) + [f"heavy {na}"])
    _, nh, seed1, seed2 = out[1][1]
    rows = [w for name, w in out[2:] if name == "hk"]
    assert len(rows) == nh
    return nh, seed1, seed2, rows


def want_heavy(pairs, na):
    cand = sorted(((m, k) for k, m in pairs if m >= 3), key=lambda x: (-x[0], x[1]))[:min(HK_MAX, HK_WORDS // na)]
    return sorted(k for _, k in cand) if sum(m for m, _ in cand) * 20 >= SAMPLE else []


@pytest.mark.parametrize("groups,na,nwant", [
    ([(2000, 3), (1000, 2)], 1, 2000),   # keys seen twice are never chosen
    ([(1000, 3), (5000, 2)], 1, 0),      # 3000 < 5 % of 65536
    ([(1093, 3)], 1, 1093),              # 3279 >= 3276.8: the smallest cover that is kept
    ([(1092, 3)], 1, 0),                 # 3276 < 3276.8
    ([(1500, 8), (1500, 3)], 1, 2048),   # cut to HK_MAX: every 8, then the 548 smallest keys of the 3s
    ([(1500, 8), (1500, 3)], 4, 512),    # cut to HK_WORDS / na
], ids=["twice", "below5", "at5", "under5", "cut1", "cut4"])
def test_heavy_keys(exe, groups, na, nwant):
    pairs = heavy_sample(groups)
    nh, seed1, seed2, rows = run_heavy(exe, pairs, na)
    want = want_heavy(pairs, na)
    assert len(want) == nwant and nh == nwant
    assert [r[0] for r in rows] == want  # ascending
    if not nh:
        return
    seeds = [(mix64((0x9E3779B97F4A7C15 + 2 * a) & M64), mix64((0x9E3779B97F4A7C15 + 2 * a + 1) & M64)) for a in range(8)]
    assert (seed1, seed2) in seeds
    for j, (k, a, sa, b, sb) in enumerate(rows):
        assert a == (mix64((k & M64) ^ seed1) >> 32) & (HK_SLOTS - 1)
        assert b == (mix64((k & M64) ^ seed2) >> 32) & (HK_SLOTS - 1)
        found = {s for s, v in ((a, sa), (b, sb)) if v == j + 1}
        assert len(found) == 1, (j, k, a, sa, b, sb)  # in exactly one of its two slots


# ---------------------------------------------------------------- sizes and level 0
NS = [2**24, 2**24 + 4099, 10**9]
LAM = 1e7 / CELLS
MODES = {"capped": (0, 0), "heavy_capped": (1, 1), "exact": (1, 0)}  # (heavy keys, NUT_OPT_GB_HEAVY = 2)


_SIZES = {}


def sizes(exe, n, bits0, mode, nstore=2):
    """go_sizes' fields (one run per build and case, shared by the tests that lay regions out in them)"""
    key = (exe, n, bits0, mode, nstore)
    if key not in _SIZES:
        heavy, keep = MODES[mode]
        w = run(exe, [f"sizes {n} {bits0} {nstore} {LAM!r} {heavy} {keep}"])[0][1]
        _SIZES[key] = dict(zip(("why", "exact", "slack1", "rows", "arena1", "b2rows", "ocap", "abase0", "acap0",
                                "data_bytes"), w))
    return _SIZES[key]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("bits0", [6, 7, 8])
@pytest.mark.parametrize("n", NS)
def test_sizes(exe, n, bits0, mode):
    z = sizes(exe, n, bits0, mode)
    assert z["exact"] == (mode == "exact")
    assert z["slack1"] == {"capped": 1.0 + 6.0 / math.sqrt(LAM), "heavy_capped": 2.5, "exact": 1.0}[mode]
    assert z["rows"] % 32 == 0 and z["b2rows"] % 32 == 0 and z["arena1"] % 32 == 0
    assert n + 2 * 65536 + 64 <= z["rows"] < n + 2 * 65536 + 64 + 32
    share = {"capped": n // 2, "heavy_capped": n // 4, "exact": 0}[mode]
    assert share <= z["arena1"] < share + 32
    regions = math.ceil(n * z["slack1"]) + 66 * CELLS
    assert regions + z["arena1"] + 2 * GP_TILE + 64 <= z["b2rows"] < regions + z["arena1"] + 2 * GP_TILE + 64 + 32
    assert z["ocap"] % 2 == 0 and z["abase0"] == z["ocap"] << bits0 and z["abase0"] % 2 == 0
    assert (z["ocap"] + 2) << bits0 > 3 * z["rows"] // 2 >= z["abase0"]  # 1.5 x the even share
    assert z["abase0"] + z["acap0"] + 2 * GP_TILE == 2 * z["rows"]
    assert z["data_bytes"] == (2 * 2 * z["rows"] + 2 * z["b2rows"]) * 8 + 256


def parse_l0(out):
    d = {name: w for name, w in out}
    d["why"] = d["l0"][0]
    d["segs"] = [tuple(d["segs"][i:i + 5]) for i in range(0, len(d["segs"]), 5)]  # (start, count, tile0, obase, ocap)
    return d


def hcount_lines(n0, hchunk, k=5):
    """k workgroups' kept rows (one of them none), n0 in all"""
    per = [min(hchunk, n0 // (k - 1) + 1)] * (k - 1)
    per[-1] = n0 - sum(per[:-1])
    assert 0 < per[-1] <= hchunk
    per.insert(2, 0)
    return [f"hcount {len(per)} {hchunk}"] + [str(x) for x in per], per


@pytest.mark.parametrize("heavy", [0, 1])
@pytest.mark.parametrize("bits0", [6, 7, 8])
@pytest.mark.parametrize("n", NS)
def test_level0_capped(exe, n, bits0, heavy):
    z = sizes(exe, n, bits0, "heavy_capped" if heavy else "capped")
    nb0, ocap = 1 << bits0, z["ocap"]
    hchunk = (n // 4 + 2047) // 2048 * 2048
    hl, per = hcount_lines(n - n // 3, hchunk) if heavy else (["hcount 0 0"], [])
    # the cursors the scatter would hand back: every third digit empty, the others part full
    p0 = [(d * ocap, d * ocap + 1 + (d * 7919) % ocap) for d in range(nb0) if d % 3 != 1]
    d = parse_l0(run(exe, hl + [f"l0 0 {n} {bits0} {z['rows']} {ocap} {len(p0)}"] + [f"{a} {b}" for a, b in p0])[1:])
    assert d["why"] == 0 and d["dig0"] == [x for x in range(nb0) if x % 3 != 1]
    if heavy:
        assert d["segs"] == [(b * hchunk, c, 0, 0, ocap) for b, c in enumerate(per) if c]
    else:
        assert d["segs"] == [(0, n, 0, 0, ocap)]
    assert all(a % 2 == 0 for a, _ in p0) and (nb0 - 1) * ocap + ocap <= z["abase0"]


def cell_counts(kind, n0):
    if kind == "one":
        return {9999: n0}
    c = {q: n0 // CELLS for q in range(CELLS)}
    if kind == "half":
        c = {q: (n0 - n0 // 2) // CELLS for q in range(CELLS)}
        c[4321] += n0 // 2
    c[0] += n0 - sum(c.values())
    return c


def counts_lines(c):
    return [f"counts {len(c)}"] + [f"{q} {r}" for q, r in c.items()]


@pytest.mark.parametrize("kind", ["one", "uniform", "half"])
@pytest.mark.parametrize("bits0", [6, 7, 8])
@pytest.mark.parametrize("n", NS)
def test_level0_exact(exe, n, bits0, kind):
    z = sizes(exe, n, bits0, "exact")
    bits1, nb0 = 14 - bits0, 1 << bits0
    n0 = n - n // 3
    c = cell_counts(kind, n0)
    hchunk = (n // 4 + 2047) // 2048 * 2048
    hl, per = hcount_lines(n0, hchunk)
    out = run(exe, hl + counts_lines(c) + [f"l0 1 {n} {bits0} {z['rows']} {z['ocap']}"])
    assert out[1] == ("counts", [0, n0])
    d = parse_l0(out[2:])
    assert d["why"] == 0
    dsum = [sum(c.get((dg << bits1) | q, 0) for q in range(1 << bits1)) for dg in range(nb0)]
    cur0 = d["cur0"]
    assert len(cur0) == nb0 + 1 and cur0[nb0] == 0  # + the overflow flag
    assert all(x % 32 == 0 for x in cur0[:nb0])
    assert all(cur0[dg] + dsum[dg] <= cur0[dg + 1] for dg in range(nb0 - 1))  # non-overlapping
    assert cur0[nb0 - 1] + dsum[nb0 - 1] + 2 * GP_TILE <= 2 * z["rows"]
    assert d["dig0"] == [dg for dg in range(nb0) if dsum[dg]]
    assert d["p0"] == [x for dg in d["dig0"] for x in (cur0[dg], cur0[dg] + dsum[dg])]
    # the scatter's input: the heavy pass's runs, no capped regions, one tile entry per 16 Ki rows
    assert d["segs"] == [(b * hchunk, cnt, t0, 0, 0) for (b, cnt), t0 in
                         zip([(b, cnt) for b, cnt in enumerate(per) if cnt],
                             [sum(-(-x // (2 * GP_TILE)) for x in [y for y in per if y][:i]) for i in range(4)])]
    assert d["ts0"] == [i for i, cnt in enumerate(y for y in per if y) for _ in range(-(-cnt // (2 * GP_TILE)))]


@pytest.mark.parametrize("bits0", [6, 7, 8])
def test_level0_exact_does_not_fit(exe, bits0):
    n = NS[1]
    z = sizes(exe, n, bits0, "exact")
    c = {q: 2 * z["rows"] // CELLS + 1 for q in range(CELLS)}  # more rows than O holds
    d = parse_l0(run(exe, ["hcount 1 4096 4096"] + counts_lines(c) + [f"l0 1 {n} {bits0} {z['rows']} {z['ocap']}"])[2:])
    assert d["why"] == CAPACITY
    fits = {q: (2 * z["rows"] - 2 * GP_TILE) // CELLS - 32 for q in range(CELLS)}  # just inside, padding included
    d = parse_l0(run(exe, ["hcount 1 4096 4096"] + counts_lines(fits) + [f"l0 1 {n} {bits0} {z['rows']} {z['ocap']}"])[2:])
    assert d["why"] == 0


# ---------------------------------------------------------------- level 1
def parse_l1(out):
    d = {name: w for name, w in out}
    d["why"], d["ovf1"], d["acap1"], d["nparts"] = d["l1"]
    d["s2"] = [tuple(d["s2"][i:i + 5]) for i in range(0, len(d["s2"]), 5)]
    return d


def want_cb(np0):
    cb = [0]
    for f in (6, 10, 13, 14, 15, 16):
        if np0 * f // 16 > cb[-1]:
            cb.append(np0 * f // 16)
    return cb


def check_chunks(d, np0, nb1, tile):
    cb = d["cb"]
    assert cb == want_cb(np0) and cb[-1] == np0
    nch = len(cb) - 1
    assert len(d["tile0"]) == nch + 1 and len(d["ntile"]) == nch and len(d["init"]) == d["nparts"] + nch
    assert d["init"][d["nparts"]:] == [0] * nch  # one overflow flag per chunk
    assert sum(d["ntile"]) == len(d["tiles"])
    for j in range(nch):
        ts = d["tiles"][d["tile0"][j]:d["tile0"][j] + d["ntile"][j]]
        segs = d["s2"][cb[j]:cb[j + 1]]
        # the chunk's table names its own segments alone (indices from the chunk's first), each
        # over ceil(count / tile) tiles, from the segment's tile0 on
        assert ts == [i for i, s in enumerate(segs) for _ in range(-(-s[1] // tile))]
        at = 0
        for s in segs:
            assert s[2] == at
            at += -(-s[1] // tile)
    assert d["nparts"] == np0 * nb1


def disjoint_even(init, rend):
    assert all(a % 2 == 0 and a <= b for a, b in zip(init, rend))
    order = sorted(zip(init, rend))
    assert all(order[i][1] <= order[i + 1][0] for i in range(len(order) - 1))


@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("heavy", [0, 1])
@pytest.mark.parametrize("bits0", [6, 7, 8])
@pytest.mark.parametrize("n", NS)
def test_level1_capped(exe, n, bits0, heavy, threads):
    z = sizes(exe, n, bits0, "heavy_capped" if heavy else "capped")
    nb0, nb1, ocap = 1 << bits0, 1 << (14 - bits0), z["ocap"]
    share = n // nb0
    digs = [dg for dg in range(nb0) if dg % 5 != 2]
    p0 = [(dg * ocap, dg * ocap + min(ocap, share // 2 + (dg * 104729) % share)) for dg in digs]
    assert sum(b - a for a, b in p0) <= n
    # the regions' end by the rule: per level-0 partition 2^bits1 regions of its even share x slack1 + 64
    # rows, an even count; one row less than ovf1 + 2 tiles in B2 declines, and so does no partition at all
    ovf1 = sum(((math.ceil((b - a) / nb1 * z["slack1"]) + 64 + 1) & ~1) << (14 - bits0) for a, b in p0)
    short = ovf1 + 2 * GP_TILE - 1
    l0_lines = ["hcount 0 0", f"l0 0 {n} {bits0} {z['rows']} {ocap} {len(p0)}"] + [f"{a} {b}" for a, b in p0]
    l1 = f"l1 0 {bits0} {z['slack1']!r} "
    out = run(exe, l0_lines + [l1 + f"{z['b2rows']} {threads}", l1 + f"{short} {threads}", l1 + f"{short + 1} {threads}",
                               f"l0 0 {n} {bits0} {z['rows']} {ocap} 0", l1 + f"{z['b2rows']} {threads}"])
    d = parse_l1(out[7:16])
    assert d["why"] == 0 and d["ovf1"] == ovf1
    assert parse_l1(out[16:25])["why"] == CAPACITY and parse_l1(out[25:34])["why"] == 0
    assert parse_l0(out[34:40])["dig0"] == [] and parse_l1(out[40:])["why"] == CAPACITY
    check_chunks(d, len(digs), nb1, threads * GP_ITEMS)
    init, rend = d["init"][:d["nparts"]], d["rend"]
    disjoint_even(init, rend)
    assert max(rend) <= d["ovf1"] and d["ovf1"] + d["acap1"] + 2 * GP_TILE == z["b2rows"]
    for i, (a, b) in enumerate(p0):
        start, count, _, obase, cap1 = d["s2"][i]
        assert (start, count) == (a, b - a) and obase % 2 == 0 and cap1 % 2 == 0
        # the even share x slack1 + 64 rows, rounded up to an even count
        assert math.ceil(count / nb1 * z["slack1"]) + 64 <= cap1 <= math.ceil(count / nb1 * z["slack1"]) + 65
        assert init[i * nb1:(i + 1) * nb1] == [obase + q * cap1 for q in range(nb1)]
        assert rend[i * nb1:(i + 1) * nb1] == [obase + (q + 1) * cap1 for q in range(nb1)]


@pytest.mark.parametrize("kind", ["one", "uniform", "half"])
@pytest.mark.parametrize("bits0", [6, 7, 8])
@pytest.mark.parametrize("n", NS)
def test_level1_exact(exe, n, bits0, kind):
    z = sizes(exe, n, bits0, "exact")
    bits1 = 14 - bits0
    nb1 = 1 << bits1
    n0 = n - n // 3
    c = cell_counts(kind, n0)
    hl, _ = hcount_lines(n0, (n // 4 + 2047) // 2048 * 2048)
    out = run(exe, hl + counts_lines(c) + [f"l0 1 {n} {bits0} {z['rows']} {z['ocap']}",
                                          f"l1 1 {bits0} {z['slack1']!r} {z['b2rows']} 1024"])
    l0, d = parse_l0(out[2:8]), parse_l1(out[8:])
    assert l0["why"] == 0 and d["why"] == 0
    check_chunks(d, len(l0["dig0"]), nb1, 1024 * GP_ITEMS)
    init, rend = d["init"][:d["nparts"]], d["rend"]
    disjoint_even(init, rend)
    for i, dg in enumerate(l0["dig0"]):
        assert [b - a for a, b in zip(init[i * nb1:(i + 1) * nb1], rend[i * nb1:(i + 1) * nb1])] == \
               [c.get((dg << bits1) | q, 0) for q in range(nb1)]
        assert d["s2"][i][:2] == (l0["p0"][2 * i], l0["p0"][2 * i + 1] - l0["p0"][2 * i]) and d["s2"][i][3] == init[i * nb1]
    assert max(rend) <= d["ovf1"] and d["ovf1"] + d["acap1"] + 2 * GP_TILE == z["b2rows"]


@pytest.mark.parametrize("np0,want", [(128, [0, 48, 80, 104, 112, 120, 128]), (16, [0, 6, 10, 13, 14, 15, 16]),
                                      (2, [0, 1, 2]), (1, [0, 1])])
def test_chunk_boundaries(exe, np0, want):
    n, bits0 = NS[1], 7
    z = sizes(exe, n, bits0, "capped")
    ocap = z["ocap"]
    digs = [dg * (128 // np0) + (128 // np0) // 2 for dg in range(np0)]  # np0 of the 128 digits hold rows
    p0 = [(dg * ocap, dg * ocap + n // 256) for dg in digs]
    d = parse_l1(run(exe, ["hcount 0 0", f"l0 0 {n} {bits0} {z['rows']} {ocap} {np0}"] + [f"{a} {b}" for a, b in p0] +
                     [f"l1 0 {bits0} {z['slack1']!r} {z['b2rows']} 1024"])[7:])
    assert d["why"] == 0 and d["cb"] == want and want_cb(np0) == want
    check_chunks(d, np0, 128, 1024 * GP_ITEMS)


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("bits0", [6, 7, 8])
def test_heavy_key_partitions(exe, bits0, exact):
    n = NS[1]
    z = sizes(exe, n, bits0, "exact" if exact else "heavy_capped")
    bits1 = 14 - bits0
    nb0, nb1, ocap = 1 << bits0, 1 << bits1, z["ocap"]
    smin, smax = -2**40, 2**40
    rnd = random.Random(bits0)
    hkeys = sorted({rnd.randint(smin, smax) for _ in range(600)} | {smin, smax, I64_MIN, I64_MAX})
    digs = [dg for dg in range(nb0) if dg % 4 != 1]  # a quarter of the level-0 partitions hold no rows
    head = [f"range {smin} {smax}", f"hkeys {len(hkeys)}"] + [str(k) for k in hkeys] + \
           [f"cell {len(hkeys)}"] + [str(k) for k in hkeys]
    if exact:
        c = {(dg << bits1) | q: 40 + (dg * nb1 + q) % 13 for dg in digs for q in range(nb1)}
        out = run(exe, head + ["hcount 1 8192 1"] + counts_lines(c) + [f"l0 1 {n} {bits0} {z['rows']} {ocap}",
                                                                      f"l1 1 {bits0} 1.0 {z['b2rows']} 1024"])
        cells, l0, d = out[2][1][1:], parse_l0(out[5:11]), parse_l1(out[11:])
    else:
        p0 = [(dg * ocap, dg * ocap + 1000) for dg in digs]
        out = run(exe, head + ["hcount 0 0", f"l0 0 {n} {bits0} {z['rows']} {ocap} {len(p0)}"] + [f"{a} {b}" for a, b in p0] +
                  [f"l1 0 {bits0} 2.5 {z['b2rows']} 1024"])
        cells, l0, d = out[2][1][1:], parse_l0(out[4:10]), parse_l1(out[10:])
    assert l0["why"] == 0 and d["why"] == 0 and l0["dig0"] == digs and len(d["hq"]) == len(hkeys)
    assert cells == sorted(cells) and cells[0] == 0 and len({x >> bits1 for x in cells} - set(digs)) > 0
    for cell, q in zip(cells, d["hq"]):
        if cell >> bits1 not in digs:
            assert q == -1
            continue
        i = digs.index(cell >> bits1)
        assert q == i * nb1 + (cell & (nb1 - 1))
        # the partition's region is the one the scatter sends the key's cell to: the level-1 digit's
        # region of the segment of the key's level-0 digit
        if exact:
            assert d["init"][q] == d["s2"][i][3] + sum((c[(digs[i] << bits1) | x] + 1) & ~1 for x in range(cell & (nb1 - 1)))
        else:
            assert d["init"][q] == d["s2"][i][3] + (cell & (nb1 - 1)) * d["s2"][i][4]
