"""The values of every nut_ctx option (include/nutexec.h nut_option) that the suite checks
for parity: tests/test_gpu_option_sweep.py runs a workload that reads the option at every
value listed here and compares the result with the oracle, tests/test_option_sweep_cpu.py
holds this table to the sources (the ranges in csrc/api.hip, the defaults in
csrc/common.hpp, Executor.OPTIONS).  A new option without an entry here, or without a
workload there, fails the CPU suite.

Every list holds the option's lower bound, upper bound and default, every member of an
enumerated set, and interior values where the range is wide."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

SWEEP = {
    "gb_partition": [-1, 0, 1],
    "gb_levels": [0, 1, 2],
    "gb_optimistic": [0, 1],
    "gb_direct": [0, 1],
    "gb_chunks": [1, 4, 8, 64],
    "join_region": [0, 1],
    "join_probe_cfg": [0, 1, 2, 3, 4],
    "join_any_cfg": [0, 1, 2, 3, 4],
    "gb_seg_slots": [1, 2, 8],
    "gb_dense": [0, 1],
    "gb_l1_bits": [6, 7, 8],
    "topk": [0, 1],
    "gb_l0_bits": [0, 3, 6, 7, 8],   # (1..5 are accepted and mean 0: the default split)
    "stream_blocks": [0, 1, 3, 32],
    "priv_bd": [0, 128, 192, 256],
    "priv_blocks": [0, 1, 2, 3, 4, 16],
    "agg_blocks": [0, 1, 2, 16],
    "sel_blocks": [0, 1, 16],
    "sort_bd": [0, 512, 1024],
    "gb_ordered": [0, 1],
    "priv_probe": [0, 1],
    "gb_heavy": [0, 1, 2],
    "join_match": [0, 1],
    "gb_l1_threads": [512, 1024],
    "agg_slots": [2, 3, 4, 8],
    "gb_l1_spare": [0, 32, 128],
}

# values inside [lo, hi] that nut_ctx_set_option still refuses (not members of the set)
NOT_MEMBERS = {"priv_bd": [160], "sort_bd": [768], "gb_l1_threads": [768]}


def _array(text, pattern):
    m = re.search(pattern + r"\s*=\s*\{([^}]*)\}", text)
    assert m, pattern
    return [int(x) for x in m.group(1).split(",")]


def source_tables():
    """{option name: (lo, hi, default, members or None)} as the sources spell them: the enum
    of include/nutexec.h, lo[] / hi[] and the set checks of nut_ctx_set_option (csrc/api.hip),
    the defaults of nut_ctx::opt (csrc/common.hpp).  members: the values an enumerated option
    takes (`option == NUT_OPT_X && [value &&] value != a && value != b ...`; a leading
    `value &&` admits 0)."""
    header = (ROOT / "include" / "nutexec.h").read_text()
    common = (ROOT / "nutdb_amd" / "csrc" / "common.hpp").read_text()
    api = (ROOT / "nutdb_amd" / "csrc" / "api.hip").read_text()
    enum = {name.lower(): int(v) for name, v in re.findall(r"NUT_OPT_([A-Z0-9_]+) = (\d+)", header)}
    count = enum.pop("count")
    defaults = _array(common, r"int64_t opt\[NUT_OPT_COUNT\]")
    lo = _array(api, r"lo\[NUT_OPT_COUNT\]")
    hi = _array(api, r"hi\[NUT_OPT_COUNT\]")
    assert len(defaults) == len(lo) == len(hi) == count == len(enum)
    members = {}
    for name, cond in re.findall(r"if \(option == NUT_OPT_([A-Z0-9_]+) && ([^)]*)\)", api):
        vals = [int(v) for v in re.findall(r"value != (\d+)", cond)]
        assert vals, (name, cond)
        if re.match(r"value &&", cond):
            vals = [0] + vals
        members[name.lower()] = vals
    return {name: (lo[i], hi[i], defaults[i], members.get(name)) for name, i in enum.items()}
