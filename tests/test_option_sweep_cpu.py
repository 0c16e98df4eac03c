"""The option sweep's table (tests/option_sweep.py) against the sources, and the GPU sweep's
dispatcher against the table (CPU only: source text, the Python tables and an import of the
GPU module, which touches no device).  An option added to nut_option without sweep values
and a parity workload fails here."""
from option_sweep import NOT_MEMBERS, SWEEP, source_tables


def test_sweep_covers_every_option():
    from nutdb_amd.executor import Executor
    assert set(SWEEP) == set(Executor.OPTIONS)
    assert set(source_tables()) == set(Executor.OPTIONS)


def test_sweep_holds_bounds_default_and_members():
    for name, (lo, hi, default, members) in source_tables().items():
        vals = SWEEP[name]
        assert len(vals) == len(set(vals)), name
        assert {lo, hi, default} <= set(vals), (name, lo, hi, default, vals)
        assert all(lo <= v <= hi for v in vals), (name, vals)
        if members is not None:
            assert set(vals) == set(members), (name, members, vals)
            assert name in NOT_MEMBERS and all(lo < v < hi and v not in members for v in NOT_MEMBERS[name]), name
        elif hi - lo >= 8:  # a wide range: not the bounds alone
            assert any(lo < v < hi for v in vals), (name, vals)
    assert set(NOT_MEMBERS) == {n for n, t in source_tables().items() if t[3] is not None}


def test_enumerated_sets_parsed_from_source():
    """The parser really finds the three set checks of nut_ctx_set_option (a silent miss
    would turn the members check above into the plain range check)."""
    t = source_tables()
    assert t["priv_bd"][3] == [0, 128, 192, 256]
    assert t["sort_bd"][3] == [0, 512, 1024]
    assert t["gb_l1_threads"][3] == [512, 1024]


def test_gpu_dispatcher_has_a_workload_for_every_option():
    import test_gpu_option_sweep as g
    assert set(g.WORKLOADS) == set(SWEEP)
    assert all(callable(f) for f in g.WORKLOADS.values())
    assert sorted(g.CASES) == sorted((n, v) for n, vals in SWEEP.items() for v in vals)
