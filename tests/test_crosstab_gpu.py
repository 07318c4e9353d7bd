"""ChandyLamportSim.snapshot_crosstab / snapshot_crosstab_in (cl_snapshot_crosstab, cl_crosstab.hip)
against the oracle.

Expected values: crosstabcheck.expected over one OracleSim per instance (selectcheck.scenario's
cached runs); every word of the flat result must be equal exactly.  Scenarios, ranges and layouts
are those of the statistics, census and select tests: the library's choice of exec kernel (AUTO)
and the instance-per-lane kernel forced, instance-major records after flush() and block-major by
slot after rerun() of a mapped plan.
"""
import importlib

import numpy as np
import pytest

import oracle as O
from crosstabcheck import XT_CELLS, assert_crosstab_equal, expected, joint_sample
from isetcheck import clause_mask
from selectcheck import from_refs, scenario
from statscheck import RING_EVENTS, RING_TOP
from test_census_gpu import (AUTO, C3_EVENTS, C3_TOP, ENGINES, EVENTS3, HUB_EVENTS, HUB_TOP, TOP3, both_layouts,
                             flush_on, make_sim, replay_blocked)

cl = importlib.import_module("chandy-lamport-distributed-snapshot-algorithm_amd")
pytestmark = pytest.mark.gpu

N = 4096                        # the smallest batch that gets a mapped block-major replay
RANGES = [(0, N), (37, 3001)]
I64 = np.iinfo(np.int64)

# (sid, field, index, lo, width, bins)
T0 = (0, "tick", None, 0, 1, 64)
T4 = (4, "tick", None, 0, 1, 64)
C3_PAIRS = [
    (T0, T4),
    ((0, "tick", None, 26, 3, 4), T4),             # both clamps and a width above 1 on one axis
    (T0, (4, "tick", None, 26, 3, 4)),
    ((0, "node", 4, 0, 1, 8), (0, "ch_msgs", 0, 0, 1, 4)),
    ((0, "msgs", None, 0, 1, 8), (4, "inflight", None, 0, 2, 8)),
]


def check(sim, rows, keys, pairs, ranges, what, iset=None, mask=None):
    for a, b in pairs:
        for lo, hi in ranges:
            got = (sim.snapshot_crosstab(a, b, lo, hi) if iset is None
                   else sim.snapshot_crosstab_in(iset, a, b, lo, hi))
            assert_crosstab_equal(got.raw, expected(rows, keys, a, b, lo, hi, mask), f"{what} {a} x {b} [{lo}, {hi})")
            assert got.table.shape == (a[5], b[5]) and int(got.table.sum()) == got.sample


# ---- 1: C3, two snapshot ids, clamps, records and totals ------------------------------------------------
@ENGINES
def test_c3_ticks_of_two_snapshots_records_and_totals(engine):
    rows, keys = scenario(C3_TOP, C3_EVENTS, N)
    assert rows.n_sids == 5
    assert int((rows.status == O.FATAL_INSUFFICIENT_TOKENS).sum()) == 117      # the exclusion is exercised
    want = expected(rows, keys, T0, T4, 0, N)
    cells = want[XT_CELLS:]
    assert want[2] == 3979 and int((cells > 0).sum()) == 314 and int(cells.max()) == 48
    assert (want[8], want[10], want[9], want[11]) == (10, 40, 26, 43)             # tick ranges 10-40 and 26-43
    pick = joint_sample(rows, T0, T4, 0, N)
    assert round(float(np.corrcoef(rows.tick[0][pick], rows.tick[4][pick])[0, 1]), 3) == 0.158
    sim = make_sim(C3_TOP, C3_EVENTS, N, engine)
    both_layouts(sim, engine, lambda what: check(sim, rows, keys, C3_PAIRS, RANGES, what))
    got = sim.snapshot_crosstab(T0, T4)
    assert round(got.correlation(), 3) == 0.158
    assert got.min == (10, 26) and got.max == (40, 43)


# ---- 2: agreement with the existing calls, no oracle ------------------------------------------------------
@ENGINES
def test_agrees_with_statistics_and_selections(engine):
    sim = make_sim(C3_TOP, C3_EVENTS, N, engine)

    def body(what):
        for lo, hi in RANGES:
            xt = sim.snapshot_crosstab(T0, T4, lo, hi)
            st0 = sim.snapshot_stats(0, lo, hi, tick_lo=0, tick_bins=64)
            st4 = sim.snapshot_stats(4, lo, hi, tick_lo=0, tick_bins=64)
            assert st0.sample == st4.sample == xt.sample                       # the five snapshots share the sample
            assert (xt.instances, xt.ok) == (st0.instances, st0.ok)
            assert np.array_equal(xt.marginal(0), st0.tick_hist) and np.array_equal(xt.marginal(1), st4.tick_hist)
            assert xt.raw[cl.XT_SUM_A] == st0.tick_sum and xt.raw[cl.XT_SUM_B] == st4.tick_sum
            assert xt.raw[cl.XT_SUM_AA] == st0.tick_sumsq and xt.raw[cl.XT_SUM_BB] == st4.tick_sumsq
            assert xt.min == (st0.min_tick, st4.min_tick) and xt.max == (st0.max_tick, st4.max_tick)
            assert xt.mean(0) == st0.mean("tick") and xt.variance(1) == st4.variance("tick")
            # a cell is a selection of sid 4 inside a set made on sid 0
            ia, ib = (int(v) for v in np.unravel_index(int(np.argmax(xt.table)), xt.table.shape))
            for ca, cb in ((ia, ib), (ia, ib + 1), (10, 26)):
                iset = sim.instance_set(0, [("tick", None, ca, ca)])
                got = sim.select_instances_in(4, iset, [("tick", None, cb, cb)], lo, hi, max_out=0)
                assert got.n_match == xt.table[ca, cb], f"{what} cell ({ca}, {cb}) [{lo}, {hi})"
            # identical axes: a diagonal table whose diagonal is the histogram
            for axis, st in ((T0, st0), ((4, "tick", None, 26, 3, 4), None)):
                same = sim.snapshot_crosstab(axis, axis, lo, hi)
                diag = np.diagonal(same.table)
                assert np.array_equal(same.table, np.diag(diag)) and int(diag.sum()) == same.sample
                assert same.raw[cl.XT_SUM_AA] == same.raw[cl.XT_SUM_AB] == same.raw[cl.XT_SUM_BB]
                if st is not None:
                    assert np.array_equal(diag, st.tick_hist)
            rec = (0, "node", 4, 0, 1, 8)
            same = sim.snapshot_crosstab(rec, rec, lo, hi)
            assert np.array_equal(same.table, np.diag(np.diagonal(same.table)))
            assert same.raw[cl.XT_SUM_A] == sim.snapshot_stats(0, lo, hi).node_sum[4]

    both_layouts(sim, engine, body)


# ---- 3: the contended cell ----------------------------------------------------------------------------------
@ENGINES
def test_three_nodes_channel_tokens_against_tick(engine):
    rows, keys = scenario(TOP3, EVENTS3, N)
    assert (rows.status == O.OK).all() and rows.n_sids == 2
    a, b = (0, "ch_tok", 0, 0, 1, 16), (1, "tick", None, 0, 1, 64)
    want = expected(rows, keys, a, b, 0, N)
    cells = want[XT_CELLS:]
    assert want[2] == N and int((cells > 0).sum()) == 102 and int(cells.max()) == 166
    assert (want[9], want[11]) == (18, 27)
    sim = make_sim(TOP3, EVENTS3, N, engine)
    pairs = [(a, b), (b, a), ((0, "ch_tok", ("N1", "N2"), 3, 4, 3), (1, "inflight", None, 0, 1, 32))]
    oracle_pairs = [(a, b), (b, a), ((0, "ch_tok", 0, 3, 4, 3), (1, "inflight", None, 0, 1, 32))]

    def body(what):
        for given, plain in zip(pairs, oracle_pairs):
            for lo, hi in RANGES:
                got = sim.snapshot_crosstab(*given, lo, hi)
                assert_crosstab_equal(got.raw, expected(rows, keys, *plain, lo, hi), f"{what} {given} [{lo}, {hi})")

    both_layouts(sim, engine, body)


# ---- 4: record shapes ---------------------------------------------------------------------------------------
HUB_PAIRS = [
    ((1, "node", 0, 30, 1, 16), (3, "ch_msgs", 11, 0, 1, 4)),      # records of two snapshot ids
    ((0, "msgs", None, 0, 1, 8), (2, "node", 4, 0, 1, 8)),
    ((2, "ch_tok", 3, 0, 1, 4), (2, "tick", None, 0, 1, 32)),
    ((3, "inflight", None, 0, 1, 16), (3, "msgs", None, 0, 1, 16)),
]


def test_hub_three_word_records_instance_major():
    n = 512
    rows, keys = scenario(HUB_TOP, HUB_EVENTS, N)   # (instance i is seeded by i alone)
    assert (rows.status == O.OK).all() and rows.n_sids == 4
    sim = make_sim(HUB_TOP, HUB_EVENTS, n, AUTO)
    assert sim.num_nodes * 3 == 33                  # 33 record words: not staged in LDS
    sim.flush()
    assert not sim.records_blocked()
    check(sim, rows, keys, HUB_PAIRS, [(0, n), (5, 300)], "hub after flush")


def test_hub_three_word_records_block_major():
    rows, keys = scenario(HUB_TOP, HUB_EVENTS, N)
    sim = make_sim(HUB_TOP, HUB_EVENTS, N, AUTO)
    sim.flush()
    replay_blocked(sim)
    check(sim, rows, keys, HUB_PAIRS, RANGES, "hub after rerun")


def test_ring_two_word_records_both_layouts():
    rows, keys = scenario(RING_TOP, RING_EVENTS, N)
    assert rows.n_sids == 2 and int((rows.status == O.FATAL_INSUFFICIENT_TOKENS).sum()) == 1679
    sim = make_sim(RING_TOP, RING_EVENTS, N, AUTO)
    assert sim.num_nodes == 5 and sim.num_channels == 5     # rw = 2: staged with scalar loads
    pairs = [
        ((0, "node", 2, 0, 1, 8), (1, "ch_tok", 1, 0, 1, 8)),       # records of two snapshot ids
        ((1, "msgs", None, 0, 1, 8), (0, "inflight", None, 1, 2, 4)),
        ((0, "ch_msgs", 1, 0, 1, 4), (0, "node", 3, 2, 2, 4)),      # one staging serves both axes
        ((1, "tick", None, 8, 1, 16), (0, "ch_tok", 2, 0, 1, 4)),
    ]
    both_layouts(sim, AUTO, lambda what: check(sim, rows, keys, pairs, RANGES, "ring " + what))


# ---- 5: the joint sample is the intersection of the two snapshots' samples ------------------------------
@ENGINES
def test_different_samples_per_axis(engine):
    n = 256
    refs = []
    for i in range(n):
        r = O.OracleSim()
        r.seed_go(O.REFERENCE_SEED + i)
        assert r.read_topology_text(TOP3) == 0
        assert r.send_tokens("N1", "N2", 1) == 0 and r.send_tokens("N2", "N3", 2) == 0
        assert r.start_snapshot("N1") == (0, 0)
        r.tick()
        assert r.start_snapshot("N3") == (0, 1)
        for _ in range(7):
            r.tick()
        refs.append(r)
    rows, keys = from_refs(refs)
    assert (rows.status == O.OK).all()
    assert (int(rows.done[0].sum()), int(rows.done[1].sum()), int((rows.done[0] & rows.done[1]).sum())) == (86, 61, 20)
    sim = make_sim(TOP3, None, n, engine)
    sim.ProcessEvent(cl.PassTokenEvent("N1", "N2", 1))
    sim.ProcessEvent(cl.PassTokenEvent("N2", "N3", 2))
    assert sim.StartSnapshot("N1") == 0
    sim.Tick(1)
    assert sim.StartSnapshot("N3") == 1
    sim.Tick(7)
    a, b = (0, "tick", None, 0, 1, 16), (1, "node", 1, 24, 1, 16)
    got = sim.snapshot_crosstab(a, b)            # executes the pending events, adds no tick
    assert (got.instances, got.ok, got.sample) == (n, n, 20)
    assert sim.snapshot_crosstab(b, a).sample == 20
    assert np.array_equal(sim.snapshot_crosstab(b, a).table, got.table.T)
    pairs = [(a, b), (b, a), ((1, "tick", None, 0, 1, 16), (0, "msgs", None, 0, 1, 4)),
             ((0, "ch_tok", 0, 0, 1, 4), (1, "ch_tok", 2, 0, 1, 4))]
    check(sim, rows, keys, pairs, [(0, n), (3, 201)], "mid-program")
    assert sim.snapshot_stats(0).sample == 86 and sim.snapshot_stats(1).sample == 61


# ---- 6: the conditional form ------------------------------------------------------------------------------
def test_conditional_crosstab_against_the_oracle():
    rows, keys = scenario(C3_TOP, C3_EVENTS, N)
    sim = make_sim(C3_TOP, C3_EVENTS, N, AUTO)
    late_w, busy_w = [("tick", None, 22, None)], [("msgs", None, 2, None)]
    late_m, busy_m = clause_mask(rows, keys, 0, late_w), clause_mask(rows, keys, 1, busy_w)
    assert (late_m & busy_m).any() and (late_m & ~busy_m).any()
    late, busy = sim.instance_set(0, late_w), sim.instance_set(1, busy_w)
    sets = [("late & busy", late & busy, late_m & busy_m), ("late - busy", late - busy, late_m & ~busy_m)]
    whole = sim.instance_set_from(np.arange(N))
    pairs = [C3_PAIRS[0], C3_PAIRS[3], ((3, "ch_tok", 2, 0, 1, 8), (0, "tick", None, 0, 2, 32))]

    def body(what):
        for name, iset, mask in sets:
            assert len(iset) == int(mask.sum())
            check(sim, rows, keys, pairs, RANGES, f"{what} {name}", iset=iset, mask=mask)
            got = sim.snapshot_crosstab_in(iset, T0, T4)
            assert (got.instances, got.ok) == (N, 3979)                       # the range's
        for a, b in pairs:                                                     # the whole batch as the set
            for lo, hi in RANGES:
                assert (sim.snapshot_crosstab_in(whole, a, b, lo, hi).raw.tobytes()
                        == sim.snapshot_crosstab(a, b, lo, hi).raw.tobytes()), f"{what} {a} x {b} [{lo}, {hi})"

    both_layouts(sim, AUTO, body)
    other = make_sim(C3_TOP, C3_EVENTS, 64, AUTO)
    other.flush()
    foreign = other.instance_set_from([1, 2, 3])
    with pytest.raises(cl.ClSnapError) as e:
        sim.snapshot_crosstab_in(foreign, T0, T4)
    assert e.value.code == cl.E_INVALID


# ---- 7: ranges and plumbing ---------------------------------------------------------------------------------
@ENGINES
def test_ranges_merge_timing_and_device_bytes(engine):
    rows, keys = scenario(C3_TOP, C3_EVENTS, N)
    sim = make_sim(C3_TOP, C3_EVENTS, N, engine)
    pairs = [C3_PAIRS[0], C3_PAIRS[3]]
    ranges = [(17, 17), (N, N), (0, 0), (63, 65), (64, 128), (N - 1, N), (0, 1000), (1000, N)]

    def body(what):
        before = sim.device_bytes
        for lo in (17, N):
            empty = sim.snapshot_crosstab(T0, T4, lo, lo)
            assert (empty.instances, empty.ok, empty.sample) == (0, 0, 0) and not empty.table.any()
            assert empty.min == (I64.max, I64.max) and empty.max == (I64.min, I64.min)
            assert not empty.raw[3:8].any()
        assert sim.device_bytes > before or what != "instance-major"         # the scratch is counted
        check(sim, rows, keys, pairs, ranges, what)
        for a, b in pairs:                                                    # sub-ranges merge into the whole
            parts = sim.snapshot_crosstab(a, b, 0, 1000).merge(sim.snapshot_crosstab(a, b, 1000, N))
            assert parts == sim.snapshot_crosstab(a, b)
        assert sim.crosstab_time() > 0

    both_layouts(sim, engine, body)


@ENGINES
def test_empty_sample(engine):
    n = 64
    rows, keys = scenario("3nodes.top", EVENTS3, n)
    assert (rows.status == O.FATAL_INSUFFICIENT_TOKENS).all()   # N3 starts with 0 tokens
    sim = make_sim("3nodes.top", EVENTS3, n, engine)
    flush_on(sim, engine)
    for a, b in (((0, "tick", None, 0, 1, 8), (1, "tick", None, 0, 1, 8)),
                 ((0, "node", 1, 0, 1, 8), (1, "inflight", None, 0, 1, 8))):
        got = sim.snapshot_crosstab(a, b)
        assert_crosstab_equal(got.raw, expected(rows, keys, a, b, 0, n), "all fatal")
        assert (got.instances, got.ok, got.sample) == (n, 0, 0) and not got.table.any()
        assert got.min == (I64.max, I64.max) and got.max == (I64.min, I64.min)


# ---- 8: ragged batch sizes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_ragged_batch_sizes(n):
    rows, keys = scenario(TOP3, EVENTS3, N)   # (instance i is seeded by i alone)
    sim = make_sim(TOP3, EVENTS3, n, AUTO)
    flush_on(sim, AUTO)
    pairs = [((0, "ch_tok", 0, 0, 1, 16), (1, "tick", None, 0, 1, 64)),
             ((1, "node", 2, 20, 2, 8), (0, "msgs", None, 0, 3, 8))]
    check(sim, rows, keys, pairs, [(0, n), (n // 2, n), (0, n // 2)], f"n = {n}")
    whole = sim.instance_set_from(np.arange(n))
    for a, b in pairs:
        assert sim.snapshot_crosstab_in(whole, a, b).raw.tobytes() == sim.snapshot_crosstab(a, b).raw.tobytes()
