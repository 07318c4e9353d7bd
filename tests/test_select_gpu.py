"""ChandyLamportSim.select_instances (cl_select_instances, cl_select.hip) and snapshot_ticks against
the oracle.

Expected values: selectcheck.expected over one OracleSim per instance; the info, the ascending
instance indices and their ticks must be equal exactly.  Each scenario runs on the library's choice
of exec kernel (AUTO) and with the instance-per-lane kernel forced where the topology fits it, in
both record layouts (instance-major after flush(), block-major by slot after rerun() of a mapped
plan).  The counts pinned below are the oracle's.
"""
import importlib

import numpy as np
import pytest

import oracle as O
from selectcheck import assert_selection_equal, expected, from_refs, scenario
from statscheck import RING_EVENTS, RING_TOP
from test_census_gpu import (AUTO, C3_EVENTS, C3_TOP, ENGINES, EVENTS3, HUB_EVENTS, HUB_TOP, TOP3, both_layouts,
                             flush_on, make_sim, replay_blocked)

cl = importlib.import_module("chandy-lamport-distributed-snapshot-algorithm_amd")
pytestmark = pytest.mark.gpu

N = 4096                        # the smallest batch that gets a mapped block-major replay
RANGES = [(0, N), (37, 3001)]


def n_match(rows, keys, sid, where, lo=0, hi=N):
    return expected(rows, keys, sid, lo, hi, where)[0][3]


def check(sim, rows, keys, sid, ranges, wheres, what):
    for lo, hi in ranges:
        for where in wheres:
            got = sim.select_instances(sid, where, lo, hi, ticks=True)
            assert_selection_equal(got, expected(rows, keys, sid, lo, hi, where),
                                   f"{what} sid {sid} [{lo}, {hi}) where {where}")


# ---- 1: mixed statuses; sparse, dense, negated and empty selections -------------------------------
C3_SID0 = [
    [("tick", None, 35, None)],                                      # sparse: 22
    [("msgs", None, 3, 3)],                                          # sparse: 5
    [("tick", None, 20, 25)],                                        # dense: 1400
    [("tick", None, 19, 24)],                                        # dense: 1349
    [("node", 4, 1, 4), ("tick", None, 15, 30)],
    [("ch_msgs", 0, 1, 1), ("tick", None, 15, 30)],
    [("node", 4, 1, 4, "not"), ("tick", None, 15, 30)],
    [("ch_msgs", 0, 1, 1, "not"), ("tick", None, 15, 30)],
    [("node", 3, 10, 10), ("ch_msgs", 0, 1, None, "not"), ("inflight", None, 2, 3), ("tick", None, None, 33)],
    [("tick", None, 30, 20)],                                        # lo > hi: nothing
    [("tick", None, 30, 20, "not")],                                 # ... negated: everything
    [],
]


@ENGINES
def test_c3_sparse_dense_negated_and_empty_selections(engine):
    rows, keys = scenario(C3_TOP, C3_EVENTS, N)
    assert rows.n_sids == 5
    fatal = np.flatnonzero(rows.status == O.FATAL_INSUFFICIENT_TOKENS)
    assert fatal.size == 117                                          # the exclusion is exercised
    assert [expected(rows, keys, sid, 0, N, [])[0] for sid in range(5)] == [(N, 3979, 3979, 3979)] * 5
    t0 = rows.tick[0][rows.done[0]]
    assert (int(t0.min()), int(t0.max())) == (10, 40)
    assert [n_match(rows, keys, 0, w) for w in C3_SID0[:4]] == [22, 5, 1400, 1349]
    assert [n_match(rows, keys, 0, w) for w in C3_SID0[9:]] == [0, 3979, 3979]
    assert all(0 < n_match(rows, keys, 0, w) < 3979 for w in C3_SID0[4:9])
    busy = [("msgs", None, 1, None)]
    assert n_match(rows, keys, 4, busy) == 69
    sim = make_sim(C3_TOP, C3_EVENTS, N, engine)

    def body(what):
        check(sim, rows, keys, 0, RANGES, C3_SID0, what)
        check(sim, rows, keys, 4, RANGES, [busy, []], what)
        whole = sim.select_instances(0)
        assert whole.n_match == whole.sample == 3979 and whole.ticks is None
        assert np.intersect1d(whole.insts, fatal).size == 0           # none of the fatal instances

    both_layouts(sim, engine, body)
    assert sim.select_time() > 0


# ---- 2: a histogram bin's count is the size of the selection for that bin; census classes --------
@ENGINES
def test_c3_agrees_with_stats_histograms_and_census_classes(engine):
    sim = make_sim(C3_TOP, C3_EVENTS, N, engine)

    def body(what):
        for sid in range(5):
            st = sim.snapshot_stats(sid, tick_lo=0, tick_bins=64, msg_bins=4)
            hist = st.tick_hist
            assert hist[0] == 0 and hist[-1] == 0 and hist.sum() == st.sample == 3979
            for b in np.flatnonzero(hist[1:-1]) + 1:                  # the non-empty interior bins
                got = sim.select_instances(sid, [("tick", None, int(b), int(b))], max_out=0)
                assert got.n_match == hist[b] and got.n_returned == 0, f"{what} sid {sid} tick bin {b}"
            for c in range(sim.num_channels):
                for m in range(3):                                    # (bin 3 clamps: not one value)
                    got = sim.select_instances(sid, [("ch_msgs", c, m, m)], max_out=0)
                    assert got.n_match == st.ch_msg_hist[c, m], f"{what} sid {sid} channel {c} msgs {m}"
            for lo, hi in RANGES:
                census = sim.snapshot_census(sid, lo, hi, class_of=True)
                assert census.n_returned == census.n_classes > 1
                for k, row in enumerate(census.classes):
                    key = int(row["key"])
                    got = sim.select_instances(sid, [("key", None, key, key)], lo, hi, ticks=True)
                    assert np.array_equal(got.insts, np.flatnonzero(census.class_of == k) + lo), \
                        f"{what} sid {sid} [{lo}, {hi}) class {k}"
                    assert got.n_match == row["count"] and got.insts[0] == row["first_inst"]
                    assert (got.ticks.min(), got.ticks.max()) == (row["min_tick"], row["max_tick"])

    both_layouts(sim, engine, body)


# ---- 3: multi-message channels, keys above 2**63, truncation ---------------------------------------
@ENGINES
def test_channel_tokens_key_ranges_and_truncation(engine):
    rows, keys = scenario(TOP3, EVENTS3, N)
    assert (rows.status == O.OK).all() and rows.n_sids == 2
    assert rows.ch_msgs[0][:, 0].max() == 12 and rows.ch_tok[0][:, 0].max() == 15     # N1 -> N2
    key_lo, key_hi = 2**63 + 12345, 0xd57c989099ce2cd0
    wheres = [
        [("ch_tok", 0, 10, None)],
        [("ch_tok", 0, 10, None, "not"), ("ch_tok", 3, 1, 2)],
        [("inflight", None, 15, 18)],
        [("inflight", None, 3, 8), ("msgs", None, None, 6)],
        [("key", None, key_lo, key_hi)],
        [("key", None, key_lo, key_hi, "not"), ("ch_msgs", 1, 2, 3)],
        [("key", None, key_hi, None), ("tick", None, None, 24)],
    ]
    dense = [("key", None, key_lo, key_hi)]
    assert n_match(rows, keys, 0, dense) > 1000 and n_match(rows, keys, 0, wheres[0]) > 0
    assert all(any(0 < n_match(rows, keys, sid, w) < N for sid in range(2)) for w in wheres)
    sim = make_sim(TOP3, EVENTS3, N, engine)

    def body(what):
        for sid in range(2):
            check(sim, rows, keys, sid, RANGES, wheres, what)
        for lo, hi in RANGES:
            want = expected(rows, keys, 0, lo, hi, dense)
            cut = sim.select_instances(0, dense, lo, hi, max_out=10, ticks=True)
            assert cut.truncated and cut.n_returned == 10 and cut.n_match == want[0][3]
            assert_selection_equal(cut, want, what + " cut", max_out=10)    # the 10 smallest matches
            roomy = sim.select_instances(0, dense, lo, hi, max_out=N, ticks=True)
            assert not roomy.truncated
            assert_selection_equal(roomy, want, what + " roomy")

    both_layouts(sim, engine, body)


# ---- 4: node records of 3 words (not a power of two), 33 record words: not staged ------------------
def hub_wheres(rows, keys, sid, hi):
    vals, counts = np.unique(keys.key[sid][expected(rows, keys, sid, 0, hi, [])[1]], return_counts=True)
    key = int(vals[counts.argmax()])                # the most frequent class
    return [
        [("node", 4, 5, None)],
        [("node", 1, 6, 6), ("node", 0, 30, 40)],
        [("ch_msgs", 11, 1, 1)],
        [("ch_msgs", 3, 1, None, "not"), ("ch_tok", 6, 0, 0)],
        [("key", None, key, key)],
        [("key", None, key, key, "not"), ("msgs", None, 1, None)],
        [("inflight", None, 2, None)],
        [],
    ]


def test_hub_three_word_records_instance_major():
    n = 512
    rows, keys = scenario(HUB_TOP, HUB_EVENTS, N)   # (instance i is seeded by i alone)
    assert (rows.status == O.OK).all() and rows.n_sids == 4
    sim = make_sim(HUB_TOP, HUB_EVENTS, n, AUTO)
    sim.flush()
    assert not sim.records_blocked()
    for sid in range(4):
        check(sim, rows, keys, sid, [(0, n), (5, 300)], hub_wheres(rows, keys, sid, n), "hub after flush")


def test_hub_three_word_records_block_major():
    rows, keys = scenario(HUB_TOP, HUB_EVENTS, N)
    sim = make_sim(HUB_TOP, HUB_EVENTS, N, AUTO)
    sim.flush()
    replay_blocked(sim)
    for sid in range(4):
        wheres = hub_wheres(rows, keys, sid, N)
        assert 0 < n_match(rows, keys, sid, wheres[4]) < N
        check(sim, rows, keys, sid, RANGES, wheres, "hub after rerun")


# ---- 4b: node records of 2 words, 10 record words: staged in LDS word by word ----------------------
def test_ring_two_word_records_both_layouts():
    rows, keys = scenario(RING_TOP, RING_EVENTS, N)
    assert rows.n_sids == 2
    assert int((rows.status == O.OK).sum()) == 2417
    assert int((rows.status == O.FATAL_INSUFFICIENT_TOKENS).sum()) == 1679
    wheres = [
        [("msgs", None, 2, None)],
        [("ch_tok", 1, 2, None)],
        [("node", 2, 0, 1), ("tick", None, None, 12)],
        [("inflight", None, 1, 2, "not")],
    ]
    assert [[n_match(rows, keys, sid, w) for sid in range(2)] for w in wheres] == [[813, 1403], [2238, 0], [13, 0],
                                                                                  [992, 100]]
    sim = make_sim(RING_TOP, RING_EVENTS, N, AUTO)
    assert sim.num_nodes == 5 and sim.num_channels == 5     # max in-degree 1: rec_words gives rw = 2

    def body(what):
        for sid in range(2):
            check(sim, rows, keys, sid, RANGES, wheres + [[]], "ring " + what)

    both_layouts(sim, AUTO, body)


# ---- 5: incomplete snapshots never match; the bulk ticks -------------------------------------------
@ENGINES
def test_incomplete_snapshots_and_bulk_ticks(engine):
    n, k = 256, 8
    refs = []
    for i in range(n):
        r = O.OracleSim()
        r.seed_go(O.REFERENCE_SEED + i)
        assert r.read_topology_text(TOP3) == 0
        assert r.send_tokens("N1", "N2", 1) == 0 and r.send_tokens("N2", "N3", 2) == 0
        assert r.start_snapshot("N1")[0] == 0
        for _ in range(k):
            r.tick()
        refs.append(r)
    rows, keys = from_refs(refs)
    ok, sample = int((rows.status == O.OK).sum()), int(rows.done[0].sum())
    assert ok == n and 0 < sample < ok
    sim = make_sim(TOP3, None, n, engine)
    sim.ProcessEvent(cl.PassTokenEvent("N1", "N2", 1))
    sim.ProcessEvent(cl.PassTokenEvent("N2", "N3", 2))
    assert sim.StartSnapshot("N1") == 0
    sim.Tick(k)
    got = sim.select_instances(0)            # executes the pending events, adds no tick
    assert (got.instances, got.ok, got.sample, got.n_match) == (n, n, sample, sample)
    assert np.array_equal(got.insts, np.flatnonzero(rows.done[0]))
    wheres = [[], [("tick", None, None, None)], [("tick", None, 0, 0, "not")], [("tick", None, -5, 6)],
              [("msgs", None, 0, 0)], [("node", 1, 29, 31), ("key", None, None, None)]]
    check(sim, rows, keys, 0, [(0, n), (3, 201)], wheres, "mid-program")
    want_ticks = np.where(rows.done[0], rows.tick[0], -1).astype(np.int32)
    ticks = sim.snapshot_ticks(0)
    assert ticks.dtype == np.int32 and np.array_equal(ticks, want_ticks)
    assert np.array_equal(sim.snapshot_ticks(0, 3, 201), want_ticks[3:201])
    assert sim.snapshot_ticks(0, 17, 17).size == 0
    assert all(sim.snapshot_tick(0, i) == want_ticks[i] for i in (0, 1, 100, n - 1))


# ---- 6: ranges and plumbing ---------------------------------------------------------------------------
@ENGINES
def test_ranges_ticks_collect_and_timing(engine):
    rows, keys = scenario(C3_TOP, C3_EVENTS, N)
    sim = make_sim(C3_TOP, C3_EVENTS, N, engine)
    where = [("tick", None, 18, 27), ("node", 4, 0, 1)]
    ranges = [(17, 17), (0, 0), (N, N), (100, 101), (1, 63), (63, 65), (64, 128), (65, 127), (5, 4000), (N - 1, N),
              (3000, N)]

    def body(what):
        before = sim.device_bytes
        empty = sim.select_instances(1, where, 17, 17, ticks=True)
        assert (empty.instances, empty.ok, empty.sample, empty.n_match, empty.n_returned) == (0, 0, 0, 0, 0)
        assert empty.insts.size == 0 and empty.ticks.size == 0 and not empty.truncated
        check(sim, rows, keys, 1, ranges, [where, []], what)
        assert sim.device_bytes > before or what != "instance-major"   # the scratch is counted
        all_ticks = sim.snapshot_ticks(1)
        want = expected(rows, keys, 1, 5, 4000, where)
        got = sim.select_instances(1, where, 5, 4000, ticks=True)
        assert got.n_returned == want[1].size > 100 and np.array_equal(got.ticks, all_ticks[got.insts])
        mine, listed = got.collect(sim), sim.collect_snapshot_list(1, want[1])
        assert len(mine) == 4 and all(np.array_equal(a, b) for a, b in zip(mine, listed))
        assert mine[1].all() and mine[0].shape == (want[1].size, sim.num_nodes)
        # the selection of sub-ranges merges into the selection of the whole
        parts = sim.select_instances(1, where, 0, 1000, ticks=True).merge(
            sim.select_instances(1, where, 1000, N, ticks=True))
        assert parts == sim.select_instances(1, where, ticks=True)
        total = sim.select_time()
        evaluate, compact = sim.select_time(stages=True)
        assert total > 0 and evaluate > 0 and compact > 0 and total == pytest.approx(evaluate + compact)

    both_layouts(sim, engine, body)


# ---- ragged batch sizes -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_ragged_batch_sizes(n):
    rows, keys = scenario(TOP3, EVENTS3, N)   # (instance i is seeded by i alone)
    sim = make_sim(TOP3, EVENTS3, n, AUTO)
    flush_on(sim, AUTO)
    wheres = [[], [("ch_tok", 0, 8, None)], [("key", None, 2**63, None), ("tick", None, None, 23)]]
    for sid in range(2):
        check(sim, rows, keys, sid, [(0, n)], wheres, f"n = {n}")
