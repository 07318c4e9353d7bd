"""Graph engine: the per-snapshot summary table reduced on the device
(cl_graph_snapshot_table, cg_table.hip) against the table restated from the CPU oracle alone
(tablecheck.expected_table: collect_channels, completion ticks, the Logger's epochs, digest_of).
Every comparison is exact."""
import functools

import numpy as np
import pytest

import graphcheck as GC
import graphgen as G
import oracle as O
import tablecheck as T
from snapcheck import read_text

pytestmark = pytest.mark.gpu

E_INVALID = -1


def topology_tokens(top):
    """Total tokens of a test_data topology: its "id tokens" lines."""
    total = 0
    for line in read_text(top).splitlines():
        f = line.split()
        if len(f) == 2 and f[1].isdigit():
            total += int(f[1])
    return total


def check(g, o, want, total):
    """The engine's whole table against the oracle's, and against the engine's own checksums."""
    assert g.status() == o.status == 0
    assert g.num_snapshots == o.num_snapshots == want.size
    tab = g.snapshot_table()
    T.assert_rows_equal(tab.rows, want)
    sums = g.checksums()
    assert tab.digest_sum() == sums["digest"] == GC.digest_from_oracle(o)
    assert int(tab.cut_residual(total).sum()) == sums["cut_residual"] == 0
    assert int((tab.rows["complete_tick"] >= 0).sum()) == sums["completed"]
    return tab


@pytest.mark.parametrize("top,events", [("10nodes.top", "10nodes.events"),
                                        ("8nodes.top", "8nodes-concurrent-snapshots.events"),
                                        ("3nodes.top", "3nodes-bidirectional-messages.events")])
def test_reference_scenarios(top, events):
    """Payloads above 1 (the payload history is on), several snapshots, n below one wave."""
    g = GC.scenario_engine(top, events, O.REFERENCE_SEED)
    o = T.scenario_oracle_logged(top, events, O.REFERENCE_SEED)
    want = T.expected_table(o)
    assert (want["rec_tokens"] > want["rec_msgs"]).any()       # a recorded payload above 1
    tab = check(g, o, want, topology_tokens(top))
    assert (tab.latency == want["complete_tick"] - want["start_tick"]).all()


def test_powerlaw_drained():
    """A hub of in-degree above 64, n no multiple of 256, every snapshot complete."""
    p, o, want = T.powerlaw_drained()
    assert np.bincount(p.dst).max() > 64 and p.n % 256
    assert (want["complete_tick"] >= 0).all() and (want["nodes_created"] == p.n).all()
    g = GC.engine_program(p, drain=True)
    tab = check(g, o, want, T.total_tokens(p))
    assert (tab.spread >= 0).all() and (tab.spread <= tab.latency).all()


def test_powerlaw_undrained_progress():
    """Stopped where one snapshot is complete and others are still spreading: the progress
    fields follow the oracle, the channel fields and the digest of incomplete rows are 0."""
    p, o, want = T.powerlaw_undrained()
    assert T.mixed(o)
    open_ = want["complete_tick"] < 0
    assert open_.any() and (~open_).any() and ((want["nodes_created"] > 0) & (want["nodes_created"] < p.n)).any()
    g = GC.engine_program(p)
    tab = check(g, o, want, T.total_tokens(p))
    T.assert_rows_equal(tab.rows, want, T.PROGRESS)
    for f in T.CHANNEL:
        assert (tab.rows[f][open_] == 0).all(), f
    assert (tab.latency[open_] == -1).all()


@functools.lru_cache(maxsize=None)
def regular_case():
    p = GC.regular_program(4096, steps=90, snaps=((5, None), (5, 0), (9, None), (17, None)))
    o = GC.oracle_program(p, log=True)
    return p, o, T.expected_table(o)


def test_regular_whole_table_and_subranges():
    p, o, want = regular_case()
    g = GC.engine_program(p)
    tab = check(g, o, want, T.total_tokens(p))
    for lo, hi in ((1, 3), (3, 4), (2, 2)):
        sub = g.snapshot_table(lo, hi)
        assert len(sub) == hi - lo
        T.assert_rows_equal(sub.rows, tab.rows[lo:hi])
        assert sub == GC.clg.SnapshotTable(want[lo:hi])


def test_many_sids_on_a_tiny_graph():
    """300 snapshots, one per tick, on 64 nodes: the workgroups stride over the sids."""
    n, s = 64, 300
    src, dst = G.regular_graph(n, 4, 5)
    p = GC.Program(np.full(n, 100), src, dst, s + 2, traffic_seed=6, thresh=1 << 30, traffic_steps=s + 2,
                   snap_step=list(range(s)), snap_rank=[G.mulhi(G.counter_hash(8, i, 0), n) for i in range(s)],
                   delay_seed=7, fifo_slots=512)
    o = GC.oracle_program(p, drain=True, log=True)
    want = T.expected_table(o)
    assert want.size == s and (want["complete_tick"] >= 0).all()
    g = GC.engine_program(p, drain=True)
    assert g.num_snapshots == s
    check(g, o, want, T.total_tokens(p))


@pytest.mark.parametrize("n", [1, 2])
def test_degenerate_graphs(n):
    """One node without channels (the oracle never completes its snapshot: no marker ever
    arrives), and two nodes with one channel each way."""
    src, dst = (np.zeros(0, np.int32), np.zeros(0, np.int32)) if n == 1 else (np.array([0, 1]), np.array([1, 0]))
    p = GC.Program(np.full(n, 100), src, dst, 12, traffic_seed=6, thresh=1 << 30, traffic_steps=6, snap_step=[1],
                   snap_rank=[0], delay_seed=7)
    o = GC.oracle_program(p, log=True)
    want = T.expected_table(o)
    assert want["nodes_created"][0] == n and want["initiator"][0] == 0
    g = GC.engine_program(p)
    check(g, o, want, T.total_tokens(p))


def test_push_lane_settings_give_one_table():
    p, o, want = T.powerlaw_drained()
    tabs = [GC.engine_program(p, lanes=lanes, drain=True).snapshot_table() for lanes in (1, 4)]
    assert tabs[0] == tabs[1]
    T.assert_rows_equal(tabs[0].rows, want)


@pytest.mark.parametrize("drain", [True, False])
def test_rerun_into_poisoned_planes(drain):
    """The table of a rerun into poisoned result planes is the run's own: nothing stale is
    read, and -- undrained -- no cursor of an incomplete snapshot is read at all."""
    p, o, want = T.powerlaw_drained() if drain else T.powerlaw_undrained()
    g = GC.engine_program(p, drain=drain)
    first = g.snapshot_table()
    g.poison_outputs()
    g.rerun()
    g.synchronize()
    again = g.snapshot_table()
    assert again == first
    T.assert_rows_equal(again.rows, want)


def test_argument_errors():
    p, _, _ = regular_case()
    g = GC.engine_program(p)
    s = g.num_snapshots
    for lo, hi in ((0, s + 1), (-1, s), (3, 2)):
        with pytest.raises(GC.cl.ClSnapError) as e:
            g.snapshot_table(lo, hi)
        assert e.value.code == E_INVALID


def test_table_time_is_positive():
    p, _, _ = regular_case()
    g = GC.engine_program(p)
    g.snapshot_table()
    assert g.table_time() > 0
