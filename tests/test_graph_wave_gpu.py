"""Graph engine: the marker-wave profile and the marker tree read out on the device
(cl_graph_snapshot_wave, cl_graph_snapshot_tree, cg_wave.hip) against the values restated from
the CPU oracle's Logger alone (wavecheck.Expected).  Every comparison is exact, and every profile
has CL_WV_BROKEN == 0 (wavecheck.assert_wave)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import graphcheck as GC
import graphgen as G
import oracle as O
import tablecheck as T
import wavecheck as WC
from snapcheck import TEST_DATA

pytestmark = pytest.mark.gpu

cl, clg = GC.cl, GC.clg
HEAD = WC.HEAD
SPECS = ((64, 1, 32), (5, 3, 2))


def check(g, x, spec, **kw):
    """The engine's trees and its profile of all sids against the helper's; the profile back."""
    WC.assert_trees(g.snapshot_tree(), x.trees())
    w = g.snapshot_wave(lat_bins=spec[0], lat_width=spec[1], depth_bins=spec[2], **kw)
    WC.assert_wave(w, x.rows(*spec, origins=kw.get("origins")), spec)
    return w


@pytest.mark.parametrize("top,events", [("10nodes.top", "10nodes.events"),
                                        ("8nodes.top", "8nodes-concurrent-snapshots.events"),
                                        ("3nodes.top", "3nodes-bidirectional-messages.events")])
def test_reference_scenarios(top, events):
    """n below one wave, several snapshot ids, the Go delay stream."""
    g = GC.scenario_engine(top, events, O.REFERENCE_SEED)
    x = WC.Expected(T.scenario_oracle_logged(top, events, O.REFERENCE_SEED))
    assert g.status() == 0 and g.num_snapshots == x.parent.shape[0]
    for spec in SPECS:
        w = check(g, x, spec)
        assert (w.created == g.num_nodes).all() and (w.depth_hist[:, 0] == 1).all()
    for t, want in zip(g.snapshot_tree(ticks=False), x.trees()):
        assert t.tick is None
        np.testing.assert_array_equal(t.parent, want.parent)
        np.testing.assert_array_equal(t.depth(), x.depth[want.sid])


@functools.lru_cache(maxsize=None)
def powerlaw_engine():
    p, _, _, _ = WC.powerlaw_drained()
    return GC.engine_program(p, drain=True)


def test_powerlaw_both_last_bins_clamp():
    """A hub of in-degree above 64, n no multiple of 256: every depth histogram and most latency
    histograms end in a clamped bin."""
    p, o, table, x = WC.powerlaw_drained()
    assert np.bincount(p.dst).max() > 64 and p.n % 256
    spec = (64, 2, 8)
    want = x.rows(*spec)
    assert (want[:, WC.W["lat_max"]] >= 64 * 2).any() and (want[:, WC.W["depth_max"]] >= 8).all()
    assert (want[:, HEAD + 63] > 0).any() and (want[:, HEAD + 64 + 7] > 1).all()
    w = check(powerlaw_engine(), x, spec)
    assert (w.coverage()[:, -1] == 1.0).all()


def test_powerlaw_nothing_clamps_and_agrees_with_the_table():
    p, o, table, x = WC.powerlaw_drained()
    spec = (256, 1, 32)
    want = x.rows(*spec)
    assert (want[:, WC.W["lat_max"]] < 255).all() and (want[:, WC.W["depth_max"]] < 31).all()
    assert (want[:, HEAD + 255] == 0).all() and (want[:, HEAD + 256 + 31] == 0).all()
    g = powerlaw_engine()
    w = check(g, x, spec)
    tab = g.snapshot_table().rows
    T.assert_rows_equal(tab, table)
    np.testing.assert_array_equal(w.created, tab["nodes_created"])
    np.testing.assert_array_equal(w.origin, tab["start_tick"])
    np.testing.assert_array_equal(w.origin + w.word("lat_max"), tab["last_create_tick"])
    assert (w.word("lat_min") == 0).all() and (w.depth_hist[:, 0] == 1).all()
    for t in g.snapshot_tree():
        d, made = t.depth(), t.created
        lat = t.tick.astype(np.int64) - w.origin[t.sid]
        assert made.all() and (d >= 0).all() and (d <= lat).all()      # a hop takes a tick at least
        np.testing.assert_array_equal(np.bincount(d, minlength=32), w.depth_hist[t.sid])
        assert t.path(int(np.argmax(d)))[-1] == tab["initiator"][t.sid] and len(t.path(int(np.argmax(d)))) == d.max() + 1


def test_powerlaw_undrained_leaves_uncreated_nodes_out():
    """Stopped while snapshots are still spreading: holes in the trees, created < n."""
    p, o, table, x = WC.powerlaw_undrained()
    assert T.mixed(o)
    g = GC.engine_program(p)
    w = check(g, x, (256, 1, 32))
    assert (w.created < p.n).any() and (w.created > 0).all()
    np.testing.assert_array_equal(w.created, table["nodes_created"])
    trees = g.snapshot_tree()
    assert any((t.parent == -2).any() for t in trees)
    for t in trees:
        assert ((t.parent == -2) == (t.tick == -1)).all() and int(t.created.sum()) == w.created[t.sid]
        np.testing.assert_array_equal(t.depth(), x.depth[t.sid])


@functools.lru_cache(maxsize=None)
def regular_case():
    p = GC.regular_program(4096, steps=90, snaps=((5, None), (5, 0), (9, None), (17, None)))
    o = GC.oracle_program(p, log=True)
    return p, WC.Expected(o)


@functools.lru_cache(maxsize=None)
def regular_engine():
    return GC.engine_program(regular_case()[0])


def test_regular_subranges_and_chunks():
    """The whole range equals its sub-ranges back to back, whatever the scratch budget: 2 sids,
    then 1 sid per chunk of pairs and of packed planes."""
    p, x = regular_case()
    g = regular_engine()
    spec = (32, 2, 16)
    whole = check(g, x, spec)
    trees = g.snapshot_tree()
    for budget in (0, 2 * 8 * p.n, 1):
        g.set_wave_scratch(budget)
        parts = [g.snapshot_wave(lo, hi, *spec) for lo, hi in ((0, 1), (1, 3), (3, 4))]
        np.testing.assert_array_equal(np.concatenate([w.rows for w in parts]), whole.rows)
        assert g.snapshot_wave(0, None, *spec) == whole
        sub = [t for lo, hi in ((0, 1), (1, 3), (3, 4)) for t in g.snapshot_tree(lo, hi)]
        assert [t.sid for t in sub] == [0, 1, 2, 3]
        WC.assert_trees(sub, trees)
        WC.assert_trees(g.snapshot_tree(), trees)
    g.set_wave_scratch(0)
    assert len(g.snapshot_wave(2, 2)) == 0 and g.snapshot_tree(2, 2) == []


def test_regular_origins_shift_the_latencies():
    """Origins 3 ticks after the start: every latency drops by 3, and the nodes created before the
    shifted origin land in bin 0."""
    p, x = regular_case()
    g = regular_engine()
    spec = (32, 2, 16)
    base = g.snapshot_wave(0, None, *spec)
    shifted = check(g, x, spec, origins=x.origin + 3)
    np.testing.assert_array_equal(shifted.origin, base.origin + 3)
    np.testing.assert_array_equal(shifted.word("lat_sum"), base.word("lat_sum") - 3 * base.created)
    np.testing.assert_array_equal(shifted.word("lat_min"), base.word("lat_min") - 3)
    np.testing.assert_array_equal(shifted.word("lat_max"), base.word("lat_max") - 3)
    assert (shifted.word("lat_min") == -3).all()
    early = np.array([((x.tick[s] >= 0) & (x.tick[s] - x.origin[s] < 3 + 2)).sum() for s in range(4)])
    np.testing.assert_array_equal(shifted.lat_hist[:, 0], early)      # latencies -3 .. 1
    np.testing.assert_array_equal(shifted.depth_hist, base.depth_hist)
    # the caller's origins also stand in for a start the part does not know
    same = g.snapshot_wave(0, None, *spec, origins=x.origin)
    assert same == base


def test_ring_depth_beyond_a_workgroup():
    """A directed ring of 600: one chain of depth 599, more than a workgroup's threads and ten
    doublings deep -- a doubling that stops early, or composes a half-written pair, shows here."""
    p, o, x = WC.ring_drained()
    assert o.time == 1840 and x.depth.max() == 599 and (x.tick[0] - x.origin[0]).max() == 1829
    g = GC.engine_program(p, drain=True)
    assert g.status() == 0 and g.time() == o.time
    spec = (64, 32, 1024)
    w = check(g, x, spec)
    ms, rounds = g.wave_time()
    assert ms > 0 and 10 <= rounds <= 32, rounds
    assert w.depth_hist[0, :600].tolist() == [1] * 600 and w.depth_hist[0, 600:].sum() == 0
    assert w.word("depth_max")[0] == 599 and w.word("depth_sum")[0] == 599 * 600 // 2
    assert w.word("lat_max")[0] == 1829
    tree = g.snapshot_tree()[0]
    assert tree.path(199) == [(199 - i) % 600 for i in range(600)]
    g.snapshot_wave(depth_bins=0)
    assert g.wave_time()[1] == 0                         # no doubling without the depth


def test_many_sids_on_a_tiny_graph():
    """1,100 snapshots on 32 nodes: more rows than the reduction's grid has workgroup rows, so
    they stride over the sids."""
    n, s = 32, 1100
    src, dst = G.regular_graph(n, 3, 5)
    p = GC.Program(np.full(n, 100), src, dst, s + 2, traffic_seed=6, thresh=1 << 28, traffic_steps=s + 2,
                   snap_step=list(range(s)), snap_rank=[G.mulhi(G.counter_hash(8, i, 0), n) for i in range(s)],
                   delay_seed=7, fifo_slots=4096)
    o = GC.oracle_program(p, drain=True, log=True)
    x = WC.Expected(o)
    g = GC.engine_program(p, drain=True)
    assert g.status() == o.status == 0 and g.num_snapshots == s
    w = check(g, x, (48, 64, 16))
    assert (w.created == n).all()


def test_rerun_into_poisoned_planes():
    p, o, table, x = WC.powerlaw_drained()
    g = GC.engine_program(p, drain=True)
    spec = (64, 2, 8)
    first = g.snapshot_wave(0, None, *spec)
    trees = g.snapshot_tree()
    before = g.device_bytes
    g.poison_outputs()
    g.rerun()
    g.synchronize()
    again = g.snapshot_wave(0, None, *spec)
    assert again.rows.tobytes() == first.rows.tobytes()
    for a, b in zip(g.snapshot_tree(), trees):
        assert a.parent.tobytes() == b.parent.tobytes() and a.tick.tobytes() == b.tick.tobytes()
    WC.assert_wave(again, x.rows(*spec), spec)
    assert g.device_bytes == before


def test_limits_and_status_on_a_flushed_graph():
    p, x = regular_case()
    g = regular_engine()
    s = g.num_snapshots
    for lo, hi in ((0, s + 1), (-1, s), (3, 2)):
        for call in (g.snapshot_wave, g.snapshot_tree):
            with pytest.raises(cl.ClSnapError) as e:
                call(lo, hi)
            assert e.value.code == cl.E_INVALID
    for bad in (dict(lat_bins=0), dict(lat_bins=1025), dict(lat_width=0), dict(depth_bins=-1), dict(depth_bins=1025)):
        with pytest.raises(cl.ClSnapError) as e:
            g.snapshot_wave(**bad)
        assert e.value.code == cl.E_INVALID, bad
    spec = np.zeros(1, dtype=clg.WAVE_SPEC_DTYPE)
    spec["lat_bins"], spec["lat_width"], spec["depth_bins"] = 8, 1, 4
    rw = HEAD + 12
    out = np.full(s * rw, 77, dtype=np.int64)
    call = lambda words: g._L.cl_graph_snapshot_wave(g._h, 0, s, cl._p(spec), None, cl._p(out), words)  # noqa: E731
    assert call(s * rw - 1) == cl.E_LIMIT and (out == 77).all()
    assert call(s * rw) == 0
    WC.assert_wave(clg.SnapshotWave(out, 8, 1, 4), x.rows(8, 1, 4), (8, 1, 4))
    # the pairs are counted while they are held
    before = g.device_bytes
    g.set_wave_scratch(0)
    g.snapshot_wave()
    assert g.device_bytes >= before and g.device_bytes >= 8 * p.n * s
    ms, rounds = g.wave_time()
    assert ms > 0 and 1 <= rounds <= 32
    t = C.c_double(0)
    assert g._L.cl_graph_wave_time(g._h, C.byref(t), None) == 0 and t.value == ms


def test_device_bytes_count_the_wave_alone_of_the_readouts():
    """The byte count over the engine and its readouts: the table and the sparse collect add
    nothing to it, the first wave adds its pairs, rows and origins (both sids in one chunk of the
    default budget), and a graph deleted with every readout buffer alive goes cleanly."""
    g = clg.GraphSim()
    g.read_topology_file(os.path.join(TEST_DATA, "3nodes.top"))
    g.set_delay_go_seed(O.REFERENCE_SEED)
    n, s = g.num_nodes, 2
    assert n == 3 and [g.StartSnapshot("N1"), g.StartSnapshot("N3")] == [0, 1]
    g.drain()
    assert g.status() == 0
    before = g.device_bytes
    assert before > 0
    assert len(g.snapshot_table()) == s and len(g.collect_sparse(tokens=True)) == s
    assert g.device_bytes == before
    w = g.snapshot_wave(0, s, lat_bins=4, depth_bins=2)
    assert (w.created == n).all()
    assert HEAD == 12 and g.device_bytes - before == 8 * n * 2 + 8 * 2 * (12 + 4 + 2) + 8 * 2
    del g
