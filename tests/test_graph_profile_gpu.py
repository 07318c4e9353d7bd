"""GPU tests of the graph engine's node and channel profile over a snapshot range
(GraphSim.snapshot_profile, cl_graph_snapshot_profile) against the CPU oracle
(profilecheck.expected_profile) and the engine's own table and wave -- all exact.  Shapes: fewer
channels than one wave (the reference scenarios), several channel tiles with a ragged last one and
hubs on both sides of every in-degree threshold of the segmented sum (2000-node power-law), a
payload history (600-node regular text program), complete and incomplete snapshots, one and
several slices of the used list."""
import functools
import os
import re

import numpy as np
import pytest

import graphcheck as GC
import oracle as O
import profilecheck as PC
import tablecheck as T
from snapcheck import ROOT
from test_graph_sparse_gpu import regular_text_program

pytestmark = pytest.mark.gpu

cl, clg = GC.cl, GC.clg
PF = PC.PF
HEAD = len(clg.PROFILE_HEAD)


def check(g, o, dst, unit, sid_lo=0, sid_hi=None, **kw):
    """One snapshot_profile call against the oracle; the profile."""
    sid_hi = o.num_snapshots if sid_hi is None else sid_hi
    got = g.snapshot_profile(sid_lo, sid_hi, **kw)
    nodes = kw.get("nodes", True)
    want = PC.expected_profile(o, sid_lo, sid_hi, use=kw.get("use"), min_msgs=kw.get("min_msgs", 1),
                               msg_bins=kw.get("msg_bins", 64), msg_width=kw.get("msg_width", 1),
                               origins=kw.get("origins"), nodes=nodes, unit_payloads=unit, dst=dst)
    PC.assert_profile_equal(got, want, nodes=nodes)
    return got


def identities(g, pr, sid_lo, sid_hi):
    """A full profile (min_msgs=1, msg_width=1, default origins) against the engine's own table and
    wave of the same range."""
    u = pr.used != 0
    rows = g.snapshot_table(sid_lo, sid_hi).rows
    assert pr.word("msgs") == rows["rec_msgs"][u].sum() and pr.word("tokens") == rows["rec_tokens"][u].sum()
    assert pr.word("active") == pr.word("entries") == pr.entries.size
    assert pr.word("max_peak") == (rows["max_ch_msgs"][u].max() if u.any() else 0)
    assert pr.hist.sum() == pr.word("channels")
    for m in (1, 2, 3):                      # (below the last bin, which gathers everything above it)
        q = g.snapshot_profile(sid_lo, sid_hi, use=pr.used, min_msgs=m, nodes=False)
        assert q.entries.size == q.word("entries") == pr.hist[m:].sum() and (q.entries["msgs"] >= m).all()
    wave = g.snapshot_wave(sid_lo, sid_hi, depth_bins=0)
    assert pr.node["lat_sum"].sum() == wave.word("lat_sum")[u].sum()
    assert pr.node["tok_sum"].sum() == rows["node_tokens"][u].sum()
    assert pr.node["in_msgs"].sum() == pr.word("msgs") and pr.node["in_tokens"].sum() == pr.word("tokens")


@pytest.mark.parametrize("top,events,unit", [("2nodes.top", "2nodes-message.events", 1),
                                             ("8nodes.top", "8nodes-concurrent-snapshots.events", 0),
                                             ("10nodes.top", "10nodes.events", 0)])
def test_reference_scenarios(top, events, unit):
    """Fewer channels than one wave; unit payloads and payloads from the history."""
    g = GC.scenario_engine(top, events, O.REFERENCE_SEED)
    o = T.scenario_oracle_logged(top, events, O.REFERENCE_SEED)
    ns = o.num_snapshots
    assert g.status() == o.status == 0 and g.num_snapshots == ns and ns > 0
    dst = g.channels()[1]
    pr = check(g, o, dst, unit)
    assert pr.n_used == ns and pr.word("unit_payloads") == unit and pr.word("msgs") > 0
    assert (pr.word("tokens") > pr.word("msgs")) == (not unit)
    identities(g, pr, 0, ns)
    for sid in range(ns):
        check(g, o, dst, unit, sid, sid + 1)
    check(g, o, dst, unit, msg_bins=2, msg_width=2, min_msgs=2)


@functools.lru_cache(maxsize=None)
def powerlaw_run():
    """(engine, oracle, program) of the drained power-law run: unit payloads, 12 snapshots over
    several channel tiles, hubs."""
    p, o, _ = T.powerlaw_drained()
    g = GC.engine_program(p, drain=True)
    assert g.status() == o.status == 0
    np.testing.assert_array_equal(g.channels()[1], p.dst)
    return g, o, p


def test_powerlaw_ranges_masks_and_specs():
    g, o, p = powerlaw_run()
    ns = o.num_snapshots
    assert ns == 12 and g.num_channels > 4 * 2048 and g.num_channels % 2048 != 0
    full = check(g, o, p.dst, 1)
    assert full.n_used == ns and full.entries.size > 0 and full.word("unit_payloads") == 1
    np.testing.assert_array_equal(full.entries["tokens"], full.entries["msgs"])
    assert full.word("max_snaps") > 1 and full.word("max_msgs") > full.word("max_peak") > 0
    identities(g, full, 0, ns)
    check(g, o, p.dst, 1, 3, 7)
    for sid in range(ns):
        one = check(g, o, p.dst, 1, sid, sid + 1)
        assert (one.entries["peak_sid"] == sid).all() and (one.entries["snaps"] == 1).all()
    half = check(g, o, p.dst, 1, use=np.arange(ns) % 2 == 0)
    assert half.n_used == 6 and half.used.tolist() == [1, 0] * 6 and (half.entries["peak_sid"] % 2 == 0).all()
    identities(g, half, 0, ns)
    none = check(g, o, p.dst, 1, use=np.zeros(ns, dtype=np.int32))
    assert none.n_used == 0 and none.entries.size == 0 and none.hist[0] == g.num_channels
    assert all(tuple(r) == PC.NODE_IDENTITY for r in none.node.tolist())
    assert np.isnan(none.mean_latency()).all()
    for m in (1, 2, full.word("max_msgs"), full.word("max_msgs") + 1):
        q = check(g, o, p.dst, 1, min_msgs=m)
        assert (q.entries.size == 0) == (m > full.word("max_msgs"))
    check(g, o, p.dst, 1, msg_bins=3, msg_width=2)            # the last bin gathers the rest
    check(g, o, p.dst, 1, msg_bins=clg.PROFILE_MAX_BINS, msg_width=1, max_entries=5)
    # explicit origins, some after the creation ticks: negative latencies
    org = full_origins(o) + np.array([0, 5, -3, 400, 1, 0, 10**6, -7, 2, 0, 60, 9])
    late = check(g, o, p.dst, 1, origins=org)
    assert late.node["lat_sum"].min() < 0 < late.node["lat_max"].max()
    behind = check(g, o, p.dst, 1, 3, 7, origins=org[3:7] + 10**6, use=[1, 0, 0, 1])
    assert behind.node["lat_max"].max() < 0
    bare = check(g, o, p.dst, 1, nodes=False)
    assert bare.node is None
    # the drill-down: the hottest channel's peak snapshot holds that many messages on it
    hot = full.hottest(1)[0]
    ch, cnt, _ = g.collect_sparse(int(hot["peak_sid"]), int(hot["peak_sid"]) + 1, payloads=False).entries(
        int(hot["peak_sid"]))
    assert cnt[ch == hot["channel"]].tolist() == [hot["peak"]]


def full_origins(o):
    return T.creation_epochs(o)[1].copy()


def test_hubs_on_both_sides_of_the_segmented_sum_thresholds():
    """k_profile_in sums a node's in-channels by its own lane up to kProfileLaneDeg, by a wave up to
    kProfileWaveDeg and by the workgroup above: the power-law run has recording nodes in all three."""
    text = open(os.path.join(ROOT, GC.PKG, "csrc", "cg_engine.h")).read()
    lane_deg = int(re.search(r"constexpr int32_t kProfileLaneDeg = (\d+);", text).group(1))
    wave_deg = int(re.search(r"constexpr int32_t kProfileWaveDeg = (\d+);", text).group(1))
    assert (lane_deg, wave_deg) == (8, 256)
    g, o, p = powerlaw_run()
    deg = np.bincount(p.dst, minlength=p.n)
    pr = check(g, o, p.dst, 1)
    for name, cls in (("lane", deg <= lane_deg), ("wave", (deg > lane_deg) & (deg <= wave_deg)),
                      ("workgroup", deg > wave_deg)):
        assert cls.sum() >= 2 and (pr.node["in_msgs"][cls] > 0).any(), name
    for d in (lane_deg, lane_deg + 1):                          # right at the first threshold
        assert (deg == d).any(), d
    assert deg.max() > 2 * wave_deg                             # more than one stride of the workgroup
    # a hub and a leaf in one workgroup of 256 nodes, and a workgroup without a hub
    block = np.arange(p.n) // 256
    hubs = np.bincount(block[deg > wave_deg], minlength=block.max() + 1)
    assert (hubs > 0).any() and (hubs == 0).any()


def test_slices_do_not_change_a_byte():
    g, o, p = powerlaw_run()
    org = full_origins(o) + 3
    try:
        got = {}
        for s in (1, 5, 12, 0):
            g.set_profile_slices(s)
            a = g.snapshot_profile()
            b = g.snapshot_profile(1, 11, use=[1, 1, 0, 1, 1, 1, 0, 1, 1, 1], origins=org[1:11], min_msgs=2)
            got[s] = [x.tobytes() for pr in (a, b) for x in (pr.head, pr.hist, pr.used, pr.entries, pr.node)]
        assert got[1] == got[5] == got[12] == got[0]
        g.set_profile_slices(12)
        check(g, o, p.dst, 1)                                   # and they are the oracle's
        g.set_profile_slices(5)
        check(g, o, p.dst, 1, 2, 9, use=[0, 1, 1, 1, 0, 1, 1])
    finally:
        g.set_profile_slices(0)


def test_mixed_completion_and_poisoned_planes():
    p, o, _ = T.powerlaw_undrained()
    assert T.mixed(o)
    g = GC.engine_program(p)
    ns = o.num_snapshots
    done = np.array([o.complete(sid) for sid in range(ns)])
    assert done.any() and not done.all()
    pr = check(g, o, p.dst, 1)
    np.testing.assert_array_equal(pr.used != 0, done)           # incomplete rows are not used
    assert pr.n_used == done.sum() and done[pr.entries["peak_sid"]].all()
    identities(g, pr, 0, ns)
    # a mask over incomplete rows alone uses nothing
    none = check(g, o, p.dst, 1, use=~done)
    assert none.n_used == 0 and none.word("msgs") == 0 and none.entries.size == 0
    try:
        g.set_profile_slices(3)
        check(g, o, p.dst, 1)
    finally:
        g.set_profile_slices(0)
    # nothing comes from incomplete planes or stale buffers: poison, rerun, the same bytes
    g.poison_outputs()
    g.rerun()
    again = g.snapshot_profile()
    for f in ("head", "hist", "used", "entries", "node"):
        assert getattr(again, f).tobytes() == getattr(pr, f).tobytes(), f


def test_payload_history_over_several_tiles():
    p, top, events = regular_text_program()
    o = O.OracleSim()
    o.use_counter_hash(p.delay_seed)
    o.log_enable()
    assert o.read_topology_text(top) == 0
    assert o.read_events_text(events) == 0
    g = clg.GraphSim()
    g.read_topology_text(top)
    g.set_delay_hash(p.delay_seed)
    assert g.read_events_text(events) == 3
    g.flush()
    assert g.status() == o.status == 0
    e = g.num_channels
    assert 2 * 2048 < e < 3 * 2048
    dst = g.channels()[1]
    pr = check(g, o, dst, 0)
    assert pr.n_used == 3 and pr.word("unit_payloads") == 0
    assert (pr.entries["tokens"] > pr.entries["msgs"]).all() and pr.word("tokens") > pr.word("msgs")
    assert pr.entries["channel"].min() < 2048 and pr.entries["channel"].max() >= 2 * 2048     # first and last tile
    # peak_sid against the oracle's per-snapshot counts, restated here
    cnt = np.stack([np.diff(o.collect_channels(s)[1]) for s in range(3)])
    ch = pr.entries["channel"]
    np.testing.assert_array_equal(pr.entries["peak"], cnt[:, ch].max(axis=0))
    np.testing.assert_array_equal(pr.entries["peak_sid"], cnt[:, ch].argmax(axis=0))
    assert len(set(pr.entries["peak_sid"].tolist())) > 1
    identities(g, pr, 0, 3)
    check(g, o, dst, 0, 1, 3, use=[0, 1], min_msgs=2, msg_width=2, msg_bins=5)
    try:
        g.set_profile_slices(2)
        check(g, o, dst, 0)
    finally:
        g.set_profile_slices(0)


def test_capacity_protocol():
    g, o, p = powerlaw_run()
    ns, n = o.num_snapshots, g.num_nodes
    want = PC.expected_profile(o, 0, ns, dst=p.dst)
    ne = want.entries.size
    assert ne > 1
    spec = np.zeros(1, dtype=clg.PROFILE_SPEC_DTYPE)
    spec["msg_bins"], spec["msg_width"], spec["min_msgs"] = 64, 1, 1

    def fetch(cap, entries=True):
        head = np.full(HEAD + 64, -7, dtype=np.int64)
        used = np.full(ns, -7, dtype=np.int32)
        rows = np.full(n, -7, dtype=clg.PROFILE_NODE_DTYPE)
        ent = np.zeros(ne + 1, dtype=clg.PROFILE_ENTRY_DTYPE)
        ent.view(np.int64)[:] = -7
        rc = g._snapshot_profile(0, ns, spec, None, None, head, used, rows if entries else None,
                                 ent if entries else None, cap)
        np.testing.assert_array_equal(head[:HEAD], want.head)       # written whenever the reduction ran
        np.testing.assert_array_equal(head[HEAD:], want.hist)
        np.testing.assert_array_equal(used, want.used)
        return rc, rows, ent

    rc, _, _ = fetch(0, entries=False)                              # the sizing call
    assert rc == cl.E_LIMIT
    rc, rows, ent = fetch(ne)                                       # the exact cap
    assert rc == 0
    np.testing.assert_array_equal(ent[:ne], want.entries)
    np.testing.assert_array_equal(rows, want.node)
    assert (ent[ne:].view(np.int64) == -7).all()                    # nothing past the total
    rc, rows, ent = fetch(ne - 1)                                   # one short
    assert rc == cl.E_LIMIT
    assert (ent.view(np.int64) == -7).all() and (rows.view(np.int64) == -7).all()
    # the wrapper repeats the call once with the exact size
    assert g.snapshot_profile(max_entries=ne - 1) == g.snapshot_profile(max_entries=ne) == want
    assert g.snapshot_profile(max_entries=0) == want


def test_profile_time_and_device_bytes():
    p, _, _ = T.powerlaw_drained()
    g = GC.engine_program(p, drain=True)
    with pytest.raises(cl.ClSnapError) as e:
        g.profile_time()
    assert e.value.code == cl.E_STATE
    before = g.device_bytes
    g.snapshot_profile()
    assert g.profile_time() > 0
    # the scratch: 32 B per owned in-position and 64 B per owned node, and little else
    scratch = 32 * g.num_channels + 64 * g.num_nodes
    grown = g.device_bytes - before
    assert scratch <= grown <= scratch + 32 * g.num_channels + (1 << 16)
    g.snapshot_profile(0, 1, nodes=False)
    assert g.profile_time() > 0 and g.device_bytes - before == grown
