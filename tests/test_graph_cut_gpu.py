"""GPU tests of the restore from a host-held cut (cl_graph_restore_cut, GraphSim.restore_cut /
cut / from_cut): the cut of a run must equal the oracle's, a graph restored from it on a template
that never ran must be indistinguishable from GraphSim.restore of the same snapshot and from the
host route (restorecheck), and the device check must refuse every malformed cut with the element
named, before any seed kernel can see it.  Sources, scenarios and continuations are those of
test_graph_restore_gpu.py; the figures asserted there were produced on the CPU oracle.  Shapes:
fewer entries than one wave (the reference scenarios), 8,580 entries / 14,699 messages over 2,000
nodes (several workgroups of the check kernel, ragged ends), non-unit payloads, one entry of
32,760 messages."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cutcheck as CC
import graphcheck as GC
import graphgen as G
import restorecheck as R
import tablecheck as T
import test_graph_restore_gpu as RT
from snapcheck import TEST_DATA

pytestmark = pytest.mark.gpu

cl, clg = GC.cl, GC.clg
SEED = RT.SEED
INT32_MIN = -2**31


def scenario_template(top, **kw):
    """A fresh graph of a reference topology under the reference Go seed: never flushed."""
    t = clg.GraphSim(**kw)
    t.read_topology_file(os.path.join(TEST_DATA, top))
    t.set_delay_go_seed(SEED)
    return t


def error_code(call, *args):
    """The code of the ClSnapError that call(*args) must raise.  The exception is let go of here:
    kept in a test's frame it would tie that frame, and every graph in it, into a reference cycle
    that only the garbage collector takes apart, whenever and in whichever process it next runs."""
    with pytest.raises(cl.ClSnapError) as e:
        call(*args)
    code = e.value.code
    del e
    return code


def topology_bytes(t):
    """The device bytes of a graph that holds its topology's arrays and nothing else."""
    n, e = t.num_nodes, t.num_channels
    return 2 * 4 * (n + 1) + (8 + 4 + 1) * e + 4 * n


@pytest.mark.parametrize("top,events,sid,m,payloads,channel", RT.SCENARIOS)
def test_reference_scenarios(top, events, sid, m, payloads, channel):
    g, o = RT.scenario(top, events)
    seed = R.seed_of_oracle(o, sid, *g.channels())
    cut = g.cut(sid)
    CC.assert_cut_is_seed(cut, seed, sid)
    assert cut.msgs == m and cut.topology_key == g.topology_key() and not cut.has_topology
    template = scenario_template(top)
    assert template.device_bytes == 0
    r2 = template.restore_cut(cut)
    assert template.device_bytes == topology_bytes(template)          # none of the template's run planes
    R.check_time0(r2, seed, sid)
    build_ms, seed_ms = r2.restore_time()
    assert build_ms > 0 and seed_ms >= 0 and (seed_ms > 0 or m == 0)
    n = g.num_nodes
    ops = [("snap", n // 2), ("tick", 2), RT.a_send(seed), ("snap", 0), ("tick", 1), ("drain",)]
    R.run_engine(r2, ops)
    R.compare_engines(R.run_engine(g.restore(sid), ops), r2)
    GC.compare(r2, R.oracle_equivalent(seed, ("go", SEED), ops))
    assert r2.num_snapshots == 2 and r2.checksums()["completed"] == 2
    b = R.engine_equivalent(seed, ("go", SEED), run=False)
    np.testing.assert_array_equal(R.step_tokens(template.restore_cut(cut)), R.step_tokens(b))


@functools.lru_cache(maxsize=None)
def powerlaw_cut():
    """(source engine, seed of sid 1, its cut)."""
    g, seed = RT.powerlaw_source()
    cut = g.cut(1)
    CC.assert_cut_is_seed(cut, seed, 1)
    assert (cut.channels, cut.msgs, cut.n_channels, cut.tokens.size) == (8580, 14699, 19348, 2000)
    return g, seed, cut


def powerlaw_template(lanes=0):
    p, _, _ = T.powerlaw_drained()
    t = clg.GraphSim(fifo_slots=512)
    t.set_topology(p.tokens, p.src, p.dst, id_width=p.width())
    t.set_delay_hash(77)
    t.set_push_lanes(lanes)
    return t


@functools.lru_cache(maxsize=None)
def powerlaw_restored(lanes):
    """g.restore(1) after the continuation, under the template's configuration."""
    g, _, _ = powerlaw_cut()
    r = g.restore(1)
    r.set_limits(fifo_slots=512)
    r.set_delay_hash(77)
    r.set_push_lanes(lanes)
    return R.run_engine(r, RT.POWERLAW_OPS)


@pytest.mark.parametrize("lanes", [1, 4])
def test_several_check_tiles_unit_payloads(lanes):
    g, seed, cut = powerlaw_cut()
    assert cut.msg_tokens is not None and (cut.msg_tokens == 1).all()
    implicit = clg.SnapshotCut(1, cut.tokens, cut.channel, cut.count, None, cut.n_channels, cut.topology_key)
    template = powerlaw_template(lanes)
    want = powerlaw_restored(lanes)
    assert (want.status(), want.time(), want.counters()["push"]) == (0, 87, 53395)     # (the restore test's figures)
    runs = []
    for c in (cut, implicit):
        r = template.restore_cut(c)
        R.check_time0(r, seed, 1)
        assert r.seed_info["unit_payloads"] == 1 and r.seed_info == want.seed_info
        runs.append(R.run_engine(r, RT.POWERLAW_OPS))
        R.compare_engines(want, r)
    assert runs[0].device_bytes == runs[1].device_bytes                              # the payload buffer is dropped
    if lanes == 1:
        GC.compare(runs[1], R.oracle_equivalent(seed, ("hash", 77), RT.POWERLAW_OPS))


def test_nonunit_payloads_recorded_again():
    """223 entries of payloads 2..4; the restored run's own snapshot, started at once at the receiver
    of a seeded channel, records seeded messages again: the payload history is sized for the seed."""
    g, o = RT.regular_source()
    seed = R.seed_of_oracle(o, 0, *g.channels())
    cut = g.cut(0)
    CC.assert_cut_is_seed(cut, seed, 0)
    assert (cut.channels, cut.msgs) == (223, 226) and cut.info()["unit_payloads"] == 0
    src, dst = G.regular_graph(600, 8, 11)
    template = clg.GraphSim()
    template.set_topology(np.full(600, 100), src, dst, id_width=3)
    template.set_delay_hash(9)
    r = template.restore_cut(cut)
    R.check_time0(r, seed, 0)
    c = int(np.nonzero(seed.counts == 2)[0][0])                        # a channel seeded with two messages
    ops = [("snap", int(seed.dst[c])), ("tick", 3), ("snap", 3), ("drain",)]
    oe, _ = RT.against_both(r, seed, ("hash", 9), ops)
    _, off, vals = oe.collect_channels(0)
    assert oe.status == 0 and off[c + 1] - off[c] == 2
    assert vals[off[c]:off[c + 1]].tolist() == seed.vals[seed.off[c]:seed.off[c + 1]].tolist()
    other = g.restore(0)
    other.set_delay_hash(9)
    R.compare_engines(R.run_engine(other, ops), r)


def test_a_hand_made_cut_nearly_as_deep_as_the_largest_ring():
    """No source run exists: two nodes, channel 0 holding 32,760 messages of payloads 1..5 in a ring
    of 32,768 slots, written by hand.  Against the oracle equivalent."""
    k, slots, md = 32760, 32768, 40000
    vals = 1 + np.arange(k) % 5
    seed = R.Seed([7, 5], [0, k, k], vals, [0, 1], [1, 0], ["N0", "N1"])
    template = clg.GraphSim(fifo_slots=slots, max_drain_ticks=md)
    template.set_topology([1, 1], [0, 1], [1, 0], id_width=1)          # (the template's own tokens do not matter)
    template.set_delay_hash(3)
    cut = clg.SnapshotCut(42, [7, 5], [0], [k], vals, n_channels=2, topology_key=template.topology_key())
    assert cut == CC.cut_of_seed(seed, 42)
    r = template.restore_cut(cut)
    R.check_time0(r, seed, 42)
    assert r.seed_info["max_ch_msgs"] == k and r.seed_info["source_sid"] == 42
    ops = [("tick", 3), ("snap", 1), ("tick", 2), ("snap", 0), ("drain",)]
    R.run_engine(r, ops)
    oe = R.oracle_equivalent(seed, ("hash", 3), ops, max_drain=md)
    assert oe.status == 0 and oe.collect_channels(0)[2].size > k - 8
    GC.compare(r, oe)


def test_template_reuse_and_independence():
    top, events = "10nodes.top", "10nodes.events"
    g, o = RT.scenario(top, events)
    seeds = {sid: R.seed_of_oracle(o, sid, *g.channels()) for sid in (0, 4)}
    cuts = {sid: g.cut(sid) for sid in (0, 4)}
    ops = [("tick", 1), ("snap", 0), ("drain",)]
    template = GC.scenario_engine(top, events, SEED)                    # a template that has run a program
    before = template.device_bytes
    first_results = RT.results(template)
    made = {sid: template.restore_cut(cuts[sid]) for sid in (0, 4)}     # one template, two cuts
    twin = template.restore_cut(cuts[0])
    assert template.device_bytes == before and RT.results(template) == first_results    # the template is unchanged
    fresh = scenario_template(top)
    bare = fresh.restore_cut(cuts[0])
    # before its first run a restored graph holds the topology, less the template's token plane, and its
    # seed: the plane, (channel, count, offset) per entry and the payloads (10 of payload 10 on one channel)
    assert bare.device_bytes - fresh.device_bytes == (4 + 4 + 8) * 1 + 4 * 10
    template.__del__()                                                  # gone before any restored graph runs
    fresh.__del__()
    del template, fresh
    for sid, r in made.items():
        R.check_time0(r, seeds[sid], sid)
        R.run_engine(r, ops)
        GC.compare(r, R.oracle_equivalent(seeds[sid], ("go", SEED), ops))
        assert RT.results(r) == RT.results(R.run_engine(g.restore(sid), ops))
    r = made[0]
    first = RT.results(r)
    assert first == RT.results(R.run_engine(twin, ops)) == RT.results(R.run_engine(bare, ops))
    r.poison_outputs()
    r.rerun()                                                           # back to the seeded state
    assert RT.results(r) == first
    assert r.restore_time()[1] > 0 and r.seed_info == seeds[0].info(0)


def test_limits_as_in_restore():
    top = "10nodes.top"
    g, o = RT.scenario(top, "10nodes.events")
    ten, eight = g.cut(0), g.cut(4)                                     # 10 and 8 messages on one channel
    r = scenario_template(top, fifo_slots=8).restore_cut(ten)
    r.Tick(3)
    r.flush()
    assert r.status() == RT.FIFO_OVERFLOW and r.time() == 0
    seed = R.seed_of_oracle(o, 4, *g.channels())
    r = scenario_template(top, fifo_slots=8).restore_cut(eight)         # exactly the ring
    ops = [("tick", 2), ("snap", 5), ("drain",)]
    R.run_engine(r, ops)
    assert r.status() == 0
    GC.compare(r, R.oracle_equivalent(seed, ("go", SEED), ops))
    t = scenario_template(top)
    t.set_delay_schedule([1, 2, 3, 4, 0])                               # shorter than M
    r = t.restore_cut(ten)
    r.Tick(3)
    r.flush()
    assert r.status() == RT.DELAY_EXHAUSTED and r.time() == 0
    sched = [(3 * i + 1) % 5 for i in range(10)]                        # exactly M draws
    t = scenario_template(top)
    t.set_delay_schedule(sched)
    r = t.restore_cut(ten)
    ops = [("tick", 7)]
    R.run_engine(r, ops)
    seed = R.seed_of_oracle(o, 0, *g.channels())
    oe = R.oracle_equivalent(seed, ("schedule", sched), ops)
    assert oe.status == 0
    GC.compare(r, oe)
    assert r._L.cl_graph_set_device(r._h, 0) == cl.E_STATE
    assert r._L.cl_graph_part_begin(r._h, 0, r.num_nodes) == cl.E_STATE
    assert r._L.cl_graph_add_node(r._h, b"Z", 1) == cl.E_STATE          # the topology is frozen
    # a partitioned template is refused on the host, and cl_graph_restore still refuses a partitioned source
    part = clg.GraphSim()
    part.read_topology_file(os.path.join(TEST_DATA, top))
    assert part._L.cl_graph_part_begin(part._h, 0, part.num_nodes) == 0
    assert error_code(part.restore_cut, ten) == cl.E_STATE
    rc, out, _ = CC.raw_restore_cut(part, ten.tokens, ten.channel, ten.count, ten.msg_tokens)
    assert rc == cl.E_STATE and out is None
    assert part._L.cl_graph_part_snapshot(part._h, 3, None) == 0
    assert error_code(part.restore, 0) == cl.E_STATE
    sid = g.num_snapshots
    assert error_code(g.cut, sid) == cl.E_INVALID                       # an unknown snapshot
    p, ou, _ = T.powerlaw_undrained()
    assert T.mixed(ou)
    u = GC.engine_program(p)
    sid = [s for s in range(ou.num_snapshots) if not ou.complete(s)][0]
    assert error_code(u.cut, sid) == cl.E_NOT_COMPLETE


# ---- the check kernel --------------------------------------------------------------------------
class Arrays:
    """The valid 8,580-entry cut as four int32 arrays, copied per case."""

    def __init__(self, cut):
        self.tokens, self.channel, self.count, self.msgs = (np.array(a, dtype=np.int32) for a in
                                                            (cut.tokens, cut.channel, cut.count, cut.msg_tokens))

    def copy(self):
        c = object.__new__(Arrays)
        c.tokens, c.channel, c.count, c.msgs = self.tokens.copy(), self.channel.copy(), self.count.copy(), self.msgs.copy()
        return c


def refused(template, a, field, index, n_msgs=None):
    """The call must return E_INVALID with *out NULL and name field[index] and its value.  A handle
    that came back all the same is destroyed unflushed -- no seed kernel runs on it -- and the test
    stops."""
    rc, out, msg = CC.raw_restore_cut(template, a.tokens, a.channel, a.count, a.msgs, n_msgs)
    if out is not None:
        template._L.cl_graph_destroy(out)
        pytest.fail(f"a malformed cut was accepted ({field}[{index}])")
    assert rc == cl.E_INVALID, (rc, msg)
    if field == "n_msgs":
        assert "n_msgs" in msg and str(index) in msg, msg
    else:
        value = int({"tokens": a.tokens, "channel": a.channel, "count": a.count, "msg_tokens": a.msgs}[field][index])
        assert f"{field}[{index}] = {value} " in msg, msg
    return msg


def test_the_check_kernel_refuses_every_defect():
    g, seed, cut = powerlaw_cut()
    template = powerlaw_template()
    base = Arrays(cut)
    n, e, ne, m = base.tokens.size, cut.n_channels, base.channel.size, base.msgs.size
    assert (n, e, ne, m) == (2000, 19348, 8580, 14699) and int(base.count.sum()) == m
    last = ne - 1
    # the starts and ends of a lane's, a wave's, a workgroup's and a tile's share under any plausible geometry
    pos = [1, 63, 64, 255, 256, 2047, 2048, 4096, last]

    def one(field, index, value, report=None):
        a = base.copy()
        {"tokens": a.tokens, "channel": a.channel, "count": a.count, "msg_tokens": a.msgs}[field][index] = value
        return refused(template, a, field, index if report is None else report)

    for i in pos:
        one("channel", i, int(base.channel[i - 1]))                     # equal to its predecessor
        one("channel", i, int(base.channel[i - 1]) - 1)                 # a descending pair
    assert "outside" in one("channel", 0, -1)
    assert "outside" in one("channel", last, e)
    assert "ascend" in one("channel", 4096, int(base.channel[4095]))
    one("channel", 0, int(base.channel[1]), report=1)                   # channel[0] itself is fine: [1] does not ascend
    for i in [0] + pos[1:]:
        for bad in (0, -1, 32769):
            one("count", i, bad)
    for j in (0, 2047, 2048, m - 1):
        for bad in (-1, INT32_MIN):
            one("msg_tokens", j, bad)
    one("tokens", 0, -1)
    one("tokens", n - 1, -1)
    for d in (+1, -1):                                                  # n_msgs = the sum +- 1, arrays sized to match
        a = base.copy()
        a.msgs = np.ones(m + d, dtype=np.int32)
        msg = refused(template, a, "n_msgs", m + d, n_msgs=m + d)
        assert str(m) in msg
        a.msgs = None                                                   # and with implicit payloads
        refused(template, a, "n_msgs", m + d, n_msgs=m + d)

    # two defects together: the lowest rule in the order tokens, channel, count, msg_tokens, n_msgs; then the lowest index
    def two(first, second):
        a = base.copy()
        for field, index, value in (first, second):
            {"tokens": a.tokens, "channel": a.channel, "count": a.count, "msg_tokens": a.msgs}[field][index] = value
        refused(template, a, first[0], first[1])

    two(("tokens", 5, -1), ("channel", 0, -1))
    two(("tokens", 1999, -7), ("msg_tokens", 0, -1))
    two(("channel", 4096, int(base.channel[4095])), ("count", 1, 0))
    two(("count", 8000, 0), ("msg_tokens", 0, INT32_MIN))
    two(("count", 10, 0), ("count", 3000, 40000))
    two(("channel", 64, e), ("channel", 8579, -1))
    two(("msg_tokens", 2048, -1), ("msg_tokens", m - 1, -1))
    two(("tokens", 3, -1), ("tokens", 1024, -1))
    a = base.copy()                                                     # a bad payload and a bad total
    a.msgs = np.ones(m + 1, dtype=np.int32)
    a.msgs[m] = -1
    refused(template, a, "msg_tokens", m, n_msgs=m + 1)

    # after the whole series the same template restores the valid cut
    rc, out, _ = CC.raw_restore_cut(template, base.tokens, base.channel, base.count, base.msgs, sid=1)
    assert rc == 0 and out is not None
    r = clg.GraphSim._of_handle(template._L, C.c_void_p(out), 0)
    R.check_time0(r, seed, 1)
    R.compare_engines(powerlaw_restored(0), R.run_engine(r, RT.POWERLAW_OPS))
    R.compare_engines(powerlaw_restored(0), R.run_engine(template.restore_cut(cut), RT.POWERLAW_OPS))


# ---- a fresh process ---------------------------------------------------------------------------
def test_a_fresh_process_restores_from_a_saved_cut(tmp_path):
    g, o = RT.scenario("10nodes.top", "10nodes.events")
    cut = g.cut(0, topology=True)
    assert cut.has_topology and [i.decode() for i in cut.ids.tolist()] == g.node_ids()
    path, out = str(tmp_path / "cut.npz"), str(tmp_path / "results.json")
    cut.save(path)
    assert clg.SnapshotCut.load(path) == cut
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cutcheck.py")
    child = subprocess.run([sys.executable, script, path, out, str(SEED)], capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    with open(out) as f:
        got = json.load(f)
    want = CC.results_doc(R.run_engine(g.restore(0), CC.CONTINUATION))
    assert got == json.loads(json.dumps(want))
    assert got["status"] == 0 and len(got["ticks"]) == 2 and all(t >= 0 for t in got["ticks"])
    seed = R.seed_of_oracle(o, 0, *g.channels())
    oe = R.oracle_equivalent(seed, ("go", SEED), CC.CONTINUATION)
    assert (got["time"], got["node_ids"]) == (oe.time, oe.node_ids())
    assert got["node_tokens"] == [oe.node_tokens()[k] for k in oe.node_ids()]
    # the same in this process: the node-by-node template (ids N1..N10 are no zero-padded ranks)
    here = clg.GraphSim.from_cut(cut)
    here.set_delay_go_seed(SEED)
    assert CC.results_doc(R.run_engine(here, CC.CONTINUATION)) == want


def test_from_cut_builds_the_bulk_template():
    """Ids that are "N" + the zero-padded rank take set_topology; the result equals restore's."""
    g, seed, _ = powerlaw_cut()
    cut = g.cut(1, topology=True)
    assert cut.ids[0] == b"N0000" and cut.ids[-1] == b"N1999"
    r = clg.GraphSim.from_cut(cut, fifo_slots=512)
    r.set_delay_hash(77)
    assert r.node_ids() == g.node_ids()
    R.check_time0(r, seed, 1)
    R.compare_engines(powerlaw_restored(0), R.run_engine(r, RT.POWERLAW_OPS))
