"""GPU tests of GraphSim.restore (cl_graph_restore): a run that begins in a recorded cut, built
and seeded by kernels on the device.  With no synthetic traffic a restored graph must be
indistinguishable from the host route (restorecheck): the same topology with node tokens T' and the
recorded messages re-sent in (channel, position) order -- checked against the unchanged CPU oracle
and against the engine's own host route, all exact.  Shapes: fewer channels than one wave (the
reference scenarios, the empty seed included), several channel tiles with a ragged last one and
several tiles of seed entries (2000-node power-law, unit payloads, 14,699 messages over 8,580
entries: four full entry tiles and a ragged fifth), non-unit payloads over several tiles (600-node
regular graph), both push paths.  The figures asserted were produced on the CPU oracle."""
import functools

import numpy as np
import pytest

import graphcheck as GC
import graphgen as G
import oracle as O
import restorecheck as R
import tablecheck as T

pytestmark = pytest.mark.gpu

cl, clg = GC.cl, GC.clg
SEED = O.REFERENCE_SEED
FIFO_OVERFLOW, DELAY_EXHAUSTED = 3, 5      # include/clsnap.h CL_INST_*


@functools.lru_cache(maxsize=None)
def scenario(top, events):
    """(engine, oracle) of a reference scenario under the reference seed."""
    g = GC.scenario_engine(top, events, SEED)
    o = GC.scenario_oracle(top, events, SEED)
    assert g.status() == o.status == 0
    return g, o


def against_both(r, seed, delay, ops, fifo_slots=16, lanes=0):
    """Runs the continuation on r and checks it against the oracle equivalent and the engine's host
    route; returns (oracle equivalent, host route)."""
    R.run_engine(r, ops)
    o = R.oracle_equivalent(seed, delay, ops)
    GC.compare(r, o)
    b = R.engine_equivalent(seed, delay, ops, fifo_slots=fifo_slots, lanes=lanes)
    R.compare_engines(r, b)
    return o, b


def first_steps(src_graph, sid, seed, delay, fifo_slots=16, config=None):
    """Node tokens after each of the first 6 single ticks: a fresh restore against a fresh host
    route.  Every seeded receiveTime decides the tick of a delivery."""
    r = src_graph.restore(sid)
    if config:
        config(r)
    b = R.engine_equivalent(seed, delay, run=False, fifo_slots=fifo_slots)
    np.testing.assert_array_equal(R.step_tokens(r), R.step_tokens(b))


def a_send(seed):
    """A host send the cut allows: 1..3 tokens on the first channel whose sender holds some."""
    c = int(np.nonzero(seed.T[seed.src] > 0)[0][0])
    return ("send", int(seed.src[c]), int(seed.dst[c]), int(min(3, seed.T[seed.src[c]])))


SCENARIOS = [
    # top, events, sid, M, payloads, (src rank, dest rank) of the one seeded channel
    ("10nodes.top", "10nodes.events", 0, 10, [10] * 10, (1, 0)),
    ("10nodes.top", "10nodes.events", 4, 8, [10] * 8, (4, 5)),
    ("10nodes.top", "10nodes.events", 7, 5, [10] * 5, (7, 8)),
    ("8nodes.top", "8nodes-concurrent-snapshots.events", 2, 1, [4], (3, 4)),
    ("8nodes.top", "8nodes-concurrent-snapshots.events", 4, 0, [], None),
    ("3nodes.top", "3nodes-bidirectional-messages.events", 0, 3, [3, 2, 1], (0, 1)),
]


@pytest.mark.parametrize("top,events,sid,m,payloads,channel", SCENARIOS)
def test_reference_scenarios(top, events, sid, m, payloads, channel):
    g, o = scenario(top, events)
    seed = R.seed_of_oracle(o, sid, *g.channels())
    assert seed.ids == g.node_ids()
    assert seed.msgs == m and seed.vals.tolist() == payloads and seed.channels == (1 if m else 0)
    if channel:
        c = int(np.nonzero(seed.counts)[0][0])
        assert (seed.src[c], seed.dst[c]) == channel
    r = g.restore(sid)
    R.check_time0(r, seed, sid)
    row = g.snapshot_table(sid, sid + 1).rows[0]
    info = r.seed_info
    assert (info["channels"], info["msgs"], info["tokens"], info["max_ch_msgs"], info["node_tokens"]) == \
        tuple(int(row[f]) for f in ("rec_channels", "rec_msgs", "rec_tokens", "max_ch_msgs", "node_tokens"))
    build_ms, seed_ms = r.restore_time()
    assert build_ms > 0 and seed_ms >= 0 and (seed_ms > 0 or m == 0)
    n = g.num_nodes
    ops = [("snap", n // 2), ("tick", 2), a_send(seed), ("snap", 0), ("tick", 1), ("drain",)]
    against_both(r, seed, ("go", SEED), ops)
    assert r.num_snapshots == 2 and r.checksums()["completed"] == 2
    first_steps(g, sid, seed, ("go", SEED))


@pytest.mark.parametrize("sid,rank,recorded,ctick", [(0, 0, 10, 32), (7, 8, 5, 36)])
def test_seeded_messages_are_recorded_again(sid, rank, recorded, ctick):
    """The restored run's own snapshot, started at the seeded channel's receiver after one tick,
    records every seeded message (payload 10): the payload history must be sized for the seed."""
    g, o = scenario("10nodes.top", "10nodes.events")
    seed = R.seed_of_oracle(o, sid, *g.channels())
    c = int(np.nonzero(seed.counts)[0][0])
    assert seed.dst[c] == rank
    r = g.restore(sid)
    r.set_delay_go_seed(SEED + 1)
    ops = [("tick", 1), ("snap", rank), ("drain",)]
    oe, _ = against_both(r, seed, ("go", SEED + 1), ops)
    assert oe.status == 0 and oe.completion_tick(0) == ctick
    assert oe.collect_channels(0)[2].tolist() == [10] * recorded
    _, off, vals = r.collect_arrays(0)
    assert vals.tolist() == [10] * recorded and off[c + 1] - off[c] == recorded
    first_steps(g, sid, seed, ("go", SEED + 1), config=lambda x: x.set_delay_go_seed(SEED + 1))


@functools.lru_cache(maxsize=None)
def powerlaw_source():
    """(engine, seed of sid 1) of the drained power-law run: 19,348 channels, unit payloads."""
    p, o, _ = T.powerlaw_drained()
    g = GC.engine_program(p, drain=True)
    assert g.status() == o.status == 0
    seed = R.seed_of_oracle(o, 1, p.src, p.dst)
    assert g.num_channels == 19348 and (seed.channels, seed.msgs, int(seed.counts.max())) == (8580, 14699, 8)
    assert (seed.vals == 1).all()
    return g, seed


POWERLAW_OPS = [("snap", 5), ("tick", 2), ("snap", 1500), ("tick", 8), ("drain",)]


@pytest.mark.parametrize("lanes", [1, 4])
def test_several_channel_tiles_unit_payloads(lanes):
    g, seed = powerlaw_source()
    r = g.restore(1)
    r.set_delay_hash(77)
    r.set_push_lanes(lanes)
    R.check_time0(r, seed, 1)
    oe, _ = against_both(r, seed, ("hash", 77), POWERLAW_OPS, fifo_slots=512, lanes=lanes)
    assert (oe.status, oe.time) == (0, 87)
    assert [oe.completion_tick(s) for s in range(2)] == [80, 81]
    assert [oe.collect_channels(s)[2].size for s in range(2)] == [3918, 1394]
    assert oe.counters()["push"] == r.counters()["push"] == 53395
    if lanes != 1:
        return
    first_steps(g, 1, seed, ("hash", 77), fifo_slots=512, config=lambda x: x.set_delay_hash(77))
    # a snapshot of a restored run restores too
    seed2 = R.seed_of_oracle(oe, 0, seed.src, seed.dst)
    assert (seed2.channels, seed2.msgs) == (2193, 3918)
    r2 = r.restore(0)
    R.check_time0(r2, seed2, 0)
    against_both(r2, seed2, ("hash", 77), [("snap", 9), ("tick", 3), ("drain",)], fifo_slots=512)
    assert r2.num_snapshots == 1 and r2.checksums()["completed"] == 1


@functools.lru_cache(maxsize=None)
def regular_source():
    """A 600-node regular graph (4,760 channels) under hash seed 5: 12 steps in which every node v
    sends 2 + (v + k) % 3 tokens on out-link (v + k) % outdeg, a snapshot at rank 7 at step 3,
    then the drain.  (engine, oracle)."""
    n = 600
    src, dst = G.regular_graph(n, 8, 11)
    g = clg.GraphSim()
    g.set_topology(np.full(n, 100), src, dst, id_width=3)
    g.set_delay_hash(5)
    o = O.OracleSim()
    o.use_counter_hash(5)
    assert o.build_graph(np.full(n, 100), src, dst, 3) == 0
    csrc, cdst = g.channels()
    assert csrc.size == 4760
    ids = o.node_ids()
    out_off = np.searchsorted(csrc, np.arange(n + 1))
    for k in range(12):
        for v in range(n):
            c = out_off[v] + (v + k) % (out_off[v + 1] - out_off[v])
            g.send_tokens_rank(v, int(cdst[c]), 2 + (v + k) % 3)
            assert o.send_tokens(ids[v], ids[cdst[c]], 2 + (v + k) % 3) == 0
        if k == 3:
            g.start_snapshot_rank(7)
            o.start_snapshot(ids[7])
        g.Tick(1)
        o.tick()
    g.drain()
    o.drain()
    g.flush()
    return g, o


def test_several_tiles_nonunit_payloads():
    g, o = regular_source()
    GC.compare(g, o)
    seed = R.seed_of_oracle(o, 0, *g.channels())
    assert (seed.channels, seed.msgs, int(seed.counts.max())) == (223, 226, 2)
    assert (int(seed.vals.min()), int(seed.vals.max())) == (2, 4)
    r = g.restore(0)
    r.set_delay_hash(9)
    R.check_time0(r, seed, 0)
    oe, _ = against_both(r, seed, ("hash", 9), [("snap", 3), ("tick", 3), ("drain",)])
    assert (oe.status, oe.time, oe.counters()["push"]) == (0, 32, 4986)
    assert sum(oe.node_tokens().values()) == int(r.node_tokens_array().sum()) == 60000
    first_steps(g, 0, seed, ("hash", 9), config=lambda x: x.set_delay_hash(9))


def test_a_channel_nearly_as_deep_as_the_largest_ring():
    """One channel seeded with 32,760 messages of payloads 1..5 in a ring of 32,768 slots (the
    restored run's own markers need the rest): the seed kernel's message-parallel path over 128
    workgroups on one entry, the count field of the hq word near its top, and a payload history
    sized by the seed.  Two nodes; against the oracle equivalent."""
    k, slots, md = 32760, 32768, 40000
    tokens, src, dst = [100000, 5], [0, 1], [1, 0]
    g = clg.GraphSim(fifo_slots=slots, max_drain_ticks=md)
    g.set_topology(tokens, src, dst, id_width=1)
    g.set_delay_hash(3)
    o = O.OracleSim()
    o.use_counter_hash(3)
    assert o.build_graph(tokens, src, dst, 1) == 0
    ids = o.node_ids()
    for i in range(k):
        g.send_tokens_rank(0, 1, 1 + i % 5)
        assert o.send_tokens(ids[0], ids[1], 1 + i % 5) == 0
    g.start_snapshot_rank(1)
    o.start_snapshot(ids[1])
    g.drain()
    o.drain(md)
    assert g.status() == o.status == 0 and g.snapshot_tick(0) == o.completion_tick(0) > k
    seed = R.seed_of_oracle(o, 0, *g.channels())
    assert seed.counts.tolist() == [k, 0] and seed.vals.tolist() == [1 + i % 5 for i in range(k)]
    r = g.restore(0)
    R.check_time0(r, seed, 0)
    ops = [("tick", 3), ("snap", 1), ("tick", 2), ("snap", 0), ("drain",)]
    R.run_engine(r, ops)
    oe = R.oracle_equivalent(seed, ("hash", 3), ops, max_drain=md)
    assert oe.status == 0 and oe.collect_channels(0)[2].size > k - 8
    GC.compare(r, oe)


def test_the_seed_leaves_no_trace_and_the_replay_starts_from_the_cut():
    """The Logger of a restored run is the host route's without its M SENT_TOKEN records of the
    re-sent messages (the first records of epoch 0), nodeTokens included."""
    g, o = scenario("10nodes.top", "10nodes.events")
    seed = R.seed_of_oracle(o, 0, *g.channels())
    ops = [("tick", 1), ("snap", 0), a_send(seed), ("tick", 4), ("drain",)]
    r = g.restore(0)
    r.trace_enable(1 << 12)
    R.run_engine(r, ops)
    log = R.oracle_equivalent(seed, ("go", SEED), ops, log=True).log()
    assert [x[1] for x in log[:seed.msgs]] == [0] * seed.msgs and len(log) > seed.msgs     # LOG_SENT_TOKEN
    got = r.trace()
    assert got == log[seed.msgs:]
    assert got[0][0] == 1 and not any(x[0] == 0 for x in got)        # nothing is logged at time 0


def results(g):
    ns = g.num_snapshots
    return (g.status(), g.time(), g.node_tokens_array().tobytes(), g.counters(), g.checksums(),
            [g.snapshot_tick(s) for s in range(ns)], g.snapshot_table().rows.tobytes(),
            [a.tobytes() for s in range(ns) if g.snapshot_tick(s) >= 0 for a in g.collect_arrays(s)])


def test_independence_and_replay():
    top, events = "10nodes.top", "10nodes.events"
    _, o = scenario(top, events)
    ops = [("tick", 1), ("snap", 0), ("drain",)]
    src = GC.scenario_engine(top, events, SEED)       # (a source of this test's own: it is destroyed)
    seed = R.seed_of_oracle(o, 0, *src.channels())
    r = src.restore(0)
    other = src.restore(0)
    src.rerun()                                       # a rerun of the source between restore and first flush
    src.flush()
    R.run_engine(other, ops)
    src.__del__()                                     # the source is gone before r first runs
    del src
    R.run_engine(r, ops)
    GC.compare(r, R.oracle_equivalent(seed, ("go", SEED), ops))
    first = results(r)
    assert first == results(other)
    r.poison_outputs()
    r.rerun()                                         # back to the seeded state, not an empty one
    assert results(r) == first
    assert r.restore_time()[1] > 0 and r.seed_info == seed.info(0)


def test_traffic_on_a_restored_graph():
    """With traffic the seed still comes first; the host-route equivalence does not hold (step-0
    traffic sees T, not T'), so invariants only."""
    g, seed = powerlaw_source()
    r = g.restore(1)
    r.set_traffic(99, 1 << 30, 30)
    for k in range(30):
        if k == 4:
            r.start_snapshot_rank(11)
        r.Tick(1)
    r.drain()
    r.flush()
    s = r.checksums()
    assert r.status() == 0 and s["ok"] == 1 and s["completed"] == 1
    assert s["cut_residual"] == s["final_residual"] == 0
    assert int(r.node_tokens_array().sum()) + s["in_flight"] == 200000
    assert r.counters()["push"] > seed.msgs
    first = results(r)
    r.poison_outputs()
    r.rerun()
    assert results(r) == first


def test_limits_and_errors():
    p, o, _ = T.powerlaw_undrained()
    assert T.mixed(o)
    g = GC.engine_program(p)
    sid = [s for s in range(o.num_snapshots) if not o.complete(s)][0]
    with pytest.raises(cl.ClSnapError) as e:
        g.restore(sid)
    assert e.value.code == cl.E_NOT_COMPLETE
    part = clg.GraphSim()
    part.set_topology(p.tokens, p.src, p.dst, id_width=p.width())
    assert part._L.cl_graph_part_begin(part._h, 0, part.num_nodes) == 0
    assert part._L.cl_graph_part_snapshot(part._h, 3, None) == 0
    with pytest.raises(cl.ClSnapError) as e:
        part.restore(0)
    assert e.value.code == cl.E_STATE

    g, o = scenario("10nodes.top", "10nodes.events")
    r = g.restore(0)                                  # 10 messages on one channel
    r.set_limits(fifo_slots=8)
    r.Tick(3)
    r.flush()
    assert r.status() == FIFO_OVERFLOW and r.time() == 0
    seed = R.seed_of_oracle(o, 4, *g.channels())      # 8 messages: exactly the ring
    r = g.restore(4)
    r.set_limits(fifo_slots=8)
    ops = [("tick", 2), ("snap", 5), ("drain",)]
    R.run_engine(r, ops)
    assert r.status() == 0
    GC.compare(r, R.oracle_equivalent(seed, ("go", SEED), ops))
    r = g.restore(0)
    r.set_delay_schedule([1, 2, 3, 4, 0])
    r.Tick(3)
    r.flush()
    assert r.status() == DELAY_EXHAUSTED and r.time() == 0
    r = g.restore(0)
    build_ms, seed_ms = r.restore_time()              # built, not yet run
    assert build_ms > 0 and seed_ms == 0
    assert r._L.cl_graph_set_device(r._h, 0) == cl.E_STATE
    assert r._L.cl_graph_part_begin(r._h, 0, r.num_nodes) == cl.E_STATE
    assert r._L.cl_graph_add_node(r._h, b"Z", 1) == cl.E_STATE          # the topology is frozen
    assert r.device_bytes > 0


def test_a_schedule_of_exactly_the_seed_and_device_bytes():
    """A schedule as long as the seed (and the run's further draws) is enough; the seed's buffers
    are counted."""
    g, o = scenario("10nodes.top", "10nodes.events")
    seed = R.seed_of_oracle(o, 0, *g.channels())
    sched = [(3 * i + 1) % 5 for i in range(10)]
    r = g.restore(0)
    r.set_delay_schedule(sched)
    ops = [("tick", 7)]
    R.run_engine(r, ops)
    oe = R.oracle_equivalent(seed, ("schedule", sched), ops)
    assert oe.status == 0
    GC.compare(r, oe)
    plain = R.engine_equivalent(seed, ("schedule", sched), ops)
    # r holds no initial-token plane of its own: the seed's, plus entries, offsets and payloads
    assert g.num_nodes == 10 and r.device_bytes - plain.device_bytes == (4 + 4 + 8) * 1 + 4 * 10
