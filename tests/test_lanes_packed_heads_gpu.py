"""The lanes kernels' paired senders (cl_lanes.h Pairs): two senders' out-link head words live in
the halves of one register and phase A scans both with packed 16-bit instructions.

Every case forces the lanes engine and the program kernels on, flushes (generic kernels), reads
every result, poisons the output planes, reruns (program-specialized kernels, asserted; the
generic ones again where the program is over their cap) and
compares array for array: status, time, counters, per-instance hashes, completion ticks and
collect_snapshot_packed of every snapshot; final node tokens and CollectSnapshot on a sample.  The
oracle pins status, time, hashes, counters and the sample.  Each case runs at 4096 + 17 instances
(replays through the slot map, block-major records, a ragged last block) and at 64 + 5 (identity
order, instance-major records).  Before the GPU runs, the oracle alone shows that more than half
the instances end OK and that the case's condition occurs.

* an odd node count: a sender whose partner half is inert, and nodes without out-links;
* a pair of unequal out-degrees with traffic on the longer sender's last link, and ticks in which
  both halves of the pair deliver, only the low one, only the high one;
* a channel at 127 queued packets (LDS ring and HBM spill ring, on the spill kernels) while its
  pair partner pushes and pops, once in the low and once in the high half: no carry between the
  halves, the refill and FULL tests read the right half;
* a program flushed in two launches on either engine in turn: the state image's link words
  round-trip through the packed form.

A wrap of the 9-bit head counter needs no test: a launch pops a channel at most 240 times
(cl_jit.cpp lanes_fit admits 240 draws), and the state image stores the head as a ring slot, so a
resumed launch starts its counter below the ring size again.

Reference: sim.go:71-95 (Tick), queue.go:6-28, node.go:97-109 (SendToNeighbors),
test_common.go:123-137 (drain).
"""
import numpy as np
import pytest

import oracle as O
import packedcheck as P
from enginecheck import cl, compare_instance, oracle_run

pytestmark = pytest.mark.gpu

LANES = cl.ChandyLamportSim.ENGINE_LANES
NODES = cl.ChandyLamportSim.ENGINE_NODES
ON = cl.ChandyLamportSim.PROGRAM_ON
SIZES = [4096 + 17, 64 + 5]
# LDS ring slots per channel where nothing is to spill: above every channel's packet count in
# those programs (at most 6: three sends and three markers), so no instance spills, the probe
# splits nothing off and the small batch replays in identity order
SLOTS = 8
RECV = (2, 3)   # CL_LOG_RECV_TOKEN, CL_LOG_RECV_MARKER


def _rows(n, width, seed):
    """Delay rows: an instance draws either 0 throughout or uniformly from 0..4.  The two kinds end
    their drains far enough apart that ordering the large batch by length saves the planner's 8 %
    of wave-ticks (cl_plan.cpp plan_order), so its replays go through the slot map."""
    rng = np.random.default_rng(seed)
    hi = rng.choice([1, 5], size=(n, 1))
    return (rng.integers(0, 5, size=(n, width)) % hi).astype(np.uint8)


def _sample(n):
    return tuple(i for i in tuple(range(0, 96)) + (777, 2048, 4095, 4096, 4112) if i < n)


def _sim(top, n, sched, slots=SLOTS, engine=LANES):
    sim = cl.ChandyLamportSim(n, fifo_lds_slots=slots)
    sim.set_exec_engine(engine)
    sim.set_program_kernels(ON)
    sim.read_topology_text(top)
    sim.set_delay_schedule(sched)
    return sim


def _outputs(sim):
    out = [sim.status(), sim.time(), sim.checksums(), sim.counters(only_ok=False), sim.counters(only_ok=True),
           sim.instance_hashes()]
    for sid in range(sim.num_snapshots):
        out.append(sim.snapshot_ticks(sid))
        out.extend(sim.collect_snapshot_packed(sid))
    out.append([sim.node_tokens(i) for i in _sample(sim.n_instances)])
    return out


def _same(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, (dict, list)):
            assert x == y, (what, k)
        else:
            assert np.array_equal(x, y), (what, k)


def _oracle_batch(top, events, n, sched):
    """The oracle's batch; more than half of it must end OK."""
    res = O.run_batch(top, events, n, sched=sched, draws=sched.shape[1], threads=8)
    assert (res[1] == O.OK).sum() > n // 2
    return res


def _logs(top, events, sched, count):
    """Logger records of the first `count` instances: (tick, kind, node, other, data, tokens)."""
    logs = []
    for i in range(count):
        ref = O.OracleSim()
        ref.use_schedule(sched[i])
        ref.log_enable(True)
        assert ref.read_topology_text(top) == 0 and ref.read_events_text(events) >= 0
        logs.append(ref.log())
    return logs


def _replay(sim, n, want_spec=True):
    """Generic flush, then a poisoned rerun on the program kernels (want_spec=False: a program
    over their cap, the generic kernels again): the rerun's outputs."""
    sim.flush()
    assert sim.exec_engine() == LANES and not sim.exec_program_kernels()   # a first launch is generic
    gen = _outputs(sim)
    sim.poison_outputs()
    sim.rerun()
    sim.synchronize()
    assert sim.exec_engine() == LANES and sim.exec_program_kernels() == want_spec
    big = n >= 4096
    assert sim.mapped_replays() == big and sim.records_blocked() == big
    spec = _outputs(sim)
    _same(spec, gen, "program-specialized rerun vs generic flush")
    return spec


def _against_oracle(sim, got, orc, top, events, sched):
    _, st, ticks, cnt, hashes = orc
    ok = st == 0
    status, times = got[0], got[1]
    assert np.array_equal(status, st)
    assert np.array_equal(times[ok], ticks[ok])
    assert np.array_equal(got[5][ok], hashes[ok])
    c = got[4]
    assert c["recorded"] == cnt[ok, 4].sum() and c["completed"] == cnt[ok, 6].sum()
    if ok.all():
        c = got[3]
        assert (c["push"], c["peek"], c["pop_tok"], c["pop_mk"]) == tuple(cnt[:, k].sum() for k in range(4))
    for i in _sample(len(st)):
        compare_instance(sim, i, oracle_run(top, events, schedule=sched[i]), status=status, times=times)


def _check(top, events, n, sched, orc, slots=SLOTS, want_spec=True):
    sim = _sim(top, n, sched, slots)
    sim.read_events_text(events)
    got = _replay(sim, n, want_spec)
    _against_oracle(sim, got, orc, top, events, sched)
    return sim, got


def _deliveries(log, sender):
    """The ticks in which `sender` (a rank) delivered a packet."""
    return {r[0] for r in log if r[1] in RECV and r[3] == sender}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", ["all_senders", "two_sinks"])
def test_odd_node_count(case, n):
    """Five nodes, three pairs.  all_senders: E, alone in the last pair, scans and delivers beside
    an inert half.  two_sinks: C's partner K has no out-link, and the last pair (L alone) has no
    link slot."""
    top, events = (P.ODD_TOP, P.ODD_EVENTS) if case == "all_senders" else (P.SINKS_TOP, P.SINKS_EVENTS)
    sched = _rows(n, 48, 31)
    orc = _oracle_batch(top, events, n, sched)
    lone = 4 if case == "all_senders" else 2   # E; C
    assert all(_deliveries(log, lone) for log in _logs(top, events, sched, 16))
    _check(top, events, n, sched, orc)


@pytest.mark.parametrize("n", SIZES)
def test_pair_of_unequal_out_degrees(n):
    """I (3 links) and X (2) share a pair; Y and Z (1 each) the other.  I -> Z, the slot X has no
    link in, carries three sends and a marker.  Over the batch there are ticks in which both I and
    X deliver, only I, and only X."""
    sched = _rows(n, 48, 32)
    orc = _oracle_batch(P.T4_TOP, P.T4_EVENTS, n, sched)
    both = low = high = last = 0
    for log in _logs(P.T4_TOP, P.T4_EVENTS, sched, 64):
        i, x = _deliveries(log, 0), _deliveries(log, 1)
        both += len(i & x)
        low += len(i - x)
        high += len(x - i)
        last += sum(1 for r in log if r[1] in RECV and r[3] == 0 and r[2] == 3)   # I -> Z
    assert both and low and high and last
    _check(P.T4_TOP, P.T4_EVENTS, n, sched, orc)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("deep,other", [("P", "Q"), ("Q", "P")], ids=["low_half", "high_half"])
def test_channel_at_127_packets_beside_its_partner(deep, other, n):
    """P -> Q and Q -> P are the two halves of one head word.  One of them is driven to 127 queued
    packets, 4 in the LDS ring and 123 in the HBM spill ring, and the partner pushes while that
    count stands; then both pop for 150 ticks, the deep one refilling its ring from the spill ring at
    every pop.  Every instance spills (replay_split), so the replay runs the spill kernel: the
    generic one, the program's 130 host ops are over the cap of the specialized kernels."""
    events = P.deep_events(deep, other)
    sched = _rows(n, 136, 33 + (deep == "Q"))
    orc = _oracle_batch(P.DEEP_TOP, events, n, sched)
    # the oracle at the point where the host ops end: 127 packets on the deep channel, 1 beside it
    ref = O.OracleSim()
    ref.use_schedule(sched[0])
    assert ref.read_topology_text(P.DEEP_TOP) == 0
    ref.send_tokens(other, deep, 2)
    ref.send_tokens(other, deep, 3)
    ref.tick()
    ref.tick()
    ref.start_snapshot(deep)
    for _ in range(126):
        ref.send_tokens(deep, other, 1)
    ref.send_tokens(other, deep, 5)
    depths = sorted(ref.queue_depths().tolist())
    assert depths[-1] == 127 and 1 <= depths[-2] <= 3
    sim, got = _check(P.DEEP_TOP, events, n, sched, orc, slots=4, want_spec=False)
    spilled, _ = sim.replay_split()
    assert spilled == n
    assert (got[0] == O.OK).all() and (got[1] >= 150).all()


def _feed(sim, text):
    for ln in text.strip().split("\n"):
        f = ln.split()
        if f[0] == "send":
            sim.ProcessEvent(cl.PassTokenEvent(f[1], f[2], int(f[3])))
        elif f[0] == "snapshot":
            sim.ProcessEvent(cl.SnapshotEvent(f[1]))
        else:
            sim.Tick(int(f[1]) if len(f) > 1 else 1)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("engines", [(LANES, LANES), (LANES, NODES), (NODES, LANES)],
                         ids=["lanes_lanes", "lanes_nodes", "nodes_lanes"])
def test_two_launches_round_trip_the_link_words(engines, n):
    """The unequal-degree program flushed where packets are in flight on both halves of (I,X) and
    on I -> Z, then finished by a second launch: the first launch's state image carries every
    head word as a link word, the second unpacks it again -- lanes to lanes, lanes to the
    node-parallel kernel and back the other way.  Equal to one launch (itself checked against its
    replay and the oracle)."""
    sched = _rows(n, 48, 32)
    orc = _oracle_batch(P.T4_TOP, P.T4_EVENTS, n, sched)
    # packets in flight at the cut, in the oracle: on I's and X's links, I -> Z among them
    ref = O.OracleSim()
    ref.use_schedule(sched[0])
    assert ref.read_topology_text(P.T4_TOP) == 0
    for ln in P.T4_PARTS[0].strip().split("\n"):
        f = ln.split()
        if f[0] == "send":
            ref.send_tokens(f[1], f[2], int(f[3]))
        elif f[0] == "snapshot":
            ref.start_snapshot(f[1])
        else:
            for _ in range(int(f[1])):
                ref.tick()
    depths = ref.queue_depths()   # channels by (src rank, dest rank): I X, I Y, I Z, X Y, X Z, Y I, Z I
    assert depths[:3].all() and depths[3:5].any()
    one, got = _check(P.T4_TOP, P.T4_EVENTS, n, sched, orc)
    inc = _sim(P.T4_TOP, n, sched, engine=engines[0])
    _feed(inc, P.T4_PARTS[0])
    inc.flush()
    assert inc.exec_engine() == engines[0]
    inc.set_exec_engine(engines[1])
    _feed(inc, P.T4_PARTS[1])
    inc.drain()
    inc.flush()
    assert inc.exec_engine() == engines[1]
    _same(_outputs(inc), got, "two launches vs one")
