"""Helpers of the block-major, ragged-batch tests (test_blocked_ragged_host.py, test_blocked_ragged_gpu.py).

A replay through the slot map writes the snapshot records block-major by slot; plan_order() maps
whenever it sorts the clean instances by length (4096 instances and more) *or* splits the batch into
a spill-free and a spill-capable half (cl_plan.cpp: mapped = sort || split_slot > 0).  A split
needs one spilled instance, a specialized layout and one wave's worth of clean instances, so a small
C3 batch with 4 LDS ring slots per channel already replays through the map.

spill_prediction() is the oracle's side of that: per instance, the most packets any channel held at
once.  It is a prediction, not the engines' spill test (they pop a tick's channels before they push);
blocked_ragged_sim() asserts the regime on the device.
"""
import importlib

import numpy as np

import oracle as O
from depthcheck import EXTRA_TICKS, parse_events
from snapcheck import read_text

cl = importlib.import_module("chandy-lamport-distributed-snapshot-algorithm_amd")

AUTO, NODES, LANES = (cl.ChandyLamportSim.ENGINE_AUTO, cl.ChandyLamportSim.ENGINE_NODES,
                      cl.ChandyLamportSim.ENGINE_LANES)
C3_TOP, C3_EVENTS = "8nodes.top", "8nodes-concurrent-snapshots.events"
SLOTS = 4                               # fifo_lds_slots of every small case
SMALL_SIZES = (63, 65, 130, 200, 257)   # none a multiple of 64; 63, 65 and 257 no multiple of 8
N_SORT = 4096 + 37                      # a true length sort (kMapMinInstances = 4096) and a ragged last block

# A ring of 17 nodes, max in-degree 1: records of 2 words, 34 record words -- more than a staging
# chunk, so the statistics stage two chunks of whole nodes, 16 nodes and then R16 alone (rows of 2
# words at the odd pitch 3), and the other readers read the plane word by word.  R00 -> R01 holds up
# to 6 packets; snapshot 0 starts at R16 while R15 -> R16 carries traffic, so R16's record varies.
RING17_TOP = ("17\n" + "".join(f"R{v:02d} 8\n" for v in range(17))
              + "".join(f"R{v:02d} R{(v + 1) % 17:02d}\n" for v in range(17)))
RING17_EVENTS = ("send R00 R01 1\nsend R00 R01 2\nsend R00 R01 1\nsend R15 R16 3\ntick 2\nsend R00 R01 1\nsnapshot R16\n"
                 "send R15 R16 1\ntick 1\nsend R03 R04 1\nsend R16 R00 2\nsnapshot R00\ntick 2\n")
N_RING17 = 130


def text(x):
    return x if "\n" in x else read_text(x)


# C3's events, then 6 ticks, to be run without the drain (test_iset_gpu's cross-sid scenario)
UNDRAINED_EVENTS = read_text(C3_EVENTS).rstrip("\n") + "\ntick 6\n"


class Prediction:
    """status[n] (the oracle's), peak[n]: the most packets one channel of the instance held at once,
    read after every event and every tick through the drain; time[n]: the oracle time at the end."""

    def __init__(self, status, peak, time, slots):
        self.status, self.peak, self.time, self.slots = status, peak, time, slots

    def spillers(self, n=None):
        """The instances predicted to need more than `slots` ring slots on some channel."""
        return np.flatnonzero(self.peak[:n] > self.slots)


def spill_prediction(top, events, n, slots, seed_base=O.REFERENCE_SEED, max_drain=O.MAX_DRAIN_TICKS, drain=True):
    """The oracle walk: instance i runs `events` on seed seed_base + i, one event and one tick at a
    time, and -- `drain` -- ends like readEventsFile (ticks until every started snapshot completed,
    then maxDelay + 1 more).  An instance that leaves status OK stops there, as the engines freeze it."""
    top, evs = text(top), parse_events(text(events))
    status = np.zeros(n, dtype=np.int64)
    peak = np.zeros(n, dtype=np.int64)
    time = np.zeros(n, dtype=np.int64)
    for i in range(n):
        ref = O.OracleSim()
        ref.seed_go(seed_base + i)
        assert ref.read_topology_text(top) == 0
        deepest = 0

        def look():
            nonlocal deepest
            deepest = max(deepest, int(ref.queue_depths().max()))
            return ref.status == O.OK

        def run():
            for ev in evs:
                if ev[0] == "send":
                    ref.send_tokens(ev[1], ev[2], ev[3])
                elif ev[0] == "snapshot":
                    ref.start_snapshot(ev[1])
                else:
                    for _ in range(ev[1]):
                        ref.tick()
                        if not look():
                            return
                if not look():
                    return
            if not drain:
                return
            waited = 0
            while not all(ref.complete(s) for s in range(ref.num_snapshots)):
                assert waited < max_drain, "the drain would hang"
                ref.tick()
                waited += 1
                if not look():
                    return
            for _ in range(EXTRA_TICKS):
                ref.tick()
                look()

        run()
        status[i], peak[i], time[i] = ref.status, deepest, ref.time
    return Prediction(status, peak, time, slots)


def undrained_refs(top, events, n, seed_base=O.REFERENCE_SEED):
    """One OracleSim per instance that ran `events` event by event with no drain at the end, so
    that late snapshots stay incomplete in some instances (selectcheck.from_refs makes rows of them)."""
    top, evs = text(top), parse_events(text(events))
    refs = []
    for i in range(n):
        ref = O.OracleSim()
        ref.seed_go(seed_base + i)
        assert ref.read_topology_text(top) == 0
        for ev in evs:
            if ev[0] == "send":
                ref.send_tokens(ev[1], ev[2], ev[3])
            elif ev[0] == "snapshot":
                ref.start_snapshot(ev[1])
            else:
                for _ in range(ev[1]):
                    ref.tick()
        refs.append(ref)
    return refs


def build_sim(top, events, n, engine, fifo_lds_slots=None, drain=True):
    """A sim with the program loaded and nothing run; drain=False: the events one by one, without
    readEventsFile's drain at the end."""
    sim = cl.ChandyLamportSim(n, fifo_lds_slots=fifo_lds_slots)
    sim.set_exec_engine(engine)
    sim.read_topology_text(text(top))
    if drain:
        sim.read_events_text(text(events))
        return sim
    for ev in parse_events(text(events)):
        if ev[0] == "send":
            sim.ProcessEvent(cl.PassTokenEvent(ev[1], ev[2], ev[3]))
        elif ev[0] == "snapshot":
            sim.ProcessEvent(cl.SnapshotEvent(ev[1]))
        else:
            sim.Tick(ev[1])
    return sim


def replay_poisoned(sim):
    sim.poison_outputs()
    sim.rerun()
    sim.synchronize()


def blocked_ragged_sim(top, events, n, engine, fifo_lds_slots=None, want_engine=None, split=True, drain=True):
    """(sim, twin): `sim` flushed, then replayed from poisoned outputs through the slot map, its
    records block-major; `twin` flushed only, its records instance-major.  The regime is asserted
    before anything is read: mapped, block-major, and -- `split` -- 0 < spilled and 0 < split < n.
    want_engine: the exec kernel the launches must have used (a forced engine's own by default)."""
    if want_engine is None and engine != AUTO:
        want_engine = engine
    twin = build_sim(top, events, n, engine, fifo_lds_slots, drain)
    twin.flush()
    assert not twin.records_blocked()
    sim = build_sim(top, events, n, engine, fifo_lds_slots, drain)
    sim.flush()
    assert not sim.records_blocked()
    replay_poisoned(sim)
    for s in (sim, twin):
        assert want_engine is None or s.exec_engine() == want_engine, (s.exec_engine(), want_engine)
    assert sim.mapped_replays() and sim.records_blocked(), f"n = {n}: the replay did not go through the slot map"
    spilled, first = sim.replay_split()
    if split:
        assert 0 < spilled < n and 0 < first < n, f"n = {n}: (spilled, split) = {(spilled, first)}"
    return sim, twin
