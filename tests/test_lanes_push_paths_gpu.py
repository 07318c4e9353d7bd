"""The instance-per-lane kernel's two push paths (cl_lanes.h phase D and start_snapshot), at the
edges of the guard that chooses between them.

A first marker's broadcast takes, for the whole wave, either the push that cannot fail (the row
holds all the broadcast's draws and none of the node's rings is full, on every lane whose trigger
is on) or push() with Queue.Push's failure bookkeeping.  These cases sit on the guard's edges:

* the delay row ends exactly at a broadcast's last link (fast path, the row's last delay is used)
  and one short of it (slow path: the earlier links of the same broadcast still land, the last
  one is DELAY_EXHAUSTED), for a tick's broadcast and for the initiator's (start_snapshot);
* a ring holds CAP - 1 packets when a broadcast pushes onto it (fast) and CAP packets (slow: the
  packet goes to the HBM spill ring, is refilled and delivered), with both kinds in one wave in
  the same tick;
* two first markers at one receiver in one tick, the first broadcast normal and the second
  running out of the row (the further passes over the receivers).

Every case runs forced onto the lanes engine through a flush (fresh, spill-capable kernel,
instance-major records) and through rerun() at 4096 instances (replay plan, block-major records:
the spill-free kernel runs every instance the plan knows not to spill), and is compared with the
oracle instance by instance -- status, time, counters, per-instance hash, CollectSnapshot on a
sample -- and array for array with the node-parallel engine, which also pins what a frozen
instance leaves behind (the oracle comparison of such an instance ends at its status).

Not reachable from here: FIFO_OVERFLOW on the spill-free kernel.  A layout whose rings can
overflow has spill rings, and the replay plan sends every instance that spills to the
spill-capable half.

Reference: node.go:97-109 (SendToNeighbors draws in dest order), sim.go:100-102, queue.go:18-20.
"""
import numpy as np
import pytest

import oracle as O
from enginecheck import cl, compare_instance, oracle_batch, oracle_run

pytestmark = pytest.mark.gpu

LANES = cl.ChandyLamportSim.ENGINE_LANES
NODES = cl.ChandyLamportSim.ENGINE_NODES
N_INST = 4096          # rerun() replays through the slot map from 4096 instances up
SAMPLE = tuple(range(0, 128)) + (777, 2048, 4095)

# I broadcasts to X, Y, Z (dest order); X to Y and Z; Y and Z answer I.  With I's marker late at
# X (delay 4) and at once at Y and Z, X's broadcast on its two links is the last of the 7 draws
# of "snapshot I": draws 0-2 I's, 3 and 4 Y's and Z's, 5 and 6 X's.
T4_TOP = "4\nI 20\nX 20\nY 20\nZ 20\nI X\nI Y\nI Z\nX Y\nX Z\nY I\nZ I\n"
# the 5-node star of test_lanes_edges_gpu: H takes several first markers in one tick
HUB_TOP = "5\nH 100\nA 50\nB 50\nC 50\nD 50\n" + "".join(f"H {x}\n{x} H\n" for x in "ABCD")


def _sim(top, events, sched, engine, slots=None):
    sim = cl.ChandyLamportSim(N_INST, fifo_lds_slots=slots)
    sim.set_exec_engine(engine)
    sim.read_topology_text(top)
    sim.set_delay_schedule(sched)
    sim.read_events_text(events)
    sim.flush()
    assert sim.exec_engine() == engine
    return sim


def _outputs(sim):
    return (sim.status(), sim.time(), sim.checksums(), sim.counters(only_ok=False), sim.counters(only_ok=True),
            sim.instance_hashes())


def _same(a, b, what):
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert x == y, what
        else:
            assert np.array_equal(x, y), what


def _check(top, events, sched, slots=None):
    """Lanes flush and lanes rerun against the oracle and the node-parallel engine.  Returns the
    oracle's statuses."""
    _, st, ticks, cnt, hashes = oracle_batch(top, events, N_INST, schedule=sched, draws=sched.shape[1])
    ok = st == 0
    nodes = _outputs(_sim(top, events, sched, NODES, slots))
    sim = _sim(top, events, sched, LANES, slots)
    for phase in ("flush", "rerun"):
        if phase == "rerun":
            sim.poison_outputs()
            sim.rerun()
            sim.synchronize()
            assert sim.exec_engine() == LANES and sim.records_blocked()
        got = _outputs(sim)
        _same(got, nodes, f"{phase}: lanes vs node-parallel")
        status, times = got[0], got[1]
        assert np.array_equal(status, st), phase
        assert np.array_equal(times[ok], ticks[ok]), phase
        assert np.array_equal(got[5][ok], hashes[ok]), phase
        c = got[4]
        assert c["recorded"] == cnt[ok, 4].sum() and c["completed"] == cnt[ok, 6].sum(), phase
        if ok.all():  # (a frozen instance's counters are the engine's, pinned by the node-parallel run)
            c = got[3]
            assert (c["push"], c["peek"], c["pop_tok"], c["pop_mk"]) == tuple(cnt[:, k].sum() for k in range(4)), phase
        for i in SAMPLE:
            compare_instance(sim, i, oracle_run(top, events, schedule=sched[i]), status=status, times=times)
    return st


def _t4_rows(width, seed):
    """Half of the instances (the even ones) with X's broadcast last in draw order, the others
    with random delays: for those the row ends in whichever broadcast comes last."""
    rng = np.random.default_rng(seed)
    sched = rng.integers(0, 5, size=(N_INST, width), dtype=np.uint8)
    sched[0::2, 0] = 4
    sched[0::2, 1:3] = 0
    return sched


@pytest.mark.parametrize("width", [2, 3, 6, 7])
def test_row_ends_at_a_broadcast(width):
    """"snapshot I" draws 7 delays.  Width 7: every broadcast fits, and in the even instances the
    row's last delay is the last link of X's broadcast (k0 + od == draws, fast path): all OK.
    Width 6: in the even instances X's push to Y lands and its push to Z is DELAY_EXHAUSTED.
    Widths 3 and 2: the same at the initiator's broadcast of three (start_snapshot), then its
    receivers' broadcasts run out (3) or its own last link does (2)."""
    st = _check(T4_TOP, "snapshot I\n", _t4_rows(width, 100 + width))
    want = O.OK if width == 7 else cl.INST_DELAY_EXHAUSTED
    assert (st == want).all()   # every instance sits on the edge (the even half at X's, by construction)


def _log_depth_at_marker(top, events, row, src, dst):
    """From the oracle's Logger: (epoch, packets queued on src -> dst) when src first sends a
    marker to dst."""
    ref = O.OracleSim()
    ref.use_schedule(row)
    ref.log_enable()
    assert ref.read_topology_text(top) == 0
    assert ref.read_events_text(events) >= 0
    ids = ref.node_ids()
    s, d = ids.index(src), ids.index(dst)
    depth = 0
    for epoch, kind, node, other, _data, _tok in ref.log():
        if kind in (cl.LOG_SENT_TOKEN, cl.LOG_SENT_MARKER) and node == s and other == d:
            if kind == cl.LOG_SENT_MARKER:
                return epoch, depth
            depth += 1
        elif kind in (cl.LOG_RECV_TOKEN, cl.LOG_RECV_MARKER) and node == d and other == s:
            depth -= 1
    raise AssertionError("no marker sent")


RING_EVENTS = "send X Y 1\nsend X Y 2\nsnapshot I\n"


def ring_rows():
    rng = np.random.default_rng(5)
    return rng.integers(0, 5, size=(N_INST, 9), dtype=np.uint8)   # 2 sends + 7 broadcast draws


def classify_ring(sched, insts):
    """Per instance of `insts`: (epoch of X's broadcast, packets on X -> Y at that push)."""
    return [_log_depth_at_marker(T4_TOP, RING_EVENTS, sched[i], "X", "Y") for i in insts]


def test_ring_full_and_one_short_in_one_wave():
    """Two LDS slots per channel; X -> Y holds the two tokens sent before the snapshot until they
    are delivered.  When X broadcasts, its ring to Y holds 2 packets (full: slow path, the marker
    goes to the HBM spill ring), 1 (CAP - 1: fast path) or none, by the instance's delays.  The
    first wave (instances 0-63) must hold, in one tick, lanes of both kinds: required here from
    the oracle alone, at least 2 lanes full and 2 lanes one short of full in the same tick."""
    sched = ring_rows()
    kinds = classify_ring(sched, range(64))
    by_tick = {}
    for epoch, depth in kinds:
        by_tick.setdefault(epoch, []).append(depth)
    assert any(v.count(2) >= 2 and v.count(1) >= 2 for v in by_tick.values()), by_tick
    st = _check(T4_TOP, RING_EVENTS, sched, slots=2)
    assert (st == O.OK).all()


@pytest.mark.parametrize("width", [9, 10])
def test_two_first_markers_in_one_tick_second_runs_out(width):
    """A and B start snapshots and both markers reach H in tick 1 (draws 0 and 1 are zero in the
    even instances): H broadcasts twice in that tick on its four links, draws 2-5 and 6-9.  Width
    9: the first broadcast is normal, the second runs out at its last link.  Width 10: the second
    ends exactly at the row's end, and the leaves' answers run out."""
    rng = np.random.default_rng(40 + width)
    sched = rng.integers(0, 5, size=(N_INST, width), dtype=np.uint8)
    sched[0::2, 0:2] = 0
    st = _check(HUB_TOP, "snapshot A\nsnapshot B\ntick 1\n", sched)
    assert (st == cl.INST_DELAY_EXHAUSTED).all()
