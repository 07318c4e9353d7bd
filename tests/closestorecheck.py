"""Programs and the replay check for the tests of the program-specialized lanes kernels' close
stores and broadcast guard (cl_lanes.h TokIn, Guard): such a kernel stores no end cursor when a
marker closes an in-link its program never sends on -- the record's word holds the 0 since the
same launch created the record -- and, where the delay rows hold the program's own bound on draws
(cl_delay_draws_needed), its broadcast guard has no row-end test.  The topologies are
tokenlinkcheck's; node ids are in rank order, so a node's in-links are numbered by the order of
its senders."""
import numpy as np

import oracle as O
import tokenlinkcheck as K
from enginecheck import cl, compare_instance, oracle_run

LANES = cl.ChandyLamportSim.ENGINE_LANES
ON, OFF = cl.ChandyLamportSim.PROGRAM_ON, cl.ChandyLamportSim.PROGRAM_OFF
SIZES = [4096 + 17, 64 + 5]
SLOTS = 8   # ring slots per channel above every channel's packet count: nothing spills

# T4 (tokenlinkcheck): I -> X, I -> Y, I -> Z, X -> Y, X -> Z, Y -> I, Z -> I.  In-links: I has
# Y (0) and Z (1), X has I (0), Y has I (0) and X (1), Z has I (0) and X (1).

# Z -> I is the only token link.  In a row of zero delays snapshot 0 runs like this: I's markers
# are due at tick 1 and I delivers one a tick, in dest order -- X at tick 1, Y at 2, Z at 3.  X
# broadcasts at tick 1, its markers are due at 2 and go to Y at tick 2 and to Z at tick 3.  So at
# tick 2 Y's in-link 0 (from I) creates Y's record and its token-free in-link 1 (from X) closes in
# the same tick, and at tick 3 the same happens at Z.  Z's marker reaches I at tick 4, which
# completes the snapshot.  The token sent before the snapshot arrives at tick 1 and is recorded.
SAME_TICK_CLOSE_EVENTS = "send Z I 1\nsnapshot I\n"

# I starts both snapshots: each of its in-links closes later, Y -> I with tokens and Z -> I without.
INITIATOR_EVENTS = "send Y I 2\nsnapshot I\ntick 1\nsend Y I 1\nsnapshot I\nsend Y I 3\n"

# 2 sends and 2 snapshot ids on 7 channels: at most 16 draws, and exactly 16 where every send
# succeeds and every node broadcasts for both snapshots (T4 is strongly connected, the tokens
# suffice).  The 16th draw is the delay of the last broadcast's last marker.
COVER_EVENTS = "send I X 1\nsnapshot I\ntick 3\nsend X Y 2\nsnapshot Y\n"
COVER_DRAWS = 16

# (name, topology, events, ring slots) of every program of the GPU cases, for the host test
COMPILE_CASES = [
    ("no_send", K.T4_TOP, K.NO_SEND_EVENTS, SLOTS),
    ("every_channel", K.T4_TOP, K.EVERY_CHANNEL_EVENTS, SLOTS),
    ("shared_cursor", K.T4_TOP, K.SHARED_CURSOR_EVENTS, SLOTS),
    ("same_tick_close", K.T4_TOP, SAME_TICK_CLOSE_EVENTS, SLOTS),
    ("initiator", K.T4_TOP, INITIATOR_EVENTS, SLOTS),
    ("spill", K.T4_TOP, K.SPILL_EVENTS, 2),
    ("cover", K.T4_TOP, COVER_EVENTS, SLOTS),
]


def mixed_rows(n, width, seed):
    """Delay rows: an instance draws either 0 throughout or uniformly from 0..4.  The two kinds end
    their drains far enough apart that the planner orders the large batch by length, so its
    replays go through the slot map."""
    rng = np.random.default_rng(seed)
    hi = rng.choice([1, 5], size=(n, 1))
    return (rng.integers(0, 5, size=(n, width)) % hi).astype(np.uint8)


def sample(n):
    return tuple(i for i in tuple(range(0, 80)) + (777, 2048, 4095, 4096, 4112) if i < n)


def make_sim(top, events, n, sched, mode, slots=SLOTS):
    sim = cl.ChandyLamportSim(n, fifo_lds_slots=slots)
    sim.set_exec_engine(LANES)
    sim.set_program_kernels(mode)
    sim.read_topology_text(top)
    sim.set_delay_schedule(sched)
    sim.read_events_text(events)
    return sim


def outputs(sim):
    out = [sim.status(), sim.time(), sim.checksums(), sim.counters(only_ok=False), sim.counters(only_ok=True),
           sim.instance_hashes()]
    for sid in range(sim.num_snapshots):
        out.append(sim.snapshot_ticks(sid))
        out.extend(sim.collect_snapshot_packed(sid))
    out.append([sim.node_tokens(i) for i in sample(sim.n_instances)])
    return out


def same(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, (dict, list)):
            assert x == y, (what, k)
        else:
            assert np.array_equal(x, y), (what, k)


def replay(sim, spec, mapped, sched_draws):
    """Generic flush, then a poisoned rerun: the rerun's outputs, equal to the flush's.
    sched_draws: draws per row of the sim's schedule."""
    sim.flush()
    assert sim.exec_engine() == LANES and not sim.exec_program_kernels()   # a first launch is generic
    gen = outputs(sim)
    sim.poison_outputs()
    sim.rerun()
    sim.synchronize()
    assert sim.exec_engine() == LANES and sim.exec_program_kernels() == spec
    # the guard's row-end test is compiled out exactly where the rows hold the program's bound
    assert sim.exec_program_cover() == (spec and sched_draws >= sim.draws_needed)
    assert sim.records_blocked() == sim.mapped_replays()
    assert mapped is None or sim.mapped_replays() == mapped
    out = outputs(sim)
    same(out, gen, "rerun vs generic flush")
    return out


def check(top, events, n, sched, slots=SLOTS, equal_lengths=False, any_order=False):
    """The specialized sim against its own generic flush, against a sim with the program kernels
    off, against the oracle's batch and, instance by instance, on the sample.  Returns (the
    specialized sim, its outputs).  any_order: the planner's choice of the slot map is not part
    of the case (instances that fail at different ticks)."""
    mapped = n >= 4096 and not equal_lengths   # (instances of one length keep the identity order)
    if any_order:
        mapped = None
    sim = make_sim(top, events, n, sched, ON, slots)
    width = sched.shape[1]
    got = replay(sim, True, mapped, width)
    off = make_sim(top, events, n, sched, OFF, slots)
    same(replay(off, False, mapped, width), got, "program kernels off vs on")
    status, times = got[0], got[1]
    _, st, ticks, cnt, hashes = O.run_batch(top, events, n, sched=sched, draws=width, threads=8)
    ok = st == 0
    assert np.array_equal(status, st)
    assert np.array_equal(times[ok], ticks[ok])
    assert np.array_equal(got[5][ok], hashes[ok])
    c = got[4]
    assert c["recorded"] == cnt[ok, 4].sum() and c["completed"] == cnt[ok, 6].sum()
    if ok.all():
        c = got[3]
        assert (c["push"], c["peek"], c["pop_tok"], c["pop_mk"]) == tuple(cnt[:, k].sum() for k in range(4))
    for i in sample(n):
        compare_instance(sim, i, oracle_run(top, events, schedule=sched[i]), status=status, times=times)
    return sim, got
