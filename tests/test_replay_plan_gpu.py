"""The replay plan of a live sim (csrc/cl_plan.h): every cause that voids a plan drops it -- a
pending probe with it -- the run after the drop probes again, and what the sim then computes is what
a fresh sim built directly in that configuration computes.

The regime is blockedcheck's: C3, 200 instances, 4 LDS ring slots per channel, so some instances
spill and replays split and go through the slot map.  Every sim here runs the node-parallel kernel
(no run-time compile): NODES, or AUTO, which stays node-parallel at this batch size.
"""
import numpy as np
import pytest

from blockedcheck import AUTO, C3_EVENTS, C3_TOP, NODES, SLOTS, build_sim, cl

pytestmark = pytest.mark.gpu

N = 200
BASE = cl.REFERENCE_SEED
MORE_EVENTS = "send N2 N3 1\nsnapshot N5\ntick 3\nsend N6 N7 1\n"
NO_PLAN = (-1, 0)


def _results(sim):
    return dict(status=sim.status(), time=sim.time(), sums=sim.checksums())


def _assert_same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def _sim(configure, engine=NODES, slots=SLOTS, more=False):
    """A sim with C3 loaded (`more`: and MORE_EVENTS) and `configure` applied, nothing run."""
    sim = build_sim(C3_TOP, C3_EVENTS, N, engine, slots)
    if more:
        sim.read_events_text(MORE_EVENTS)
    configure(sim)
    return sim


def _assert_regime(sim):
    spilled, split = sim.replay_split()
    assert 0 < spilled < N and 0 < split < N and sim.mapped_replays(), (spilled, split)


def test_every_cause_drops_the_plan():
    sim = _sim(lambda s: None)
    sim.flush()
    _assert_regime(sim)
    seeds = [BASE + 3 * i + 11 for i in range(N)]
    schedule = {}

    def the_schedule(s):  # (as long as the program of the sim it is set on needs)
        d = s.draws_needed
        schedule.setdefault(d, cl.go_delay_schedule(BASE + 7, N, d))
        s.set_delay_schedule(schedule[d])

    # (cause, what it does to the live sim, the same configuration on a fresh sim): cumulative
    config = []
    causes = [
        ("another seed base", lambda s: s.set_delay_go_seeds(BASE + 5), {}),
        ("a seed list", lambda s: s.set_delay_go_seed_list(seeds), {}),
        ("the other generator", lambda s: s.set_delay_generator("device"), {}),
        ("appended events", lambda s: s.read_events_text(MORE_EVENTS), {"more": True}),
        ("a schedule", the_schedule, {}),
        ("the exec engine", lambda s: s.set_exec_engine(AUTO), {"engine": AUTO}),
    ]
    fresh_kw = {}
    for what, apply, kw in causes:
        apply(sim)
        assert sim.replay_split() == NO_PLAN and not sim.mapped_replays(), what
        sim.rerun()
        sim.synchronize()
        assert sim.replay_split()[0] >= 0, what  # that run was a probe
        r = _results(sim)
        if kw:
            fresh_kw.update(kw)
        else:
            config.append(apply)
        fresh = _sim(lambda s: [c(s) for c in config], **fresh_kw)
        fresh.flush()
        _assert_same(_results(fresh), r, what)
        assert sim.replay_split() == fresh.replay_split(), what
        assert sim.exec_engine() == NODES and fresh.exec_engine() == NODES, what
        if sim.mapped_replays():  # the replay through the new plan
            sim.rerun()
            assert sim.records_blocked(), what
            _assert_same(_results(sim), r, what)

    # other ring slots change the layout: the plan goes at the next launch, not in the setter
    sim.set_limits(fifo_lds_slots=8)
    sim.rerun()
    sim.synchronize()
    assert sim.replay_split()[0] >= 0
    fresh = _sim(lambda s: [c(s) for c in config], slots=8, **fresh_kw)
    fresh.flush()
    _assert_same(_results(fresh), _results(sim), "8 ring slots")
    assert sim.replay_split() == fresh.replay_split()


def test_a_drop_cancels_the_pending_probe():
    sim = _sim(lambda s: None)
    sim.rerun()  # the probe, not yet evaluated
    sim.set_delay_go_seeds(BASE + 5)
    assert sim.replay_split() == NO_PLAN  # (not a plan of the run on the old seeds)
    assert not sim.mapped_replays()
    sim.rerun()
    sim.synchronize()
    fresh = _sim(lambda s: s.set_delay_go_seeds(BASE + 5))
    fresh.flush()
    _assert_same(_results(fresh), _results(sim), "after the cancelled probe")
    _assert_regime(sim)
    assert sim.replay_split() == fresh.replay_split()


def test_the_plan_is_the_policys_for_the_probe():
    """cl_replay_plan_of on the probe's own final ticks.  The spill flags cannot be read per
    instance, and the split depends only on how many there are: the flags go on the last instances."""
    sim = _sim(lambda s: None)
    sim.flush()
    _assert_regime(sim)
    spilled, split = sim.replay_split()
    flags = np.zeros(N, dtype=np.uint8)
    flags[N - spilled:] = 1
    ipw = 64 // sim.num_nodes
    _, mapped, p_split, p_spilled = cl.replay_plan_of(sim.time(), flags, ipw, True)
    assert (p_spilled, p_split, mapped) == (spilled, split, sim.mapped_replays())
