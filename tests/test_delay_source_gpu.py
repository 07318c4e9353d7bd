"""The delay source of a live sim (csrc/cl_delays.cpp): seeds, seed lists, the generator and an
explicit schedule changed between runs of one sim.  After every change the sim must compute what
a fresh sim built directly in that configuration computes, and what the oracle computes."""
import numpy as np
import pytest

import oracle as O
from enginecheck import cl, compare_instance, new_sim, oracle_run
from snapcheck import read_text

pytestmark = pytest.mark.gpu

TOP, EVENTS = "8nodes.top", "8nodes-concurrent-snapshots.events"
BASE = cl.REFERENCE_SEED
LANES = cl.ChandyLamportSim.ENGINE_LANES


def _seed_list(n):
    # distinct streams unlike seed_base + i, one of them with a rejection inside the rows
    # (seed 2126476 rejects its 47th output)
    seeds = [BASE + 3 * i + 11 for i in range(n)]
    seeds[63] = 2126476
    return seeds


def _run(n, generator="host", seeds=None, seed_base=BASE, engine=None, events=None):
    sim = new_sim(n, seed_base=seed_base)
    if engine is not None:
        sim.set_exec_engine(engine)
    sim.set_delay_generator(generator)
    if seeds is not None:
        sim.set_delay_go_seed_list(seeds)
    sim.read_topology_text(read_text(TOP))
    sim.read_events_text(read_text(EVENTS) if events is None else events)
    sim.flush()
    return sim


def _results(sim):
    return dict(status=sim.status(), time=sim.time(), hashes=sim.instance_hashes(), sums=sim.checksums(),
                counters=sim.counters(), ok_counters=sim.counters(only_ok=True),
                ticks=np.stack([sim.snapshot_ticks(s) for s in range(sim.num_snapshots)]))


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _assert_oracle(sim, r, seed_of):
    n = sim.n_instances
    for i in (0, 63, 64, n - 1):
        compare_instance(sim, i, oracle_run(TOP, EVENTS, seed=seed_of(i)), status=r["status"], times=r["time"])


def test_packed_rows_follow_the_rows():
    n = 4096  # the smallest batch that replays through the slot map, on packed rows under the lanes kernels
    seeds = _seed_list(n)
    sim = _run(n, engine=LANES)

    def replayed_twice(want_generator):
        sim.rerun()
        assert sim.mapped_replays()  # (the first replay after a change is the probe of a new plan)
        sim.rerun()
        assert sim.exec_engine() == LANES and sim.records_blocked()  # through the map: packed rows
        r = _results(sim)
        assert sim.delay_generator == want_generator
        return r

    r = replayed_twice("host")
    _assert_same(_results(_run(n, engine=LANES)), r)
    _assert_oracle(sim, r, lambda i: BASE + i)

    sim.set_delay_go_seeds(BASE + 1)
    r = replayed_twice("host")
    _assert_same(_results(_run(n, engine=LANES, seed_base=BASE + 1)), r)
    _assert_oracle(sim, r, lambda i: BASE + 1 + i)

    sim.set_delay_go_seed_list(seeds)
    r = replayed_twice("host")
    _assert_same(_results(_run(n, engine=LANES, seeds=seeds)), r)
    _assert_oracle(sim, r, lambda i: seeds[i])

    sim.set_delay_generator("device")
    r2 = replayed_twice("device")
    _assert_same(r, r2)  # the same rows from the other generator
    _assert_same(_results(_run(n, "device", engine=LANES, seeds=seeds)), r2)
    _assert_oracle(sim, r2, lambda i: seeds[i])


def test_seed_list_moves_both_ways():
    n = 200
    seeds = _seed_list(n)
    sim = _run(n, "device", seeds=seeds)
    r = _results(sim)
    assert sim.delay_generator == "device"
    on_device = sim.device_bytes  # (after the readouts above: their buffers are counted too)
    _assert_oracle(sim, r, lambda i: seeds[i])

    sim.set_delay_generator("host")
    sim.rerun()
    _assert_same(r, _results(sim))
    assert sim.delay_generator == "host"
    # the list left the device; the device generator's flagged-row list stays
    assert sim.device_bytes == on_device - 8 * n

    sim.set_delay_generator("device")
    sim.rerun()
    r2 = _results(sim)
    _assert_same(r, r2)
    assert sim.delay_generator == "device" and sim.device_bytes == on_device
    _assert_oracle(sim, r2, lambda i: seeds[i])


def test_schedule_replaces_go_seeds_and_back():
    n = 256
    sim = _run(n)
    r = _results(sim)
    assert sim.delay_generator == "host"

    sim.set_delay_schedule(cl.go_delay_schedule(BASE + 7, n, sim.draws_needed))
    sim.rerun()
    r7 = _results(sim)
    _assert_same(_results(_run(n, seed_base=BASE + 7)), r7)
    assert sim.delay_generator is None  # the documented answer for an explicit schedule
    _assert_oracle(sim, r7, lambda i: BASE + 7 + i)

    sim.set_delay_go_seeds(BASE)
    sim.rerun()
    r0 = _results(sim)
    _assert_same(r, r0)
    assert sim.delay_generator == "host"
    _assert_oracle(sim, r0, lambda i: BASE + i)


def test_rows_grow_under_a_seed_list_on_the_device():
    n = 256
    seeds = _seed_list(n)
    lines = [ln for ln in read_text(EVENTS).split("\n") if ln]
    half = len(lines) // 2
    parts = ["\n".join(lines[:half]) + "\n", "\n".join(lines[half:]) + "\n"]
    sim = _run(n, "device", seeds=seeds, events=parts[0])
    first = sim.draws_needed
    assert sim.delay_generator == "device"
    sim.read_events_text(parts[1])
    assert (sim.draws_needed + 15) // 16 > (first + 15) // 16  # the rows must get longer
    sim.flush()
    assert sim.delay_generator == "device"
    r = _results(sim)
    # the one-shot run with the same list (on host-generated rows)
    one = _run(n, seeds=seeds, events=parts[0])
    one.read_events_text(parts[1])
    _assert_same(_results(one), r)
    for i in (0, 63, 64, n - 1):
        ref = O.OracleSim()
        ref.seed_go(seeds[i])
        assert ref.read_topology_text(read_text(TOP)) == 0
        for text in parts:  # (two texts, each with its drain, as the sims ran them)
            assert ref.read_events_text(text, O.MAX_DRAIN_TICKS) >= 0
        compare_instance(sim, i, ref, status=r["status"], times=r["time"])
