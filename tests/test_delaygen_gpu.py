"""The device delay generator (csrc/cl_gorand.hip): its schedules against the sequential host
generator, and a batch run on device-generated rows against the same batch on host-generated rows
and against the oracle; per-instance seed lists under both generators."""
import os

import numpy as np
import pytest

import delaygencheck as G
import oracle as O
from enginecheck import compare_instance, new_sim, oracle_run
from snapcheck import TEST_DATA, read_text

cl = G.cl
pytestmark = pytest.mark.gpu

C3 = ("8nodes.top", "8nodes-concurrent-snapshots.events")
C2 = ("10nodes.top", "10nodes.events")


@pytest.mark.parametrize("draws", G.DRAWS)
def test_device_schedule_equals_sequential_on_consecutive_seeds(draws):
    # 4,096 rows: several workgroups on either mapping, and workgroups that end inside a row
    # (256 dwords per workgroup against rows of 4 .. 68 dwords) or inside a tile of four instances
    want = G.sequential(4097, draws)
    for n in (4096, 1, 4097):
        got, patched, ms = cl.go_delay_schedule_device(cl.REFERENCE_SEED, n, draws, return_info=True)
        assert got.shape == (n, draws) and got.dtype == np.uint8
        assert np.array_equal(got, want[:n]), f"n={n}: first difference at {np.argwhere(got != want[:n])[:1]}"
        assert ms > 0  # the kernel ran
        # what the host evaluation of the same closed form counted
        assert patched == cl.go_delay_schedule_jump(cl.REFERENCE_SEED, n, draws, return_info=True)[1]


@pytest.mark.parametrize("draws", G.DRAWS)
def test_device_schedule_equals_sequential_on_edge_seeds(draws):
    got = cl.go_delay_schedule_device(draws=draws, seeds=G.EDGE_SEEDS)
    assert np.array_equal(got, G.sequential_list(tuple(G.EDGE_SEEDS), draws))


def test_rejected_rows_are_patched_and_counted():
    got, patched, _ = cl.go_delay_schedule_device(draws=G.REJECT_DRAWS, seeds=G.REJECT_SEEDS, return_info=True)
    assert np.array_equal(got, G.sequential_list(tuple(G.REJECT_SEEDS), G.REJECT_DRAWS))
    assert patched == 3
    # a rejection beyond the draws asked for (rows are padded to 16 bytes) is none of this row's
    k = 47  # seed 2126476 rejects its 47th output
    got, patched, _ = cl.go_delay_schedule_device(2126476, 1, k - 1, return_info=True)
    assert patched == 0 and np.array_equal(got, G.sequential(1, k - 1, 2126476))
    got, patched, _ = cl.go_delay_schedule_device(2126476, 1, k, return_info=True)
    assert patched == 1 and np.array_equal(got, G.sequential(1, k, 2126476))
    # the north-star row: no rejection among 4,096 consecutive seeds at 112 draws -- by the kernel's
    # count, and by the sequential generator's raw outputs
    got, patched, _ = cl.go_delay_schedule_device(cl.REFERENCE_SEED, 4096, 112, return_info=True)
    assert patched == 0
    assert all(len(G.naive_intn5(cl.REFERENCE_SEED + i, 112)[1]) == 0 for i in range(4096))
    assert np.array_equal(got, G.sequential(4097, 112)[:4096])


def test_many_rejected_rows():
    # the same rejecting seed in every row: the flagged list holds duplicates of none, 600 rows
    seeds = [2126476] * 600
    got, patched, _ = cl.go_delay_schedule_device(draws=64, seeds=seeds, return_info=True)
    assert patched == 600
    assert np.array_equal(got, np.repeat(G.sequential(1, 64, 2126476), 600, axis=0))


def test_many_rejected_long_rows_flag_once_per_row():
    # the long-row kernel: 600 rows of 304 bytes, each with its one rejection
    got, patched, ms = cl.go_delay_schedule_device(draws=300, seeds=[2126476] * 600, return_info=True)
    assert patched == 600 and ms > 0
    assert np.array_equal(got, np.repeat(G.sequential(1, 300, 2126476), 600, axis=0))


def test_more_rejected_rows_than_the_list_holds_take_the_host_generator():
    n = 4200  # the flagged list holds 4,096 rows
    seeds = [2126476] * n
    got, patched, ms = cl.go_delay_schedule_device(draws=64, seeds=seeds, return_info=True)
    assert patched == 0 and ms == 0  # as above the row cap: nothing of this came from the kernel
    assert np.array_equal(got, np.repeat(G.sequential(1, 64, 2126476), n, axis=0))
    # the engine: the same batch under the device generator runs on host-generated rows
    sims = {g: _run(C3[0], C3[1], n, g, seeds=seeds) for g in ("host", "device")}
    assert sims["device"].delay_generator == "host" and sims["device"].delay_gen_time()[0] == 0
    r = _results(sims["device"])
    _assert_same(_results(sims["host"]), r)
    assert len(np.unique(r["hashes"])) == 1 and len(np.unique(r["time"])) == 1  # one stream, n times
    compare_instance(sims["device"], n - 1, oracle_run(C3[0], C3[1], seed=2126476), status=r["status"], times=r["time"])


# 12 nodes, every ordered pair linked: 132 channels, so 32 snapshots draw 4,224 delays
BIG_TOP = "12\n" + "".join(f"N{i:02d} 3\n" for i in range(12)) + \
    "".join(f"N{i:02d} N{j:02d}\n" for i in range(12) for j in range(12) if i != j)


def test_engine_rows_above_the_cap_fall_back_to_the_host_generator():
    n = 16
    seeds = [cl.REFERENCE_SEED + 3 * i for i in range(n - 1)] + [2126476]
    first = "snapshot N00\ntick\n"
    rest = "".join(f"snapshot N{(s % 12):02d}\ntick\n" for s in range(1, 32))
    sims = {}
    for g in ("host", "device"):
        sim = new_sim(n)
        sim.set_delay_generator(g)
        sim.set_delay_go_seed_list(seeds)
        sim.read_topology_text(BIG_TOP)
        sim.read_events_text(first)
        sim.flush()
        assert sim.draws_needed == 132 and sim.delay_generator == g  # (the list is in device memory now)
        sim.read_events_text(rest)
        assert sim.draws_needed == 32 * 132 > cl.DELAYGEN_MAX_DRAWS
        sim.flush()
        # rows longer than the kernel takes: the host generator, with the list fetched back
        assert sim.delay_generator == "host" and sim.delay_gen_time()[0] == 0
        sims[g] = sim
    assert sims["device"].device_bytes - sims["host"].device_bytes == 8 * 4097  # (no seed list on the device any more)
    r = _results(sims["device"])
    _assert_same(_results(sims["host"]), r)
    for i in (0, n - 1):
        ref = O.OracleSim()
        ref.seed_go(seeds[i])
        assert ref.read_topology_text(BIG_TOP) == 0
        for text in (first, rest):  # (two texts, each with its drain, as the sims ran them)
            assert ref.read_events_text(text, O.MAX_DRAIN_TICKS) >= 0
        compare_instance(sims["device"], i, ref, status=r["status"], times=r["time"])


def test_row_cap():
    cap = cl.DELAYGEN_MAX_DRAWS
    want = G.sequential(9, cap + 1)
    got, _, ms = cl.go_delay_schedule_device(cl.REFERENCE_SEED, 9, cap, return_info=True)
    assert ms > 0 and np.array_equal(got, want[:, :cap])      # the longest row the kernel takes
    got, patched, ms = cl.go_delay_schedule_device(cl.REFERENCE_SEED, 9, cap + 1, return_info=True)
    assert ms == 0 and patched == 0 and np.array_equal(got, want)  # above it: the host generator


def _run(top, events, n, generator, seeds=None, seed_base=cl.REFERENCE_SEED):
    sim = new_sim(n, seed_base=seed_base)
    sim.set_delay_generator(generator)
    if seeds is not None:
        sim.set_delay_go_seed_list(seeds)
    sim.read_topology_text(read_text(top))
    sim.read_events_text(events if "\n" in events else read_text(events))
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


# 10nodes.events needs 200 draws (rows of 208 bytes: still the no-communication mapping); the same
# program issued twice in one text needs 400, rows the kernel computes block by block
@pytest.mark.parametrize("cfg", [C3 + (8192, 1), C2 + (512, 1), C2 + (512, 2)],
                         ids=["8nodes_concurrent_x8192", "10nodes_x512", "10nodes_twice_x512"])
def test_engine_on_device_rows_equals_host_rows_and_oracle(cfg):
    top, name, n, times = cfg
    events = read_text(name) * times
    host, dev = _run(top, events, n, "host"), _run(top, events, n, "device")
    assert host.delay_generator == "host" and dev.delay_generator == "device"
    assert (dev.draws_needed > 273) == (times == 2)
    r = _results(dev)
    _assert_same(_results(host), r)
    device_ms, host_ms, patched = dev.delay_gen_time()
    assert device_ms > 0 and host_ms >= 0
    row = (dev.draws_needed + 15) // 16 * 16
    assert patched == cl.go_delay_schedule_jump(cl.REFERENCE_SEED, n, row, return_info=True)[1]
    assert host.delay_gen_time()[0] == 0 and host.delay_gen_time()[2] == 0
    for i in (0, 1, 63, 64, n // 2 + 1, n - 1):
        compare_instance(dev, i, oracle_run(top, events, seed=O.REFERENCE_SEED + i), status=r["status"],
                         times=r["time"])


def test_rows_grow_with_the_program():
    top, n = C3[0], 256
    lines = [ln for ln in read_text(C3[1]).split("\n") if ln]
    half = len(lines) // 2
    sims = {}
    for generator in ("host", "device"):
        sim = new_sim(n)
        sim.set_delay_generator(generator)
        sim.read_topology_text(read_text(top))
        sim.read_events_text("\n".join(lines[:half]) + "\n")
        sim.flush()
        first = sim.draws_needed
        assert sim.delay_generator == generator
        sim.read_events_text("\n".join(lines[half:]) + "\n")
        assert (sim.draws_needed + 15) // 16 > (first + 15) // 16  # the rows must get longer
        sim.flush()
        assert sim.delay_generator == generator
        sims[generator] = sim
    _assert_same(_results(sims["host"]), _results(sims["device"]))
    # and the regenerated rows are the same streams: the one-shot run's results
    one = new_sim(n)
    one.read_topology_text(read_text(top))
    one.read_events_text("\n".join(lines[:half]) + "\n")
    one.read_events_text("\n".join(lines[half:]) + "\n")
    _assert_same(_results(one), _results(sims["device"]))


def test_seed_list_reruns_selected_instances():
    top, events = C3
    a = _results(_run(top, events, 4096, "host"))
    rng = np.random.default_rng(11)
    insts = rng.choice(4096, 199, replace=False)  # unordered
    insts = np.concatenate([insts, insts[:1]])    # and one of them twice
    seeds = [cl.REFERENCE_SEED + int(j) for j in insts]
    sims = {g: _run(top, events, 200, g, seeds=seeds, seed_base=12345) for g in ("host", "device")}
    for g, sim in sims.items():
        assert sim.delay_generator == g
        b = _results(sim)
        assert np.array_equal(b["hashes"], a["hashes"][insts]), g
        assert np.array_equal(b["ticks"], a["ticks"][:, insts]), g
        assert np.array_equal(b["status"], a["status"][insts]) and np.array_equal(b["time"], a["time"][insts]), g
    # the list lives in device memory under the device generator (with the generator's flagged-row list)
    assert sims["device"].device_bytes - sims["host"].device_bytes == 8 * 200 + 8 * 4097


@pytest.mark.parametrize("generator", ["host", "device"])
def test_seed_list_with_rejecting_seeds_equals_the_oracle(generator):
    top, events = C3
    seeds = G.REJECT_SEEDS + [-1, 0, 2**63 - 1]
    sim = _run(top, events, len(seeds), generator, seeds=seeds)
    assert sim.draws_needed >= 64  # the three rejections (draws 38, 47, 54) are inside the rows
    status, times = sim.status(), sim.time()
    for i, seed in enumerate(seeds):
        compare_instance(sim, i, oracle_run(top, events, seed=seed), status=status, times=times)
    if generator == "device":
        row = (sim.draws_needed + 15) // 16 * 16
        want = cl.go_delay_schedule_jump(draws=row, seeds=seeds, return_info=True)[1]
        assert want >= 3 and sim.delay_gen_time()[2] == want
