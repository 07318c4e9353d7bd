"""The closed form of Go's math/rand delay streams (csrc/cl_gorand.h) evaluated on the host
(cl_go_delay_schedule_jump) against the sequential generator, and the host side of the new
delay-generator calls.  No GPU: every check here must hold on a machine without a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import delaygencheck as G
from snapcheck import ROOT, TEST_DATA

cl = G.cl
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "go_rng_kat.json")))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("draws", G.DRAWS)
def test_jump_equals_sequential_on_consecutive_seeds(draws):
    got, rejected = cl.go_delay_schedule_jump(cl.REFERENCE_SEED, 300, draws, return_info=True)
    assert got.shape == (300, draws) and got.dtype == np.uint8
    assert np.array_equal(got, G.sequential(300, draws))
    assert rejected == 0  # (and none of these rows needed the sequential generator)


@pytest.mark.parametrize("draws", G.DRAWS)
def test_jump_equals_sequential_on_edge_seeds(draws):
    got = cl.go_delay_schedule_jump(draws=draws, seeds=G.EDGE_SEEDS)
    assert np.array_equal(got, G.sequential_list(tuple(G.EDGE_SEEDS), draws))


def test_edge_seeds_normalise_as_go_does():
    # norm_seed of cl_gorand.h: seed mod (2^31 - 1), made positive; 0 -> 89482311 (rng.go Seed)
    w = cl.go_delay_schedule_jump(draws=64, seeds=G.EDGE_SEEDS)
    by = dict(zip(G.EDGE_SEEDS, w))
    assert np.array_equal(by[0], by[G.M]) and np.array_equal(by[0], by[2 * G.M]) and np.array_equal(by[0], by[-G.M])
    assert np.array_equal(by[0], cl.go_delay_schedule(89482311, 1, 64)[0])
    assert np.array_equal(by[1], by[G.M + 1]) and np.array_equal(by[-1], by[G.M - 1])
    assert not np.array_equal(by[0], by[1])


def test_rejections_are_found_and_resolved():
    got, rejected = cl.go_delay_schedule_jump(draws=G.REJECT_DRAWS, seeds=G.REJECT_SEEDS, return_info=True)
    assert np.array_equal(got, G.sequential_list(tuple(G.REJECT_SEEDS), G.REJECT_DRAWS))
    assert rejected == 3
    for row, seed in zip(got, G.REJECT_SEEDS):
        naive, at = G.naive_intn5(seed, G.REJECT_DRAWS + 1)
        if seed in G.REJECTING:
            assert len(at) == 1 and at[0] < G.REJECT_DRAWS
            k = at[0]
            assert not np.array_equal(row, naive[:G.REJECT_DRAWS])
            # equal before the rejected output, shifted by one output after it
            assert np.array_equal(row[:k], naive[:k]) and np.array_equal(row[k:], naive[k + 1:])
        else:
            assert len(at) == 0 and np.array_equal(row, naive[:G.REJECT_DRAWS])
    # the draws the rejections were found at (counted from 1: the output numbers k)
    assert [int(G.naive_intn5(s, 97)[1][0]) + 1 for s in G.REJECTING] == [47, 54, 38]


def test_jump_agrees_with_the_known_answers():
    got = cl.go_delay_schedule_jump(KAT["refseed"], 1, 200)
    assert "".join(str(v) for v in got[0].tolist()) == KAT["refseed_intn5_200"]


def test_empty_shapes():
    assert cl.go_delay_schedule_jump(5, 0, 10).shape == (0, 10)
    assert cl.go_delay_schedule_jump(5, 3, 0).shape == (3, 0)


def test_argument_checks():
    L = cl.lib()
    out = np.zeros((4, 8), dtype=np.uint8)
    seeds = np.arange(4, dtype=np.int64)
    rej = C.c_int64(-1)
    # jump: NULL out, negative shapes; a NULL rejected_rows and a NULL seed list are fine
    assert L.cl_go_delay_schedule_jump(1, None, 4, 8, None, C.byref(rej)) == cl.E_INVALID
    assert L.cl_go_delay_schedule_jump(1, None, -1, 8, _p(out), C.byref(rej)) == cl.E_INVALID
    assert L.cl_go_delay_schedule_jump(1, None, 4, -1, _p(out), C.byref(rej)) == cl.E_INVALID
    assert L.cl_go_delay_schedule_jump(1, None, 4, 8, _p(out), None) == 0
    assert L.cl_go_delay_schedule_jump(0, _p(seeds), 4, 8, _p(out), C.byref(rej)) == 0 and rej.value == 0
    assert np.array_equal(out, cl.go_delay_schedule(0, 4, 8))
    # device form: arguments are checked before the device is looked for
    assert L.cl_go_delay_schedule_device(0, 1, None, 4, 8, None, None, None) == cl.E_INVALID
    assert L.cl_go_delay_schedule_device(0, 1, None, -1, 8, _p(out), None, None) == cl.E_INVALID
    assert L.cl_go_delay_schedule_device(0, 1, None, 4, -1, _p(out), None, None) == cl.E_INVALID

    sim = cl.ChandyLamportSim(4)
    for mode in (-1, 2, 7):
        assert L.cl_set_delay_generator(sim._h, mode) == cl.E_INVALID
    with pytest.raises(cl.ClSnapError) as e:
        sim.set_delay_generator("gpu")
    assert e.value.code == cl.E_INVALID
    assert L.cl_delay_generator(sim._h, None) == cl.E_INVALID
    assert sim.delay_generator is None  # no rows exist yet
    assert L.cl_set_delay_go_seed_list(sim._h, None, 4) == cl.E_INVALID
    for n in (0, 3, 5):
        assert L.cl_set_delay_go_seed_list(sim._h, _p(seeds), n) == cl.E_INVALID
    assert L.cl_set_delay_go_seed_list(sim._h, _p(seeds), 4) == 0
    with pytest.raises(cl.ClSnapError) as e:
        sim.set_delay_go_seed_list([1, 2, 3])
    assert e.value.code == cl.E_INVALID
    # nothing has been generated: no times to report, whichever pointers are asked for
    assert L.cl_delay_gen_time(sim._h, None, None, None) == cl.E_STATE
    with pytest.raises(cl.ClSnapError) as e:
        sim.delay_gen_time()
    assert e.value.code == cl.E_STATE
    for name in ("go_delay_schedule_device", "go_delay_schedule_jump"):
        assert name in cl.__all__
        for kw in ({}, {"draws": 4}, {"n": 3, "seeds": [1, 2]}):  # neither n nor seeds; n against the list
            with pytest.raises(cl.ClSnapError) as e:
                getattr(cl, name)(**kw)
            assert e.value.code == cl.E_INVALID
    assert sim.device_bytes == 0  # (the list is on the host until the device generator runs)


def test_generator_choice_and_seed_list_replace_each_other_on_the_host():
    sim = cl.ChandyLamportSim(4)
    sim.set_delay_generator("device")
    sim.set_delay_generator("host")
    sim.set_delay_go_seed_list([5, 5, -9, 2**63 - 1])
    sim.set_delay_go_seeds(17)
    sim.set_delay_go_seed_list(np.array([1, 2, 3, 4]))
    sim.set_delay_schedule(np.zeros((4, 3), dtype=np.uint8))
    assert sim.delay_generator is None


def test_no_gpu_device_form_and_seed_list_flush_fail_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    out = np.zeros((4, 8), dtype=np.uint8)
    assert cl.lib().cl_go_delay_schedule_device(0, 1, None, 4, 8, _p(out), None, None) == cl.E_DEVICE
    with pytest.raises(cl.ClSnapError) as e:
        cl.go_delay_schedule_device(1, 4, 8)
    assert e.value.code == cl.E_DEVICE

    def program(sim):
        sim.read_topology_file(os.path.join(TEST_DATA, "2nodes.top"))
        sim.read_events_file(os.path.join(TEST_DATA, "2nodes-simple.events"))
        return sim.draws_needed

    plain = cl.ChandyLamportSim(4)
    want = program(plain)
    for generator in ("host", "device"):
        sim = cl.ChandyLamportSim(4)
        sim.set_delay_generator(generator)
        sim.set_delay_go_seed_list([9, 8, 7, 6])
        assert program(sim) == want
        with pytest.raises(cl.ClSnapError) as e:
            sim.flush()
        assert e.value.code == cl.E_DEVICE
        with pytest.raises(cl.ClSnapError):
            sim.status()
        assert sim.delay_generator is None
