"""The delay source's setters on a sim that has no device yet (csrc/cl_delays.cpp): the sequences
tests/test_delay_source_gpu.py runs on a live sim.  No GPU: nothing here may need a device."""
import ctypes as C

import numpy as np

import delaygencheck as G

cl = G.cl
BASE = cl.REFERENCE_SEED


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_setter_sequences_need_no_device():
    L = cl.lib()
    n = 8
    seeds = np.array([BASE + 3 * i + 11 for i in range(n)], dtype=np.int64)
    plane = cl.go_delay_schedule(BASE + 7, n, 48)
    HOST, DEVICE = 0, 1

    def no_generation_yet(sim):
        assert L.cl_delay_gen_time(sim._h, None, None, None) == cl.E_STATE
        assert sim.delay_generator is None and sim.device_bytes == 0

    # seeds, then a seed list, then the other generator
    sim = cl.ChandyLamportSim(n)
    assert L.cl_set_delay_go_seeds(sim._h, BASE + 1) == 0
    assert L.cl_set_delay_go_seed_list(sim._h, _p(seeds), n) == 0
    assert L.cl_set_delay_generator(sim._h, DEVICE) == 0
    no_generation_yet(sim)
    # a seed list under the device generator, to the host generator and back
    sim = cl.ChandyLamportSim(n)
    assert L.cl_set_delay_generator(sim._h, DEVICE) == 0
    assert L.cl_set_delay_go_seed_list(sim._h, _p(seeds), n) == 0
    assert L.cl_set_delay_generator(sim._h, HOST) == 0
    assert L.cl_set_delay_generator(sim._h, HOST) == 0  # (already that mode)
    assert L.cl_set_delay_generator(sim._h, DEVICE) == 0
    no_generation_yet(sim)
    # a schedule in place of Go seeds, and back
    sim = cl.ChandyLamportSim(n)
    assert L.cl_set_delay_schedule(sim._h, _p(plane), plane.shape[1]) == 0
    assert L.cl_set_delay_go_seeds(sim._h, BASE) == 0
    no_generation_yet(sim)
    # a refused schedule leaves the source as it was
    bad = plane.copy()
    bad[3, 5] = 5
    assert L.cl_set_delay_schedule(sim._h, _p(bad), bad.shape[1]) == cl.E_INVALID
    assert L.cl_set_delay_schedule(sim._h, None, 4) == cl.E_INVALID
    assert L.cl_set_delay_schedule(sim._h, _p(plane), 0) == cl.E_INVALID
    no_generation_yet(sim)
