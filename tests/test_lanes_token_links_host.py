"""CPU checks of the lanes kernels' token-link predicate (cl_lanes.h TokIn): the generic kernels
and the program-specialized ones compile for gfx950 without a device on every topology and program of the GPU runs (test_lanes_token_links_gpu.py) -- programs without a
send, with a send on every channel, with a send to an unknown destination, with records of 2, 4
and 8 words, with one and two pending words -- and the oracle shows that each program does what
its case is about."""
import numpy as np
import pytest

import oracle as O
import tokenlinkcheck as K
from enginecheck import canonical, cl, oracle_run


@pytest.mark.parametrize("top,events", [c[1:] for c in K.COMPILE_CASES], ids=[c[0] for c in K.COMPILE_CASES])
def test_kernels_compile(top, events):
    sim = cl.ChandyLamportSim(64, fifo_lds_slots=2 if events is K.SPILL_EVENTS else 8)
    sim.read_topology_text(top)
    sim.read_events_text(events)
    ms, log = sim.lanes_compile_check()
    assert ms > 0 and "error" not in log.lower()
    ms, specialized, log = sim.lanes_program_compile_check()
    assert specialized and ms > 0
    assert "error" not in log.lower()


def test_program_with_its_last_send_after_the_drain_compiles():
    sim = cl.ChandyLamportSim(64, fifo_lds_slots=8)
    sim.read_topology_text(K.T4_TOP)
    sim.read_events_text(K.LAST_ARM_EVENTS)
    sim.ProcessEvent(cl.PassTokenEvent(*K.LAST_ARM_SEND))
    ms, specialized, log = sim.lanes_program_compile_check()
    assert specialized and ms > 0 and "error" not in log.lower()


def test_oracle_statuses_of_the_programs():
    rows = np.random.default_rng(7).integers(0, 5, size=(16, 120), dtype=np.uint8)
    want = {"unknown_dest": {O.FATAL_UNKNOWN_DEST}, "source_initiator": {O.HANG},
            "insufficient": {O.OK, O.FATAL_INSUFFICIENT_TOKENS}}
    for name, top, events in K.COMPILE_CASES:
        md = 24 if name == "source_initiator" else O.MAX_DRAIN_TICKS
        got = {oracle_run(top, events, schedule=rows[i], max_drain=md).status for i in range(16)}
        assert got <= want.get(name, {O.OK}), name


def test_oracle_records_tokens_only_on_the_token_link():
    rows = np.zeros((1, 48), dtype=np.uint8)
    ref = oracle_run(K.T4_TOP, K.SHARED_CURSOR_EVENTS, schedule=rows[0])
    assert canonical(ref.collect(0).messages) == {("Z", "I"): [2, 1]}
    assert canonical(ref.collect(1).messages) == {("Z", "I"): [3]}
