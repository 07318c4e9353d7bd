"""CPU checks of the lanes kernels' sender pairing (cl_lanes.h Pairs): the constexpr pairing
table and the packed phase A compile for gfx950 without a device on topologies with an odd node
count, with nodes without out-links, and with pairs of unequal out-degrees -- the generic kernels
and the program-specialized ones (the GPU runs are test_lanes_packed_heads_gpu.py)."""
import pytest

import packedcheck as P
from enginecheck import cl

CASES = [(P.ODD_TOP, P.ODD_EVENTS), (P.SINKS_TOP, P.SINKS_EVENTS), (P.T4_TOP, P.T4_EVENTS)]
IDS = ["odd_all_senders", "odd_two_sinks", "unequal_degrees"]


@pytest.mark.parametrize("top,events", CASES, ids=IDS)
def test_paired_kernels_compile(top, events):
    sim = cl.ChandyLamportSim(64)
    sim.read_topology_text(top)
    sim.read_events_text(events)
    ms, log = sim.lanes_compile_check()
    assert ms > 0 and "error" not in log.lower()
    ms, specialized, log = sim.lanes_program_compile_check()
    assert specialized and ms > 0
    assert "error" not in log.lower()


def test_spill_twin_compiles_on_the_deep_topology():
    """Three nodes, pairs (P,Q) and (R,-), with a channel's worth of spill traffic in the program:
    the generic kernels (the program is over the cap of the specialized ones)."""
    sim = cl.ChandyLamportSim(64, fifo_lds_slots=4)
    sim.read_topology_text(P.DEEP_TOP)
    sim.read_events_text(P.deep_events("Q", "P"))
    ms, log = sim.lanes_compile_check()
    assert ms > 0 and "error" not in log.lower()
    assert not sim.lanes_program_compile_check()[1]
