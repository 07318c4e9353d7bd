"""CPU checks of the program-specialized instance-per-lane kernels (cl_lanes.h program type P):
the source cl_jit.cpp generates from a sim's topology and program compiles for gfx950 without a
device, a program over the cap reports "generic" instead of failing, and the setter and the query
behave (the GPU runs are test_lanes_program_gpu.py)."""
import pytest

from enginecheck import cl
from snapcheck import read_text


@pytest.mark.parametrize("top,events", [("8nodes.top", "8nodes-concurrent-snapshots.events"),
                                        ("10nodes.top", "10nodes.events")])
def test_program_kernels_compile(top, events):
    """The flagship program (8 nodes, degree 3: groups of sends, 5 snapshot starts, 6 tick ops)
    and the 10-node ring's (degree 1)."""
    sim = cl.ChandyLamportSim(64)
    sim.read_topology_text(read_text(top))
    sim.read_events_text(read_text(events))
    ms, specialized, log = sim.lanes_program_compile_check()
    assert specialized and ms > 0
    assert "error" not in log.lower()


T4_TOP = "4\nI 200\nX 200\nY 200\nZ 200\nI X\nI Y\nI Z\nX Y\nX Z\nY I\nZ I\n"


@pytest.mark.parametrize("events", [
    "".join(f"send {'IXYZ'[k % 4]} {'XYII'[k % 4]} 1\n" for k in range(129)),  # 129 host ops
    "send I X 1\ntick 1\n" * 33,                                                # 34 tick ops with the drain
])
def test_program_over_the_cap_reports_generic(events):
    sim = cl.ChandyLamportSim(64)
    sim.read_topology_text(T4_TOP)
    sim.read_events_text(events)
    ms, specialized, _ = sim.lanes_program_compile_check()
    assert not specialized and ms == 0


def test_program_at_the_cap_is_specialized_with_unknown_dest_and_tail_ops():
    """128 host ops, one of them a send to a node the sender has no link to, the last one after the
    program's last tick op (read_events_text ends in a drain; the snapshot start follows it): still
    a program the kernels describe."""
    ev = "".join(f"send {'IXYZ'[k % 4]} {'XYII'[k % 4]} 1\n" + ("tick 1\n" if k == 40 else "") for k in range(126))
    ev += "send X I 1\n"
    sim = cl.ChandyLamportSim(64)
    sim.read_topology_text(T4_TOP)
    sim.read_events_text(ev)
    sim.StartSnapshot("Z")
    _, specialized, log = sim.lanes_program_compile_check()
    assert specialized and "error" not in log.lower()


def test_program_kernels_setter_and_query():
    sim = cl.ChandyLamportSim(8)
    assert sim.exec_program_kernels() is False       # nothing launched yet
    for m in (sim.PROGRAM_OFF, sim.PROGRAM_ON, sim.PROGRAM_AUTO):
        sim.set_program_kernels(m)
    with pytest.raises(cl.ClSnapError) as err:
        sim.set_program_kernels(5)
    assert err.value.code == cl.E_INVALID


def test_program_compile_check_refuses_what_the_lanes_kernels_do():
    top = "6\nH 9\nA 0\nB 0\nC 0\nD 0\nE 0\n" + "".join(f"H {x}\n{x} H\n" for x in "ABCDE")
    sim = cl.ChandyLamportSim(8)
    sim.read_topology_text(top)
    sim.read_events_text("snapshot H\n")
    with pytest.raises(cl.ClSnapError) as err:
        sim.lanes_program_compile_check()
    assert err.value.code == cl.E_LIMIT
