"""CPU checks for test_lanes_close_stores_gpu.py: the program-specialized lanes kernels of every
program of its cases compile for gfx950 without a device -- both twins and both record layouts,
with the broadcast guard's row-end test compiled out (rows that hold the program's bound on draws:
Go rows, or a schedule of exactly that many) and compiled in (a schedule one draw shorter) -- and
the oracle shows that each program does what its case is about."""
import numpy as np
import pytest

import closestorecheck as S
import oracle as O
import tokenlinkcheck as K
from enginecheck import canonical, cl, oracle_run

IDS = [c[0] for c in S.COMPILE_CASES]
ZEROS = np.zeros(48, dtype=np.uint8)


def _sim(top, events, slots):
    sim = cl.ChandyLamportSim(64, fifo_lds_slots=slots)
    sim.read_topology_text(top)
    sim.read_events_text(events)
    return sim


def _compiles(sim, cover):
    """The program kernels compile, with the guard's row-end test compiled out (cover) or in."""
    assert not sim.exec_program_cover()   # (nothing compiled yet)
    ms, specialized, log = sim.lanes_program_compile_check()
    assert specialized and ms > 0
    assert "error" not in log.lower()
    assert sim.exec_program_cover() == cover


@pytest.mark.parametrize("rows", ["go", "short"])
@pytest.mark.parametrize("top,events,slots", [c[1:] for c in S.COMPILE_CASES], ids=IDS)
def test_program_kernels_compile(top, events, slots, rows):
    sim = _sim(top, events, slots)
    if rows == "short":   # (every program here draws at least 7 delays)
        sim.set_delay_schedule(np.zeros((64, sim.draws_needed - 1), dtype=np.uint8))
    _compiles(sim, cover=rows == "go")


def test_program_kernels_compile_on_a_schedule_of_exactly_the_bound():
    sim = _sim(K.T4_TOP, S.COVER_EVENTS, S.SLOTS)
    sim.set_delay_schedule(np.zeros((64, S.COVER_DRAWS), dtype=np.uint8))
    _compiles(sim, cover=True)


def test_draw_bound_of_the_cover_program():
    assert _sim(K.T4_TOP, S.COVER_EVENTS, S.SLOTS).draws_needed == S.COVER_DRAWS


def test_oracle_every_program_completes_on_full_rows():
    rows = np.random.default_rng(11).integers(0, 5, size=(16, 48), dtype=np.uint8)
    for name, top, events, _ in S.COMPILE_CASES:
        for i in range(16):
            ref = oracle_run(top, events, schedule=rows[i])
            assert ref.status == O.OK, name
            assert all(ref.complete(sid) for sid in range(ref.num_snapshots)), name


def test_oracle_no_send_records_no_message():
    ref = oracle_run(K.T4_TOP, K.NO_SEND_EVENTS, schedule=ZEROS)
    assert ref.num_snapshots == 2
    assert all(not ref.collect(sid).messages for sid in range(2))


def test_oracle_same_tick_close_on_zero_rows():
    """closestorecheck's account of the zero-delay run: the snapshot completes at tick 4, which
    needs Z's record created and its in-link from X closed by tick 3 and Y's by tick 2; the token
    sent ahead is the only recorded message."""
    ref = oracle_run(K.T4_TOP, S.SAME_TICK_CLOSE_EVENTS, schedule=ZEROS)
    assert ref.status == O.OK and ref.completion_tick(0) == 4
    assert canonical(ref.collect(0).messages) == {("Z", "I"): [1]}


def test_oracle_initiator_records_on_its_token_link_only():
    seen = set()
    for seed in range(8):
        rows = np.random.default_rng(seed).integers(0, 5, size=48, dtype=np.uint8)
        ref = oracle_run(K.T4_TOP, S.INITIATOR_EVENTS, schedule=rows)
        assert ref.status == O.OK and ref.num_snapshots == 2
        for sid in range(2):
            seen |= set(canonical(ref.collect(sid).messages))
    assert seen == {("Y", "I")}


def test_oracle_cover_program_takes_exactly_its_bound():
    """With COVER_DRAWS draws every push succeeds and both snapshots complete; with one fewer the
    run ends in DELAY_EXHAUSTED: the last draw of the full row is needed, and it is the last."""
    n = 8
    rows = S.mixed_rows(n, S.COVER_DRAWS, 3)
    rows[0] = 0
    _, st, _, cnt, _ = O.run_batch(K.T4_TOP, S.COVER_EVENTS, n, sched=rows, draws=S.COVER_DRAWS, threads=2)
    assert (st == O.OK).all() and (cnt[:, 0] == S.COVER_DRAWS).all() and (cnt[:, 6] == 2).all()
    short = np.ascontiguousarray(rows[:, :S.COVER_DRAWS - 1])
    _, st, _, _, _ = O.run_batch(K.T4_TOP, S.COVER_EVENTS, n, sched=short, draws=S.COVER_DRAWS - 1, threads=2)
    assert (st == cl.INST_DELAY_EXHAUSTED).all()
