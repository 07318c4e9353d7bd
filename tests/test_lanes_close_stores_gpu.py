"""Program-specialized lanes kernels without the end-cursor store on the in-links their program
never sends on (cl_lanes.h TokIn: the 0 is in the record since the same launch created it), and
with the broadcast guard's row-end test compiled out where the delay rows hold the program's own
bound on draws (cl_lanes.h Guard, the program type's COVER).

Every case forces the lanes engine, flushes (generic kernels), reads every result, poisons the
output planes, reruns on the program-specialized kernels (asserted) and compares array for array:
status, time, counters, per-instance hashes, completion ticks and collect_snapshot_packed of every
snapshot; final node tokens on a sample.  On poisoned planes a record word that no store of the
rerun wrote reads as 0xA5A5A5A5, so a close store dropped where it was needed shows as a
difference.  A second sim with the program kernels off replays the same inputs on the generic
kernels and must give the same arrays.  The oracle pins status, time, hashes, counters and, on the
sample, final tokens, completion ticks and every snapshot's contents.  Each case runs at
4096 + 17 instances (replays through the slot map, block-major records, a ragged last wave) and
at 64 + 5 (identity order, instance-major records).  All results are integers: equality, no
tolerance.  test_lanes_close_stores_host.py shows in the oracle that each program does what its
case is about.

Reference: node.go:149-171 (HandleMarker), node.go:58-84 (CreateLocalSnapshot), node.go:97-109
(SendToNeighbors), sim.go:100-102 (GetReceiveTime).
"""
import numpy as np
import pytest

import closestorecheck as S
import oracle as O
import tokenlinkcheck as K
from enginecheck import cl

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", S.SIZES)
def test_program_without_a_send_keeps_no_close_store(n):
    """Every in-link is token-free: the rerun has no close store at all, and every record word
    comes from the creation's store."""
    sim, got = S.check(K.T4_TOP, K.NO_SEND_EVENTS, n, S.mixed_rows(n, 48, 61))
    assert (got[0] == O.OK).all()
    assert got[3]["pop_tok"] == 0 and got[3]["completed"] == 2 * n


@pytest.mark.parametrize("n", S.SIZES)
def test_send_on_every_channel_keeps_every_close_store(n):
    sim, got = S.check(K.T4_TOP, K.EVERY_CHANNEL_EVENTS, n, S.mixed_rows(n, 48, 62))
    assert (got[0] == O.OK).all()
    assert got[3]["pop_tok"] == 7 * n


@pytest.mark.parametrize("n", S.SIZES)
def test_token_and_token_free_in_link_share_a_cursor_register(n):
    """I's in-links Y -> I (token-free: no close store) and Z -> I (its close store reads the high
    half of the same cursor register)."""
    sim, got = S.check(K.T4_TOP, K.SHARED_CURSOR_EVENTS, n, S.mixed_rows(n, 48, 63))
    assert (got[0] == O.OK).all()


@pytest.mark.parametrize("n", S.SIZES)
def test_token_free_in_link_closes_in_the_tick_that_created_the_record(n):
    """In the instances whose rows are all zero, Y's record is created by the marker from I and its
    token-free in-link from X closes in the same tick, and so at Z a tick later (closestorecheck):
    those snapshots complete at tick 4."""
    sched = S.mixed_rows(n, 48, 64)
    sim, got = S.check(K.T4_TOP, S.SAME_TICK_CLOSE_EVENTS, n, sched)
    assert (got[0] == O.OK).all()
    zero = ~sched.any(axis=1)
    assert zero.any() and not zero.all()
    assert (sim.snapshot_ticks(0)[zero] == 4).all()


@pytest.mark.parametrize("n", S.SIZES)
def test_every_in_link_of_an_initiator_closes_later(n):
    """I starts both snapshots with both in-links recording: Y -> I closes with a store of its
    cursor, Z -> I without a store."""
    sim, got = S.check(K.T4_TOP, S.INITIATOR_EVENTS, n, S.mixed_rows(n, 48, 65))
    assert (got[0] == O.OK).all()
    assert got[3]["completed"] == 2 * n


@pytest.mark.parametrize("n", S.SIZES)
def test_every_instance_on_the_spill_twin(n):
    """Two ring slots per channel and four packets on X -> Y before the first tick: every instance
    spills to the HBM ring, so the whole replay runs the specialized spill-capable kernel."""
    sim, got = S.check(K.T4_TOP, K.SPILL_EVENTS, n, S.mixed_rows(n, 48, 66), slots=2)
    assert (got[0] == O.OK).all()
    assert sim.replay_split()[0] == n


@pytest.mark.parametrize("n", S.SIZES)
def test_rows_of_exactly_the_programs_draws(n):
    """User rows of cl_delay_draws_needed draws, all zero: the kernels are compiled without the
    guard's row-end test, every push succeeds and the last broadcast's last marker takes the
    row's last delay."""
    sched = np.zeros((n, S.COVER_DRAWS), dtype=np.uint8)
    sim, got = S.check(K.T4_TOP, S.COVER_EVENTS, n, sched, equal_lengths=True)
    assert sim.draws_needed == S.COVER_DRAWS
    assert (got[0] == O.OK).all()
    assert got[3]["completed"] == 2 * n
    assert got[3]["push"] == S.COVER_DRAWS * n   # one draw per push: every draw of the row was taken


@pytest.mark.parametrize("n", S.SIZES)
def test_rows_one_draw_short_of_the_programs_draws(n):
    """One draw fewer: the guard keeps its row-end test, and the last broadcast runs out of delays
    in every instance, as in the oracle."""
    sim, got = S.check(K.T4_TOP, S.COVER_EVENTS, n, S.mixed_rows(n, S.COVER_DRAWS - 1, 68), any_order=True)
    assert sim.draws_needed == S.COVER_DRAWS
    assert (got[0] == cl.INST_DELAY_EXHAUSTED).all()
