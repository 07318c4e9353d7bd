"""Program-specialized lanes kernels without a token path on the in-links their program never
sends on (cl_lanes.h TokIn), and the edges of the per-tick completion check over the nodes'
pending words (two words, two snapshots in one tick, the sentinel of an initiator without in-links).

Every case forces the lanes engine, flushes (generic kernels), reads every result, poisons the
output planes, reruns on the program-specialized kernels (asserted) and compares array for array:
status, time, counters (the token and marker pop counts among them), per-instance hashes,
completion ticks and collect_snapshot_packed of every snapshot; final node tokens on a sample.  A
second sim with the program kernels off replays the same inputs on the generic kernels and must
give the same arrays.  The oracle pins status, time, hashes, counters and, on the sample, final
tokens, completion ticks and every snapshot's contents.  Each case runs at 4096 + 17 instances
(replays through the slot map, block-major records, a ragged last wave) and at 64 + 5 (identity
order, instance-major records).  All results are integers: equality, no tolerance.

Reference: node.go:149-185 (HandleMarker, HandleToken), node.go:58-84 (CreateLocalSnapshot),
sim.go:126-131 (NotifyCompletedSnapshot), test_common.go:123-137 (drain).
"""
import numpy as np
import pytest

import oracle as O
import tokenlinkcheck as K
from enginecheck import canonical, cl, compare_instance, oracle_run

pytestmark = pytest.mark.gpu

LANES = cl.ChandyLamportSim.ENGINE_LANES
ON, OFF = cl.ChandyLamportSim.PROGRAM_ON, cl.ChandyLamportSim.PROGRAM_OFF
SIZES = [4096 + 17, 64 + 5]
SLOTS = 8   # ring slots per channel above every channel's packet count: nothing spills


def _rows(n, width, seed):
    """Delay rows: an instance draws either 0 throughout or uniformly from 0..4.  The two kinds end
    their drains far enough apart that the planner orders the large batch by length, so its
    replays go through the slot map."""
    rng = np.random.default_rng(seed)
    hi = rng.choice([1, 5], size=(n, 1))
    return (rng.integers(0, 5, size=(n, width)) % hi).astype(np.uint8)


def _sample(n):
    return tuple(i for i in tuple(range(0, 80)) + (777, 2048, 4095, 4096, 4112) if i < n)


def _sim(top, events, n, sched, mode, slots=SLOTS, max_drain=None, extra=None):
    sim = cl.ChandyLamportSim(n, fifo_lds_slots=slots, max_drain_ticks=max_drain)
    sim.set_exec_engine(LANES)
    sim.set_program_kernels(mode)
    sim.read_topology_text(top)
    sim.set_delay_schedule(sched)
    sim.read_events_text(events)
    if extra:
        sim.ProcessEvent(cl.PassTokenEvent(*extra))
    return sim


def _outputs(sim):
    out = [sim.status(), sim.time(), sim.checksums(), sim.counters(only_ok=False), sim.counters(only_ok=True),
           sim.instance_hashes()]
    for sid in range(sim.num_snapshots):
        out.append(sim.snapshot_ticks(sid))
        out.extend(sim.collect_snapshot_packed(sid))
    out.append([sim.node_tokens(i) for i in _sample(sim.n_instances)])
    return out


def _same(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, (dict, list)):
            assert x == y, (what, k)
        else:
            assert np.array_equal(x, y), (what, k)


def _replay(sim, spec, mapped):
    """Generic flush, then a poisoned rerun: the rerun's outputs, equal to the flush's."""
    sim.flush()
    assert sim.exec_engine() == LANES and not sim.exec_program_kernels()   # a first launch is generic
    gen = _outputs(sim)
    sim.poison_outputs()
    sim.rerun()
    sim.synchronize()
    assert sim.exec_engine() == LANES and sim.exec_program_kernels() == spec
    assert sim.mapped_replays() == mapped and sim.records_blocked() == mapped
    out = _outputs(sim)
    _same(out, gen, "rerun vs generic flush")
    return out


def _check(top, events, n, seed, width=48, slots=SLOTS, max_drain=None, extra=None, equal_lengths=False):
    """Both sims, the oracle's batch (not with an extra event: the sample alone) and the sample.
    Returns (specialized sim, its outputs, the delay rows)."""
    sched = _rows(n, width, seed)
    mapped = n >= 4096 and not equal_lengths   # (instances of one length keep the identity order)
    sim = _sim(top, events, n, sched, ON, slots, max_drain, extra)
    got = _replay(sim, True, mapped)
    off = _sim(top, events, n, sched, OFF, slots, max_drain, extra)
    _same(_replay(off, False, mapped), got, "program kernels off vs on")
    md = O.MAX_DRAIN_TICKS if max_drain is None else max_drain
    status, times = got[0], got[1]
    if extra is None:
        _, st, ticks, cnt, hashes = O.run_batch(top, events, n, sched=sched, draws=width, threads=8, max_drain=md)
        ok = st == 0
        assert np.array_equal(status, st)
        assert np.array_equal(times[ok], ticks[ok])
        assert np.array_equal(got[5][ok], hashes[ok])
        c = got[4]
        assert c["recorded"] == cnt[ok, 4].sum() and c["completed"] == cnt[ok, 6].sum()
        if ok.all():
            c = got[3]
            assert (c["push"], c["peek"], c["pop_tok"], c["pop_mk"]) == tuple(cnt[:, k].sum() for k in range(4))
    for i in _sample(n):
        ref = oracle_run(top, events, schedule=sched[i], max_drain=md)
        if extra:
            ref.send_tokens(*extra)
        compare_instance(sim, i, ref, status=status, times=times)
    return sim, got, sched


@pytest.mark.parametrize("n", SIZES)
def test_token_and_token_free_in_link_share_a_cursor_register(n):
    """I's in-links Y -> I and Z -> I are the halves of one cursor register; only Z -> I carries
    tokens.  I's record of snapshot 0 (I initiates) has a begin cursor of 1 and a larger end cursor
    on Z -> I, zeros on Y -> I; its record of snapshot 1 is created by the marker on Y -> I."""
    sim, got, sched = _check(K.T4_TOP, K.SHARED_CURSOR_EVENTS, n, 41)
    assert (got[0] == O.OK).all()
    for i in range(8):   # the condition, in the oracle
        ref = oracle_run(K.T4_TOP, K.SHARED_CURSOR_EVENTS, schedule=sched[i])
        rec0 = canonical(ref.collect(0).messages)
        assert list(rec0) == [("Z", "I")] and rec0[("Z", "I")][:2] == [2, 1]   # after the first token (cursor 1)
        assert set(canonical(ref.collect(1).messages)) <= {("Z", "I")}
    assert any(canonical(oracle_run(K.T4_TOP, K.SHARED_CURSOR_EVENTS, schedule=sched[i]).collect(1).messages)
               for i in range(8))


@pytest.mark.parametrize("n", SIZES)
def test_degree_four_receiver_with_mixed_in_links(n):
    """R's record is 8 words in two 16-byte stores; of its four in-links A -> R and E -> R carry
    tokens (one half of each cursor register), B -> R and C -> R none.  Snapshot 0 reaches R on the
    token-free B -> R, snapshot 1 starts at R with all four recording."""
    sim, got, sched = _check(K.STAR_TOP, K.STAR_EVENTS, n, 42)
    assert (got[0] == O.OK).all()
    seen = set()
    for i in range(8):
        ref = oracle_run(K.STAR_TOP, K.STAR_EVENTS, schedule=sched[i])
        for sid in (0, 1):
            seen |= set(canonical(ref.collect(sid).messages))
    assert seen == {("A", "R"), ("E", "R"), ("R", "B")}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", ["no_send", "every_channel"])
def test_no_token_link_and_all_token_links(case, n):
    """A program without a send (every in-link token-free, every cursor word a constant) and one
    with a send on each of the seven channels (the token path everywhere, as in the generic
    kernels)."""
    events = K.NO_SEND_EVENTS if case == "no_send" else K.EVERY_CHANNEL_EVENTS
    sim, got, _ = _check(K.T4_TOP, events, n, 43)
    assert (got[0] == O.OK).all()
    pops = got[3]["pop_tok"]
    assert pops == (0 if case == "no_send" else 7 * n)


@pytest.mark.parametrize("n", SIZES)
def test_only_send_of_a_channel_after_the_last_tick_op(n):
    """Y -> I's only send is an event after the program's drain: it stands in the arm of host ops
    that no tick loop follows, and still makes Y -> I a token link.  The token stays queued."""
    sim, got, _ = _check(K.T4_TOP, K.LAST_ARM_EVENTS, n, 44, extra=K.LAST_ARM_SEND)
    assert (got[0] == O.OK).all()
    assert got[3]["push"] - got[3]["pop_tok"] - got[3]["pop_mk"] == n   # one packet queued per instance


@pytest.mark.parametrize("n", SIZES)
def test_send_that_fails_for_insufficient_tokens(n):
    """"send I X 25" fails wherever Y's 10 tokens have not arrived by then: those instances freeze
    INSUFFICIENT (I -> X stays a token link of the program), their neighbours in the wave go on."""
    sim, got, _ = _check(K.T4_TOP, K.INSUFFICIENT_EVENTS, n, 45)
    st = got[0]
    assert 0 < (st == cl.INST_FATAL_INSUFFICIENT_TOKENS).sum() < n and (st == O.OK).any()
    assert ((st == O.OK) | (st == cl.INST_FATAL_INSUFFICIENT_TOKENS)).all()


@pytest.mark.parametrize("n", SIZES)
def test_send_to_an_unknown_destination(n):
    """X has no link to I: the send names no channel, every instance freezes UNKNOWN_DEST there."""
    sim, got, _ = _check(K.T4_TOP, K.UNKNOWN_DEST_EVENTS, n, 46, equal_lengths=True)
    assert (got[0] == cl.INST_FATAL_UNKNOWN_DEST).all()


@pytest.mark.parametrize("n", SIZES)
def test_send_group(n):
    """One event line per node: the four sends fold into one OP_SENDS group, and each counts for
    its channel."""
    sim, got, _ = _check(K.T4_TOP, K.GROUP_EVENTS, n, 47)
    assert (got[0] == O.OK).all()


@pytest.mark.parametrize("n", SIZES)
def test_every_instance_on_the_spill_twin(n):
    """Two ring slots per channel and four packets on X -> Y before the first tick: every instance
    spills to the HBM ring, so the whole replay runs the specialized spill-capable kernel."""
    sim, got, _ = _check(K.T4_TOP, K.SPILL_EVENTS, n, 48, slots=2)
    assert (got[0] == O.OK).all()
    assert sim.replay_split()[0] == n


@pytest.mark.parametrize("n", SIZES)
def test_ten_snapshots_use_both_pending_words(n):
    """More than 8 snapshot ids: the completion check tests two pending words per node."""
    sim, got, _ = _check(K.SINK_TOP, K.TEN_SNAPSHOTS_EVENTS, n, 49, width=120)
    assert sim.num_snapshots == 10 and (got[0] == O.OK).all()
    assert got[3]["completed"] == 10 * n


@pytest.mark.parametrize("n", SIZES)
def test_two_snapshots_complete_in_the_same_tick(n):
    """Two nodes, a snapshot started at each: where a row's delays are equal both complete in one
    tick (two fresh bits of one pending word), elsewhere in different ticks."""
    sim, got, sched = _check(K.PAIR_TOP, K.SAME_TICK_EVENTS, n, 50)
    assert (got[0] == O.OK).all()
    refs = [oracle_run(K.PAIR_TOP, K.SAME_TICK_EVENTS, schedule=sched[i]) for i in range(32)]
    same = [r.completion_tick(0) == r.completion_tick(1) for r in refs]
    assert any(same) and not all(same)
    t0, t1 = sim.snapshot_ticks(0), sim.snapshot_ticks(1)
    assert [bool(a == b) for a, b in zip(t0[:32], t1[:32])] == same


@pytest.mark.parametrize("n", SIZES)
def test_initiator_without_in_links_never_completes(n):
    """S has no in-link (pending nibble 15): its snapshot never completes, nor does A's, which
    cannot reach S; the drain ends in HANG after its 24 ticks in every instance."""
    sim, got, _ = _check(K.SOURCE_TOP, K.SOURCE_EVENTS, n, 51, max_drain=24, equal_lengths=True)
    assert (got[0] == cl.INST_HANG).all()
    assert got[3]["completed"] == 0
