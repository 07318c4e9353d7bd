"""Replays on the instance-per-lane kernels specialized on the topology AND the program
(cl_lanes.h program type P, send_c / snap_c), against the same sim's generic flush and the oracle.

A replay of a planned program runs kernels in which every send and snapshot start is
straight-line code on its node's registers.  Each case forces the lanes engine and the program
kernels on (set_program_kernels(PROGRAM_ON): the default compiles them only for batches of 2^17
instances and more), flushes -- the first launch is always generic, asserted -- reads every result,
poisons the output planes, reruns, asserts through exec_program_kernels() which kernels ran, and
compares array for array: status, time, counters, per-instance hashes, completion ticks and
collect_snapshot_packed of every snapshot; final node tokens and CollectSnapshot on a sample.  The
oracle pins status, time, hashes, counters and the sample.

The batch is 4096 + 17 instances: the smallest at which a rerun goes through the slot map
(block-major records, asserted), plus a ragged last block.  Only the split case is larger: a
replay's spilling half runs on the lanes spill kernel from one wave per SIMD (65,536 instances).

Reference: node.go:112-131 (SendTokens), sim.go:105-123 and node.go:198-212 (StartSnapshot),
test_common.go:123-137 (drain).
"""
import numpy as np
import pytest

import oracle as O
from enginecheck import cl, compare_instance, oracle_run
from snapcheck import read_text

pytestmark = pytest.mark.gpu

LANES = cl.ChandyLamportSim.ENGINE_LANES
ON = cl.ChandyLamportSim.PROGRAM_ON
N_INST = 4096 + 17
SAMPLE = tuple(range(0, 96)) + (777, 2048, 4095, 4096, 4112)

T4_TOP = "4\nI 20\nX 20\nY 20\nZ 20\nI X\nI Y\nI Z\nX Y\nX Z\nY I\nZ I\n"


def _rows(n, width, seed):
    return np.random.default_rng(seed).integers(0, 5, size=(n, width), dtype=np.uint8)


def _sim(top, events, n, sched=None, slots=None, max_drain=None):
    sim = cl.ChandyLamportSim(n, fifo_lds_slots=slots, max_drain_ticks=max_drain)
    sim.set_exec_engine(LANES)
    sim.set_program_kernels(ON)
    sim.read_topology_text(top)
    if sched is not None:
        sim.set_delay_schedule(sched)
    sim.read_events_text(events)
    return sim


def _outputs(sim):
    out = [sim.status(), sim.time(), sim.checksums(), sim.counters(only_ok=False), sim.counters(only_ok=True),
           sim.instance_hashes()]
    for sid in range(sim.num_snapshots):
        out.append(sim.snapshot_ticks(sid))
        out.extend(sim.collect_snapshot_packed(sid))
    out.append([sim.node_tokens(i) for i in SAMPLE if i < sim.n_instances])
    return out


def _same(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, (dict, list)):
            assert x == y, (what, k)
        else:
            assert np.array_equal(x, y), (what, k)


def _replay(sim, want_spec=True, want_map=True):
    """Generic flush, then a poisoned rerun: returns (flush outputs, rerun outputs)."""
    sim.flush()
    assert sim.exec_engine() == LANES and not sim.exec_program_kernels()   # a first launch is generic
    gen = _outputs(sim)
    sim.poison_outputs()
    sim.rerun()
    sim.synchronize()
    assert sim.exec_engine() == LANES
    assert sim.exec_program_kernels() == want_spec
    if want_map:
        assert sim.mapped_replays() and sim.records_blocked()
    spec = _outputs(sim)
    _same(spec, gen, "program-specialized rerun vs generic flush")
    return gen, spec


def _against_oracle(sim, got, top, events, n, sched=None, max_drain=O.MAX_DRAIN_TICKS, sample=SAMPLE):
    _, st, ticks, cnt, hashes = O.run_batch(top, events, n, sched=sched, draws=0 if sched is None else sched.shape[1],
                                            threads=8, max_drain=max_drain)
    ok = st == 0
    status, times = got[0], got[1]
    assert np.array_equal(status, st)
    assert np.array_equal(times[ok], ticks[ok])
    assert np.array_equal(got[5][ok], hashes[ok])
    c = got[4]
    assert c["recorded"] == cnt[ok, 4].sum() and c["completed"] == cnt[ok, 6].sum()
    if ok.all():
        c = got[3]
        assert (c["push"], c["peek"], c["pop_tok"], c["pop_mk"]) == tuple(cnt[:, k].sum() for k in range(4))
    for i in sample:
        ref = oracle_run(top, events, seed=O.REFERENCE_SEED + i, schedule=None if sched is None else sched[i],
                         max_drain=max_drain)
        compare_instance(sim, i, ref, status=status, times=times)
    return st


def _check(top, events, n=N_INST, sched=None, slots=None, max_drain=None, want_spec=True, want_map=True,
           sample=SAMPLE):
    sim = _sim(top, events, n, sched, slots, max_drain)
    _, spec = _replay(sim, want_spec, want_map)
    st = _against_oracle(sim, spec, top, events, n, sched, O.MAX_DRAIN_TICKS if max_drain is None else max_drain,
                         sample)
    return sim, st


def test_c3_program_block_major():
    """The flagship program: 8 sends (two groups), 5 snapshot starts, 6 tick segments."""
    _, st = _check(read_text("8nodes.top"), read_text("8nodes-concurrent-snapshots.events"))
    assert (st == O.OK).sum() > N_INST // 2   # (a few Go delay streams leave a sender short: the oracle's statuses)


def test_insufficient_tokens_part_way():
    """I holds 20 tokens and sends 25 after two ticks: possible only where Y's 10 arrived by then.
    The other instances freeze INSUFFICIENT at that op, and the snapshot, sends and ticks after it
    are no-ops for them while their neighbours in the wave go on."""
    ev = "send Y I 10\nsnapshot X\ntick 2\nsend I X 25\nsnapshot Z\nsend X Z 3\ntick 1\nsend Z I 2\n"
    _, st = _check(T4_TOP, ev, sched=_rows(N_INST, 24, 11))
    assert 0 < (st == cl.INST_FATAL_INSUFFICIENT_TOKENS).sum() < N_INST and (st == O.OK).any()


def test_unknown_destination_part_way():
    """X has no link to I: every instance freezes UNKNOWN_DEST there, after a snapshot and a tick
    loop ran and before a further snapshot start, sends and ticks that must change nothing."""
    ev = "send I X 4\nsnapshot Y\ntick 1\nsend X I 1\nsnapshot I\nsend I Y 2\ntick 2\n"
    # (every instance ends at the same tick: the plan keeps the identity slot order, no map)
    _, st = _check(T4_TOP, ev, sched=_rows(N_INST, 24, 12), want_map=False)
    assert (st == cl.INST_FATAL_UNKNOWN_DEST).all()


def test_send_group_and_two_sends_from_one_sender():
    """Sends from I, X, Y fold into one OP_SENDS group; the next two are I's again (a sender twice
    in one segment, two links and then one link twice)."""
    ev = ("send I X 1\nsend X Y 2\nsend Y I 3\nsend I Y 4\nsend I Y 5\nsend I Z 1\nsnapshot X\ntick 2\n"
          "send Z I 2\nsend Y I 1\nsend Y I 2\nsnapshot I\n")
    _, st = _check(T4_TOP, ev, sched=_rows(N_INST, 40, 13))
    assert (st == O.OK).all()


# S has no in-link, K no out-link
SINK_TOP = "4\nA 9\nB 9\nM 9\nK 9\nA B\nB A\nA M\nM A\nB M\nM K\nA K\n"
SRC_SINK_TOP = "4\nS 9\nA 9\nB 9\nK 9\nS A\nS B\nA B\nB A\nA K\nB K\n"


def test_ten_snapshots_and_a_sink():
    """More than 8 snapshot ids (two pending words per node), on a topology with a node of
    out-degree 0, which receives every marker and broadcasts to nobody."""
    ev = "send A K 2\nsend M K 1\n" + "".join(f"snapshot {x}\ntick 1\nsend {x} {y} 1\n"
                                               for x, y in zip("ABMABMABMA", "MAKBMABAAK"))
    sim, st = _check(SINK_TOP, ev, sched=_rows(N_INST, 120, 14))
    assert sim.num_snapshots == 10 and (st == O.OK).all()


def test_starts_at_a_source_and_at_a_sink():
    """A snapshot started at a node without in-links (pending nibble 15: never checked for
    completion) and one started at a node without out-links (no broadcast, no draw): neither can
    complete, the drain ends in HANG; a third, from A, does not reach S either."""
    ev = "send S A 1\nsnapshot S\ntick 1\nsnapshot K\nsend A K 1\ntick 2\nsnapshot A\n"
    _, st = _check(SRC_SINK_TOP, ev, sched=_rows(N_INST, 40, 15), max_drain=24, want_map=False)  # (equal lengths)
    assert (st == cl.INST_HANG).all()


def test_drain_hangs_in_some_instances():
    """A drain of at most 9 ticks: enough where the markers travel fast, HANG elsewhere; the
    instances that finish tick the drain's extra ticks."""
    ev = "send I X 2\nsnapshot I\ntick 1\nsend X Y 1\nsnapshot Y\n"
    _, st = _check(T4_TOP, ev, sched=_rows(N_INST, 40, 16), max_drain=9)
    assert 0 < (st == cl.INST_HANG).sum() < N_INST and (st == O.OK).any()


def test_split_replay_runs_both_specialized_twins():
    """Two ring slots per channel.  X -> Y takes two tokens, one tick, then X's marker: it spills to
    the HBM ring wherever the first token was not delivered in that tick (4 delays of 5) and fits
    the ring elsewhere.  At 2^17 instances the spilling half is over a wave per SIMD, so the
    split replay runs it on the specialized spill-capable kernel beside the spill-free one."""
    n = (1 << 17) + 17
    ev = "send X Y 1\nsend X Y 2\ntick 1\nsnapshot X\ntick 1\nsend I Y 1\n"
    sched = _rows(n, 16, 17)
    sim = _sim(T4_TOP, ev, n, sched, slots=2)
    _, spec = _replay(sim)
    spilled, split = sim.replay_split()
    assert spilled >= 65536 and 0 < split < n
    sample = SAMPLE + (n - 1, n - 18, 70000)
    st = _against_oracle(sim, spec, T4_TOP, ev, n, sched, sample=sample)
    assert (st == O.OK).all()


@pytest.mark.parametrize("width", [2, 3])
def test_row_runs_out_in_a_snapshot_start(width):
    """"snapshot I" broadcasts on three links.  Width 3: the row ends exactly at its last link
    (the guard holds) and the receivers' broadcasts run out.  Width 2: the guard fails, the first
    two links land through push() and the third is DELAY_EXHAUSTED."""
    _, st = _check(T4_TOP, "snapshot I\n", sched=_rows(N_INST, width, 18 + width))
    assert (st == cl.INST_DELAY_EXHAUSTED).all()


def test_two_programs_one_topology_and_appended_ops():
    """Two sims with one topology and different programs get kernels of their own (one more
    compile each, none on a second replay).  Ops appended after a specialized replay run through
    a generic flush from the start and the next replay through kernels of the longer program."""
    ev_a = "send I X 2\nsnapshot X\ntick 2\nsend X Z 1\n"
    ev_b = "send I X 2\nsnapshot Y\ntick 2\nsend X Z 1\n"
    more = "send Z I 3\nsnapshot I\n"
    sched = _rows(N_INST, 60, 21)
    sims = []
    for ev in (ev_a, ev_b):
        c0 = cl.jit_stats()[1]
        sim = _sim(T4_TOP, ev, N_INST, sched)
        _, spec = _replay(sim)
        c1 = cl.jit_stats()[1]
        assert c1 > c0                       # this program's kernels (and, once, the topology's)
        _against_oracle(sim, spec, T4_TOP, ev, N_INST, sched)
        sim.rerun()
        sim.synchronize()
        assert sim.exec_program_kernels() and cl.jit_stats()[1] == c1
        sims.append(sim)
    sim = sims[0]
    sim.read_events_text(more)
    sim.flush()                              # generic (asserted in _replay), from the program's start
    c2 = cl.jit_stats()[1]
    gen, spec = _replay(sim)                 # the rerun: the longer program's kernels, one compile
    assert cl.jit_stats()[1] == c2 + 1
    status, times = spec[0], spec[1]
    for i in SAMPLE:
        ref = O.OracleSim()
        ref.use_schedule(sched[i])
        assert ref.read_topology_text(T4_TOP) == 0
        assert ref.read_events_text(ev_a) >= 0 and ref.read_events_text(more) >= 0
        compare_instance(sim, i, ref, status=status, times=times)
    # the other sim's program still replays on its own kernels
    sims[1].rerun()
    sims[1].synchronize()
    assert sims[1].exec_program_kernels() and cl.jit_stats()[1] == c2 + 1


def test_host_ops_after_the_last_tick_op():
    """A snapshot start after the program's final drain: the arm of host ops that no tick loop
    follows.  Its record and its markers' queue entries are there, nothing is delivered."""
    ev = "send I X 2\nsnapshot X\n"
    sched = _rows(N_INST, 24, 23)
    sim = _sim(T4_TOP, ev, N_INST, sched)
    assert sim.StartSnapshot("I") == 1
    _, spec = _replay(sim)
    status, times = spec[0], spec[1]
    assert (status == O.OK).all()
    for i in SAMPLE:
        ref = O.OracleSim()
        ref.use_schedule(sched[i])
        assert ref.read_topology_text(T4_TOP) == 0 and ref.read_events_text(ev) >= 0
        assert ref.start_snapshot("I") == (0, 1)
        compare_instance(sim, i, ref, status=status, times=times)


def test_program_over_the_cap_replays_generic():
    """130 sends and a snapshot start are over the cap of 128 host ops: the replay runs the generic
    kernels, with the same results."""
    top = T4_TOP.replace(" 20\n", " 200\n")
    ev = "".join(f"send {'IXYZ'[k % 4]} {'XYII'[k % 4]} 1\n" + ("tick 1\n" if k % 8 == 7 else "") for k in range(130))
    ev += "snapshot I\n"
    _, st = _check(top, ev, sched=_rows(N_INST, 144, 22), want_spec=False)
    assert (st == O.OK).all()
