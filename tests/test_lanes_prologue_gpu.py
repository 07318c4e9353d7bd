"""The instance-per-lane kernel's prologue: how a lane fetches its delay row (cl_lanes.h program()).

The row's 16-byte chunks are loaded in groups of eight, every load of a group in flight before
the first is used, and a group's chunks past the row's end repeat its last chunk.  A launch reads
the rows either in instance order (a fresh launch) or through the replay plan's slot map, whose
second, spill-capable half starts at a slot that is a multiple of 8 and ends in a ragged wave.
Whatever the loader does, a replay must read the schedule that is current: after appended events
(more draws: longer rows), new seeds, a regenerated delay stream or a changed FIFO limit (another
plan), the next flush()/rerun() equals a sim built from scratch.

Every case forces the lanes engine and compares status, time, counters, checksums,
instance_hashes and CollectSnapshot of a few instances against the CPU oracle and against a
flush-only sim that never replays.

Reference: sim.go:100-102 (GetReceiveTime draws), node.go:97-109 (SendToNeighbors draws in dest
order), test_common.go:79-140 (readEventsFile and its drain).
"""
import numpy as np
import pytest

import oracle as O
from enginecheck import batch_sums_from_oracle, canonical, cl, compare_instance, oracle_batch, oracle_run
from snapcheck import read_text

pytestmark = pytest.mark.gpu

LANES = cl.ChandyLamportSim.ENGINE_LANES
TOP = read_text("8nodes.top")
EVENTS = read_text("8nodes-concurrent-snapshots.events")   # 97 draws: rows of 112 bytes, 7 chunks
# + 19 draws: 116, rows of 128 bytes (one full group of chunks)
MORE = "send N1 N2 1\nsnapshot N3\ntick 3\n"
# + 19 draws: 135, rows of 144 bytes (a group and one chunk of the next)
MORE2 = "send N3 N4 1\nsnapshot N5\ntick 3\n"
# past 4096 the clean instances replay in length order, with a ragged last wave (a split alone maps
# far smaller batches, in index order: test_blocked_ragged_gpu)
N_MAP = 4096 + 37


def new_sim(n, top=TOP, seed_base=O.REFERENCE_SEED, schedule=None, **kw):
    sim = cl.ChandyLamportSim(n, seed_base=seed_base, **kw)
    sim.set_exec_engine(LANES)
    sim.read_topology_text(top)
    if schedule is not None:
        sim.set_delay_schedule(schedule)
    return sim


def feed(sim, text):
    """The events of `text` one by one, without readEventsFile's drain at the end."""
    for ln in text.strip().split("\n"):
        f = ln.split()
        if f[0] == "send":
            sim.ProcessEvent(cl.PassTokenEvent(f[1], f[2], int(f[3])))
        elif f[0] == "snapshot":
            sim.ProcessEvent(cl.SnapshotEvent(f[1]))
        else:
            sim.Tick(int(f[1]) if len(f) > 1 else 1)


def flush_only(n, events, top=TOP, **kw):
    sim = new_sim(n, top=top, **kw)
    sim.read_events_text(events)
    sim.flush()
    assert sim.exec_engine() == LANES
    return sim


class Want:
    """What a batch must compute: the oracle's run of every instance and a flush-only sim."""

    def __init__(self, n, events, top=TOP, seed_base=O.REFERENCE_SEED, schedule=None, **kw):
        self.n, self.events, self.top, self.seed_base, self.schedule = n, events, top, seed_base, schedule
        draws = 0 if schedule is None else schedule.shape[1]
        _, self.status, self.ticks, self.counters, self.hashes = oracle_batch(
            top, events, n, seed_base=seed_base, schedule=schedule, draws=draws)
        self.flat = flush_only(n, events, top=top, seed_base=seed_base, schedule=schedule, **kw)
        bad = np.nonzero(self.status != 0)[0][:3].tolist()
        self.sample = sorted(set([0, 1, 63, 64, n // 2, n - 38, n - 37, n - 1] + bad) & set(range(n)))
        self.refs = {i: (oracle_run(top, events, schedule=schedule[i]) if schedule is not None
                         else oracle_run(top, events, seed=seed_base + i)) for i in self.sample}

    def check(self, sim):
        flat, ok = self.flat, self.status == 0
        status, times = sim.status(), sim.time()
        assert np.array_equal(status, self.status)
        assert np.array_equal(status, flat.status())
        assert np.array_equal(times[ok], self.ticks[ok])
        assert np.array_equal(times, flat.time())
        sums = dict(zip(cl.SUM_NAMES, sim.checksums().tolist()))
        for k, v in batch_sums_from_oracle(self.status, self.counters, self.hashes).items():
            assert sums[k] == v, f"{k}: engine {sums[k]} vs oracle {v}"
        assert np.array_equal(sim.checksums(), flat.checksums())
        assert sim.counters() == flat.counters()
        assert sim.counters(only_ok=True) == flat.counters(only_ok=True)
        hashes = sim.instance_hashes()
        assert np.array_equal(hashes, flat.instance_hashes())
        assert np.array_equal(hashes[ok], self.hashes[ok])
        for i, ref in self.refs.items():
            compare_instance(sim, i, ref, status=status, times=times)
            if status[i] != 0:
                continue
            for sid in range(ref.num_snapshots):
                if not ref.complete(sid):
                    continue
                got, base = sim.CollectSnapshot(sid, instance=i), flat.CollectSnapshot(sid, instance=i)
                assert got.tokenMap == base.tokenMap
                assert canonical(got.messages) == canonical(base.messages)


def replay(sim, want, times=1):
    """rerun() `times` times from poisoned outputs, each checked."""
    for _ in range(times):
        sim.poison_outputs()
        sim.rerun()
        sim.synchronize()
        want.check(sim)


@pytest.fixture(scope="module")
def c3_want():
    return Want(N_MAP, EVENTS)


def test_split_replay_through_the_slot_map_with_a_ragged_last_wave(c3_want):
    """4,096 + 37 instances: about 6 % spill, so replays are split and go through the slot map; the
    second half starts at a multiple of 8 and its last wave has lanes past the batch."""
    sim = new_sim(N_MAP)
    sim.read_events_text(EVENTS)
    sim.flush()
    assert sim.exec_engine() == LANES
    c3_want.check(sim)
    replay(sim, c3_want)
    assert sim.exec_engine() == LANES
    assert sim.mapped_replays() and sim.records_blocked()
    spilled, split = sim.replay_split()
    assert 0 < spilled < N_MAP // 4 and 0 < split < N_MAP
    assert (N_MAP - split) % 64 != 0   # (a ragged last wave in the second half)
    replay(sim, c3_want)               # the second replay of the same plan


def _replayed(n=N_MAP, events=None, feed_events=None, **kw):
    sim = new_sim(n, **kw)
    if feed_events is not None:
        feed(sim, feed_events)
    else:
        sim.read_events_text(events)
    sim.flush()
    for _ in range(2):
        sim.rerun()
    sim.synchronize()
    assert sim.exec_engine() == LANES and sim.mapped_replays()
    return sim


def test_appended_events_change_the_draw_count_after_a_replay():
    """97 draws (rows of 112 bytes) replayed, then a send and a snapshot more: 116 draws, rows of
    128 bytes.  The flush and the replays after it read the new rows."""
    sim = _replayed(feed_events=EVENTS)
    assert sim.draws_needed == 97
    sim.read_events_text(MORE)
    assert sim.draws_needed == 116
    want = Want(N_MAP, EVENTS + MORE)
    sim.flush()
    want.check(sim)
    replay(sim, want, times=2)


def test_new_seeds_after_a_replay(c3_want):
    sim = _replayed(events=EVENTS)
    c3_want.check(sim)
    sim.set_delay_go_seeds(O.REFERENCE_SEED + 100003)
    want = Want(N_MAP, EVENTS, seed_base=O.REFERENCE_SEED + 100003)
    assert not np.array_equal(want.hashes, c3_want.hashes)
    sim.flush()
    want.check(sim)
    replay(sim, want, times=2)


def test_regenerated_delay_stream_after_a_replay(c3_want):
    """The same Go streams made again by the device generator: the same bytes, a new plan."""
    sim = _replayed(events=EVENTS)
    sim.set_delay_generator("device")
    sim.flush()
    assert sim.delay_generator == "device"
    c3_want.check(sim)
    replay(sim, c3_want, times=2)


def test_changed_fifo_limit_rebuilds_the_plan_after_a_replay(c3_want):
    """8 LDS ring slots per channel hold every packet this program pushes on one: nothing spills
    any more, so the plan (split, slot map) is another one; the results are the same."""
    sim = _replayed(events=EVENTS)
    before = sim.replay_split()
    sim.set_limits(fifo_lds_slots=8)
    sim.flush()
    c3_want.check(sim)
    replay(sim, c3_want, times=2)
    assert sim.replay_split() != before
    want8 = Want(N_MAP, EVENTS, fifo_lds_slots=8)
    want8.check(sim)


# ---- a row that ends mid-word, with draws that run out (test_lanes_edges_gpu's hub) ----------

HUB_TOP = "5\nH 100\nA 50\nB 50\nC 50\nD 50\n" + "".join(f"H {x}\n{x} H\n" for x in "ABCD")
HUB_EVENTS = ("send H A 3\nsend H C 1\n"
              "snapshot A\nsnapshot B\nsnapshot C\nsnapshot D\n"
              "tick 2\nsend A H 2\nsend H B 5\nsend D H 4\nsnapshot H\ntick\n")


@pytest.mark.parametrize("draws", [14, 17, 20, 23, 26, 29])
def test_hub_row_ends_mid_word_and_runs_out_in_replays(draws):
    """Rows of `draws` delays (16 or 32 bytes, the last nibble word partly filled) that run out in
    the tick of the hub's four broadcasts: the reads past the row's end are clamped to its last
    word, in the fresh launch and in replays."""
    n = 4096
    rng = np.random.default_rng(draws)
    sched = rng.integers(0, 5, size=(n, draws), dtype=np.uint8)
    sched[:, 2:6] = 0
    want = Want(n, HUB_EVENTS, top=HUB_TOP, schedule=sched)
    assert (want.status != cl.INST_OK).any()
    sim = new_sim(n, top=HUB_TOP, schedule=sched)
    sim.read_events_text(HUB_EVENTS)
    sim.flush()
    assert sim.exec_engine() == LANES
    want.check(sim)
    replay(sim, want, times=2)
    assert sim.exec_engine() == LANES


# ---- rows one chunk apart: a full group of chunks, and a group plus one chunk ---------------

def test_rows_of_a_full_chunk_group_and_of_one_chunk_more():
    """Two programs on one schedule: 116 draws in rows of 128 bytes (eight chunks, exactly one
    group of loads) and 135 draws in rows of 144 bytes (the ninth chunk alone in its group, its
    delays drawn by the last snapshot's markers)."""
    n = 4096 + 37
    rng = np.random.default_rng(135)
    sched = rng.integers(0, 5, size=(n, 135), dtype=np.uint8)
    for events, width in ((EVENTS + MORE, 128), (EVENTS + MORE + MORE2, 135)):
        s = np.ascontiguousarray(sched[:, :width])
        want = Want(n, events, schedule=s)
        assert (want.status == cl.INST_OK).sum() > n // 2
        sim = new_sim(n, schedule=s)
        sim.read_events_text(events)
        assert sim.draws_needed == (116 if width == 128 else 135)
        sim.flush()
        assert sim.exec_engine() == LANES
        want.check(sim)
        replay(sim, want, times=2)


def test_fresh_launch_of_one_wave():
    """64 instances, one flush: no plan yet, the byte rows in instance order."""
    want = Want(64, EVENTS)
    sim = new_sim(64)
    sim.read_events_text(EVENTS)
    sim.flush()
    assert sim.exec_engine() == LANES
    assert not sim.records_blocked()
    want.check(sim)
