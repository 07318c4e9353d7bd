"""The node-parallel kernel (cl_kernels.hip) at the limits of its packed words, against the oracle.

The kernel keeps a FIFO entry in one word -- marker bit, 15-bit receiveTime (kMaxTime = 32759),
16-bit payload -- and a link in two half-words: 8-bit ring head | 8-bit queued count (kMaxQueued =
255) and a 16-bit recording cursor (cl_engine.h:33-51).  The unrolled kernels (degree bound <= 4)
hold two head half-words per register and bump a count with a bare add; packets beyond the LDS ring
(2-8 slots under automatic sizing) live in an HBM spill ring whose head is reset lazily.  The
reference scenarios stay far from all of it (payloads <= 200, time < 600, depth ~10).  These tests
drive the kernel, forced with ENGINE_NODES, to each limit and one step past it:

* 255 packets queued on one channel (the even and the odd half of a shared head register, heads in
  LDS for degree bounds 8 and 16), and the 256th push -- a single send, a send inside an OP_SENDS
  group, a StartSnapshot's marker, a marker broadcast inside a tick -- which must freeze the instance
  with INST_FIFO_OVERFLOW at the time of that push and leave its wave-mates alone;
* the spill ring: 700 pushes through its 256 slots, a restart after the channel drained into the
  LDS ring, state images saved with live ring contents, rings filled with no slack;
* payloads of 65535 and 32768, simulated time 32759, recording cursors past 256 and 4096.

Every test compares bit for bit with the CPU oracle and asserts, on the oracle's side
(depthcheck.walk), that the regime it names was reached.  The queue of the reference is unbounded
(queue.go:6-28): the expected overflow status and its time are depthcheck's.

Reference: sim.go:71-95 (Tick), sim.go:100-102 (GetReceiveTime), sim.go:105-123 (StartSnapshot),
node.go:97-131 (SendToNeighbors, SendTokens), node.go:149-171 (HandleMarker), queue.go:6-28.
"""
import functools

import numpy as np
import pytest

import depthcheck as D
import oracle as O
import selectcheck
import statscheck
from enginecheck import cl, compare_instance, oracle_batch

pytestmark = pytest.mark.gpu

NODES = cl.ChandyLamportSim.ENGINE_NODES
LANES = cl.ChandyLamportSim.ENGINE_LANES
OVERFLOW = cl.INST_FIFO_OVERFLOW
SEED = O.REFERENCE_SEED

# degree 2: the unrolled kernel, both head words of A in one register (A -> B the even half)
TOP3 = "3\nA 30000\nB 0\nC 0\nA B\nA C\nB A\nC A\n"
# a hub with 5 leaves: degree bound 8, head words in LDS
_L5 = [f"L{k}" for k in range(5)]
HUB5_TOP = "6\nH 30000\n" + "".join(f"{x} 0\n" for x in _L5) + "".join(f"H {x}\n{x} H\n" for x in _L5)
# the 10-leaf hub of test_rec_blocked_gpu.py: degree bound 16, 3-word records, 40 tokens at H
_L10 = [f"L{k}" for k in range(10)]
HUB10_TOP = (f"{len(_L10) + 1}\nH 40\n" + "".join(f"{x} 5\n" for x in _L10) + "".join(f"H {x}\n" for x in _L10)
             + "".join(f"{_L10[k]} {_L10[(k + 1) % 10]}\n" for k in range(10)) + "L0 H\n")


# ---- drivers ------------------------------------------------------------------------------------

def make_sim(top, n, schedule=None, engine=NODES, **kw):
    sim = cl.ChandyLamportSim(n, seed_base=SEED, **kw)
    sim.set_exec_engine(engine)
    sim.read_topology_text(top)
    if schedule is not None:
        sim.set_delay_schedule(schedule)
    return sim


def one_shot(top, events, n, schedule=None, engine=NODES, **kw):
    """readEventsFile of `events` (with its drain) in one launch."""
    sim = make_sim(top, n, schedule, engine, **kw)
    sim.read_events_text(events)
    sim.flush()
    assert sim.exec_engine() == engine
    return sim


def feed(sim, lines, drain, engine=NODES):
    """The events through ProcessEvent / Tick, flushing at every "|" line and at the end."""
    for ln in lines:
        f = ln.split()
        if ln == "|":
            sim.flush()
            assert sim.exec_engine() == engine
        elif f[0] == "send":
            sim.ProcessEvent(cl.PassTokenEvent(f[1], f[2], int(f[3])))
        elif f[0] == "snapshot":
            sim.ProcessEvent(cl.SnapshotEvent(f[1]))
        else:
            sim.Tick(int(f[1]) if len(f) > 1 else 1)
    if drain:
        sim.drain()
    sim.flush()
    assert sim.exec_engine() == engine
    return sim


def text_of(lines):
    return "".join(ln + "\n" for ln in lines if ln != "|")


@functools.lru_cache(maxsize=None)
def _walks(top, events, n, sched_bytes, drain, in_tick):
    if sched_bytes is None:
        return [D.walk(top, events, seed=SEED + i, drain=drain, in_tick=in_tick) for i in range(n)]
    sched = np.frombuffer(sched_bytes, dtype=np.uint8).reshape(n, -1)
    return [D.walk(top, events, schedule=sched[i], drain=drain, in_tick=in_tick) for i in range(n)]


def walks(top, events, n, schedule=None, drain=True, in_tick=False):
    """One depthcheck walk per instance, under Go seed SEED + i or row i of an explicit schedule
    (computed once per program and shared by the cases that run it)."""
    return _walks(top, events, n, None if schedule is None else schedule.tobytes(), drain, in_tick)


def total_tokens(top):
    f = top.split()
    return sum(int(x) for x in f[2:1 + 2 * int(f[0]):2])


def sums_of(sim):
    return dict(zip(cl.SUM_NAMES, sim.checksums().tolist()))


def check(sim, top, ws):
    """Every instance against its walk: an instance the walk saw overflow reports
    INST_FIFO_OVERFLOW and the oracle's time at the failing push; every other one equals the
    oracle in full.  The checksums count the two classes and the tokens still queued."""
    status, times = sim.status(), sim.time()
    n_over, in_flight = 0, 0
    for i, w in enumerate(ws):
        if w.overflow is None:
            compare_instance(sim, i, w.ref, status=status, times=times)
            in_flight += total_tokens(top) - sum(w.ref.node_tokens().values())
        else:
            assert status[i] == OVERFLOW, f"instance {i}: status {status[i]}, the oracle overflows at {w.overflow}"
            assert times[i] == w.overflow[1], \
                f"instance {i}: frozen at {times[i]}, the oracle's push is at {w.overflow[1]}"
            n_over += 1
    s = sums_of(sim)
    assert (s["instances"], s["ok"], s["fatal"], s["other"]) == (len(ws), len(ws) - n_over, 0, n_over)
    assert s["cut_residual"] == 0 and s["final_residual"] == 0
    assert s["in_flight"] == in_flight
    return n_over


def check_counters(sim, top, events, n, schedule=None):
    """The batch counters and per-instance hashes against the oracle's run of every instance."""
    draws = 0 if schedule is None else schedule.shape[1]
    _, st, ticks, cnt, hashes = oracle_batch(top, events, n, schedule=schedule, draws=draws)
    assert (st == O.OK).all()
    got = sim.counters(only_ok=False)
    for k, col in (("push", 0), ("peek", 1), ("pop_tok", 2), ("pop_mk", 3)):
        assert got[k] == cnt[:, col].sum(), k
    assert got["ticks"] == ticks.sum()
    got_ok = sim.counters(only_ok=True)
    assert got_ok["recorded"] == cnt[:, 4].sum() and got_ok["completed"] == cnt[:, 6].sum()
    assert np.array_equal(sim.instance_hashes(), hashes)


def replay_same(sim):
    """poison_outputs(); rerun(); synchronize() reproduces the flush."""
    want = (sim.status().copy(), sim.time().copy(), sim.checksums().copy(), sim.counters(only_ok=False))
    sim.poison_outputs()
    sim.rerun()
    sim.synchronize()
    assert np.array_equal(sim.status(), want[0])
    assert np.array_equal(sim.time(), want[1])
    assert np.array_equal(sim.checksums(), want[2])
    assert sim.counters(only_ok=False) == want[3]


def same_outputs(a, b):
    assert np.array_equal(a.status(), b.status())
    assert np.array_equal(a.time(), b.time())
    assert np.array_equal(a.checksums(), b.checksums())
    assert a.counters(only_ok=False) == b.counters(only_ok=False)


# ---- 255 packets on one channel, and the 256th -----------------------------------------------------

# (topology, the sender, its deep out-link's dest, a second out-link's dest, payload of send k)
DEEP = {
    "even_half": (TOP3, "A", "B", "C", lambda k: 1 + k % 5),
    "odd_half": (TOP3, "A", "C", "B", lambda k: 1 + k % 5),
    "hub5_lds_heads": (HUB5_TOP, "H", "L2", "L4", lambda k: 1 + k % 5),
    "hub10_lds_heads": (HUB10_TOP, "H", "L3", "L7", lambda k: 1 if k % 8 == 0 else 0),   # (H has 40 tokens)
}


def program_255(where):
    """255 sends on the deep channel at time 0 and three on a neighbour; from time 5 on every
    packet is due and the sender delivers one per tick, so after 12 ticks the deep channel has
    room for the two markers of the snapshots (at the sender, then at the neighbour's dest: that
    one records what the neighbour still carries behind the deep channel's traffic)."""
    _, src, deep, oth, pay = DEEP[where]
    return ("".join(f"send {src} {deep} {pay(k)}\n" for k in range(255))
            + f"send {src} {oth} 1\n" * 3 + f"tick 12\nsnapshot {src}\ntick 2\nsnapshot {oth}\n")


@pytest.mark.parametrize("where", list(DEEP))
def test_depth_exactly_255(where):
    """Regime (oracle): no instance overflows, the deep channel's peak depth is exactly 255 and the
    neighbour's at most 5.  Every instance is OK and equals the oracle -- the neighbour's packets,
    markers and recorded interval included -- and so do the batch counters; a replay
    reproduces the flush."""
    top, src, deep, oth, _ = DEEP[where]
    n, ev = 64, program_255(where)
    ws = walks(top, ev, n)
    for w in ws:
        assert w.overflow is None
        assert w.peak_of(src, deep) == 255 and w.peak_of(src, oth) <= 5
        assert w.ref.num_snapshots == 2 and w.ref.complete(0) and w.ref.complete(1)
    sim = one_shot(top, ev, n)
    assert check(sim, top, ws) == 0
    check_counters(sim, top, ev, n)
    replay_same(sim)


def program_256(where, variant):
    """Time 7, then a 256th push on the deep channel with no tick in between: a single send, a
    send inside a group of sends from distinct senders (OP_SENDS), or the marker of the sender's
    own StartSnapshot (its other out-link's marker is still due).  The program goes on after it."""
    _, src, deep, oth, pay = DEEP[where]
    send = [f"send {src} {deep} {pay(k)}\n" for k in range(256)]
    if variant == "single":
        body = "".join(send)
    elif variant == "grouped":
        body = "".join(send[k] + f"send {'BC'[k % 2]} A 0\n" for k in range(256))
    else:
        body = "".join(send[:255]) + f"snapshot {src}\n"
    return "tick 7\n" + body + f"tick 3\nsend {src} {oth} 1\ntick 2\n"


@pytest.mark.parametrize("where,variant", [(w, v) for w in ("even_half", "odd_half")
                                           for v in ("single", "grouped", "marker")]
                         + [("hub5_lds_heads", "single"), ("hub5_lds_heads", "marker"),
                            ("hub10_lds_heads", "single"), ("hub10_lds_heads", "marker")])
def test_push_256_freezes_the_instance(where, variant):
    """Regime (oracle): every instance meets 255 queued packets at the same event -- event 256 (511
    in the grouped program) -- at oracle time 7.  Every instance reports INST_FIFO_OVERFLOW with
    time() == 7 and is counted under `other`; a replay reproduces it."""
    top = DEEP[where][0]
    n, ev = 64, program_256(where, variant)
    ws = walks(top, ev, n)
    at = 1 + (2 * 255 if variant == "grouped" else 255)
    for w in ws:
        assert w.overflow == (at, 7)
    sim = one_shot(top, ev, n)
    assert check(sim, top, ws) == n
    replay_same(sim)


@pytest.mark.parametrize("deep", ["B", "C"], ids=["even_half", "odd_half"])
def test_data_dependent_overflow_inside_shared_waves(deep):
    """250 sends, 4 ticks, 8 more sends: whether the 256th push meets a full channel depends on
    how many packets the instance's delays let through in 4 ticks.  Regime (oracle): both classes
    hold at least 32 of the 256 instances (204 overflow at time 4, events 256-258; 52 do not and
    peak at 254-255).  21 instances share a wave: a frozen segment must not disturb its wave-mates,
    which equal the oracle in full."""
    n = 256
    ev = f"send A {deep} 1\n" * 250 + "tick 4\n" + f"send A {deep} 2\n" * 8 + "tick 300\n"
    ws = walks(TOP3, ev, n)
    over = [w for w in ws if w.overflow is not None]
    assert len(over) >= 32 and n - len(over) >= 32
    assert all(w.overflow[1] == 4 for w in over)
    assert all(254 <= w.peak_of("A", deep) <= 255 for w in ws if w.overflow is None)
    sim = one_shot(TOP3, ev, n)
    assert check(sim, TOP3, ws) == len(over)
    replay_same(sim)


TOPB = "3\nA 100\nB 30000\nC 0\nA B\nA C\nB A\nC A\n"


def in_tick_case(top, src, dest, k, n):
    """k sends on src -> dest, every one with delay 4 (receiveTime 5), then a snapshot at `dest`
    whose marker to `src` has delay 0: at tick 1 nothing on src -> dest is due, src takes its first
    marker and broadcasts onto src -> dest.  (events, schedule)"""
    ev = f"send {src} {dest} 1\n" * k + f"snapshot {dest}\ntick 1\ntick 5\nsend {dest} {src} 0\ntick 3\n"
    rng = np.random.default_rng(k)
    sched = rng.integers(0, 5, size=(n, 272), dtype=np.uint8)
    sched[:, :k] = 4
    # the snapshot's broadcast draws in dest order: the marker to `src` is draw k + (links of
    # `dest` to nodes before `src`) -- here `dest` reaches only A, or `src` = B is A's first link
    sched[:, k] = 0
    return ev, sched


@pytest.mark.parametrize("top,src,dest", [(TOPB, "B", "A"), (TOP3, "A", "B"), (TOP3, "A", "C")],
                         ids=["B_to_A", "A_even_half", "A_odd_half"])
def test_in_tick_overflow_at_255(top, src, dest):
    """Regime (oracle, in_tick walk): tick 1 (event 256) leaves 256 packets on the channel at oracle
    time 1; nothing on it was due (every receiveTime is 5), so the broadcast's push met exactly 255.
    Every instance freezes with INST_FIFO_OVERFLOW at time 1 (the marker broadcast of the staged
    unrolled kernel, push_pred; with A as the sender its other link's marker is still pushed)."""
    n = 64
    ev, sched = in_tick_case(top, src, dest, 255, n)
    ws = walks(top, ev, n, schedule=sched, in_tick=True)
    for w in ws:
        assert w.overflow == (256, 1) and w.peak_of(src, dest) == 256
    sim = one_shot(top, ev, n, schedule=sched)
    assert check(sim, top, ws) == n
    replay_same(sim)


@pytest.mark.parametrize("top,src,dest", [(TOPB, "B", "A"), (TOP3, "A", "B"), (TOP3, "A", "C")],
                         ids=["B_to_A", "A_even_half", "A_odd_half"])
def test_in_tick_marker_is_the_255th_packet(top, src, dest):
    """The twin with 254 sends.  Regime (oracle): no overflow, peak depth exactly 255, reached by the
    broadcast at tick 1.  Every instance equals the oracle to the end."""
    n = 64
    ev, sched = in_tick_case(top, src, dest, 254, n)
    ws = walks(top, ev, n, schedule=sched)
    for w in ws:
        assert w.overflow is None and w.peak_of(src, dest) == 255
        assert w.depth_before(256, src, dest) == 255      # (event 256: the "tick 5" after tick 1)
    sim = one_shot(top, ev, n, schedule=sched)
    assert check(sim, top, ws) == 0
    check_counters(sim, top, ev, n, schedule=sched)
    replay_same(sim)


# ---- the HBM spill ring -------------------------------------------------------------------------------

def wrap_lines(deep):
    """Phase 1: 240 sends on A -> `deep`, then 46 rounds of 10 ticks and 10 sends, a snapshot and 600
    ticks: 701 pushes through the 256 slots of the spill ring, which ends empty with its head left
    wherever the last refill put it.  Phase 2: 110 sends (the ring restarts), 108 ticks -- from 5
    ticks after the sends every packet is due and A delivers one per tick, so 2-6 packets remain, all
    in the 8-slot LDS ring -- then 120 sends that spill again from a ring that is not empty, a
    snapshot, and a tail.  "|": flush points with more than 100 packets queued."""
    out = [f"send A {deep} {1 + k % 7}" for k in range(240)]
    for r in range(46):
        out.append("tick 10")
        out += [f"send A {deep} {1 + (r + k) % 7}" for k in range(10)]
        if r in (4, 29):
            out.append("|")
    out += ["snapshot A", "tick 600"]
    out += [f"send A {deep} {1 + k % 7}" for k in range(110)] + ["|", "tick 108"]
    out += [f"send A {deep} {2 + k % 5}" for k in range(120)] + ["|", f"snapshot {deep}", "tick 3"]
    out += [f"send A {deep} {1 + k % 3}" for k in range(10)] + ["tick 300"]
    return out


@pytest.mark.parametrize("deep", ["B", "C"], ids=["even_half", "odd_half"])
def test_spill_ring_wrap_and_restart(deep):
    """Regime (oracle, 64 instances): no overflow; peak depth of the channel 241-250 (observed
    241-245); 942 pushes on it; more than 100 packets queued at each of the 4 flush points (240-244,
    240-244, 110, 122-126); 1-8 packets (observed 2-6: the LDS ring, not empty) queued when the
    third burst starts.  The 948 draws per row are too long to stage in LDS, so this runs the
    unstaged generic kernel.  One launch, and flushes that save and resume the state image while the
    ring holds packets, equal each other and the oracle."""
    n, lines = 64, wrap_lines(deep)
    ev = text_of(lines)
    events = D.parse_events(ev)
    sched = cl.go_delay_schedule(SEED, n, 948)
    assert sum(e[0] == "send" for e in events) + 2 * 4 <= sched.shape[1]
    ws = walks(TOP3, ev, n, schedule=sched)
    flushes, k = [], 0
    for ln in lines:
        if ln == "|":
            flushes.append(k)
        else:
            k += 1
    third = flushes[2] + 1     # the first send after "tick 108"
    assert events[third - 1] == ("tick", 108) and events[third][0] == "send"
    for w in ws:
        assert w.overflow is None and 241 <= w.peak_of("A", deep) <= 250
        assert all(w.depth_before(f, "A", deep) > 100 for f in flushes)
        assert 1 <= w.depth_before(third, "A", deep) <= 8
    one = one_shot(TOP3, ev, n, schedule=sched)
    assert check(one, TOP3, ws) == 0
    check_counters(one, TOP3, ev, n, schedule=sched)
    inc = feed(make_sim(TOP3, n, sched), lines, drain=True)
    same_outputs(one, inc)
    assert check(inc, TOP3, ws) == 0
    replay_same(one)


@pytest.mark.parametrize("deep", ["B", "C"], ids=["even_half", "odd_half"])
@pytest.mark.parametrize("slots,total,long_rows", [(2, 130, False), (2, 130, True), (64, 128, False), (64, 192, False)],
                         ids=["2_slots_plus_128", "2_slots_plus_128_unstaged", "64_slots_plus_64", "64_slots_plus_128"])
def test_spill_ring_filled_with_no_slack(slots, total, long_rows, deep):
    """total - 1 sends and the sender's own marker are all the packets the channel ever carries, so
    the host sizes the spill ring to exactly total - slots slots (a power of two) and every one is
    used.  Regime (oracle): peak depth == total, no overflow.  The dest's tokenMap entry counts every
    send (its marker is the last packet of the channel).  64 LDS slots and the 416-draw rows (not
    staged in LDS) run the generic kernel, 2 slots with short rows the specialized one."""
    n = 64
    oth = "C" if deep == "B" else "B"
    ev = "".join(f"send A {deep} {1 + k % 9}\n" for k in range(total - 1)) + f"snapshot A\ntick 3\nsend A {oth} 5\n"
    sched = cl.go_delay_schedule(SEED, n, 416) if long_rows else None
    ws = walks(TOP3, ev, n, schedule=sched)
    for w in ws:
        assert w.overflow is None and w.peak_of("A", deep) == total
        assert w.ref.collect(0).tokens[deep] == sum(1 + k % 9 for k in range(total - 1))
    sim = one_shot(TOP3, ev, n, schedule=sched, fifo_lds_slots=slots)
    assert check(sim, TOP3, ws) == 0
    check_counters(sim, TOP3, ev, n, schedule=sched)
    replay_same(sim)


# ---- payload, time and cursor widths --------------------------------------------------------------------

def pay_top(a_tokens):
    return f"3\nA {a_tokens}\nB 0\nC 0\nA B\nA C\nB A\nC A\n"


PAY_LINES = ["send A B 65535", "send A B 65534", "tick 8", "snapshot B",
             "send A B 32768", "send A B 32767", "send A B 0", "send A B 65535", "send A C 65535",
             "tick 2", "snapshot A", "send A B 65534", "send B A 65535", "tick 1", "snapshot C"]


def check_analytics(sim, ws, n):
    """collect_snapshot_packed, snapshot_stats and select_instances against the oracle rows."""
    refs = [w.ref for w in ws]
    rows, keys = selectcheck.from_refs(refs)
    layout = sim.stats_layout()
    chans = D.channels_of(TOP3)
    ab = chans.index(("A", "B"))
    for sid in range(3):
        tok, done, off, msg = sim.collect_snapshot_packed(sid)
        assert done.all()
        for i, r in enumerate(refs):
            t, o, vals = r.collect_channels(sid)
            assert np.array_equal(tok[i], t)
            c = len(chans)
            assert np.array_equal(off[i * c:(i + 1) * c + 1] - off[i * c], o)
            assert np.array_equal(msg[off[i * c]:off[(i + 1) * c]], vals)
        got = sim.snapshot_stats(sid)
        statscheck.assert_stats_equal(got.raw, statscheck.expected(layout, rows, sid, 0, n), layout, f"snapshot {sid}")
        for clauses, want in (([("ch_tok", ("A", "B"), 65536, None)], [("ch_tok", ab, 65536, None)]),
                              ([("inflight", None, 65536, 200000)], [("inflight", None, 65536, 200000)]),
                              ([("node", "B", 65536, None), ("ch_tok", ("A", "B"), None, 65535)],
                               [("node", 1, 65536, None), ("ch_tok", ab, None, 65535)])):
            sel = sim.select_instances(sid, clauses, ticks=True)
            selectcheck.assert_selection_equal(sel, selectcheck.expected(rows, keys, sid, 0, n, want),
                                               f"snapshot {sid}")
    return rows


@pytest.mark.parametrize("queued", [False, True], ids=["drained", "250_packets_queued"])
def test_payload_width(queued):
    """Sends of 65535, 65534, 32768, 32767 and 0 tokens.  Regime (oracle): B records 131069 tokens
    (> 65535) in snapshot 0, which records at least 65535 + 32768 tokens on A -> B in some instance
    and more than 65535 in every one.  Drained (A 1000000), and ending with 250 packets of 65535
    queued on A -> B across the LDS ring and the spill ring -- 16,383,750 tokens in flight, so A
    starts with 17,000,000 there.  Node tokens, CollectSnapshot, the packed collect, the statistics
    and the selections equal the oracle; both residuals are 0."""
    n = 64
    top = pay_top(17_000_000 if queued else 1_000_000)
    lines = PAY_LINES + (["tick 60"] + ["send A B 65535"] * 250 if queued else [])
    ev = text_of(lines)
    ws = walks(top, ev, n, drain=not queued)
    ab = D.channels_of(top).index(("A", "B"))
    for w in ws:
        assert w.overflow is None
        assert all(w.ref.complete(s) for s in range(3))
        assert w.ref.collect(0).tokens["B"] == 65535 + 65534
        if queued:
            assert w.ref.queue_depths()[ab] == 250 and w.ref.node_tokens()["A"] < 17_000_000 - 250 * 65535
    sim = feed(make_sim(top, n), lines, drain=not queued)
    assert check(sim, top, ws) == 0
    if queued:
        assert sums_of(sim)["in_flight"] == n * 250 * 65535
    rows = check_analytics(sim, ws, n)
    assert rows.ch_tok[0][:, ab].min() > 65535 and rows.ch_tok[0][:, ab].max() >= 65535 + 32768
    replay_same(sim)
    if not queued:
        same_outputs(sim, one_shot(top, ev, n))


def time_lines():
    """Traffic and two snapshots after time 32700, ending at exactly 32759 with one send."""
    return ["tick 32700", "send A B 100", "send A C 50", "send A B 127", "|", "snapshot B", "tick 20",
            "send B A 60", "snapshot A", "|", "tick 30", "|", "tick 9", "send A B 5"]


@pytest.mark.parametrize("engine", [NODES, LANES], ids=["nodes", "lanes"])
def test_time_width(engine):
    """Regime (oracle, 64 instances): the run ends at time 32759 = kMaxTime; both snapshots complete
    after 32700; the last send's draw is 4, so its receiveTime is 32764 -- the largest a FIFO entry
    ever holds -- and its 5 tokens are still in flight at the end.  One launch, and flushes across the
    late part, equal each other and the oracle (payloads below 128: the lanes kernel runs it too)."""
    n, lines = 64, time_lines()
    ev = text_of(lines)
    sched = cl.go_delay_schedule(SEED, n, 16).copy()
    last = 4 + 2 * 4            # the draw of the last send: 4 sends and two snapshots' broadcasts before it
    assert sum(ln.startswith("send") for ln in lines) == 5
    sched[:, last] = 4
    ws = walks(TOP3, ev, n, schedule=sched, drain=False)
    ab = D.channels_of(TOP3).index(("A", "B"))
    for w in ws:
        assert w.overflow is None and w.ref.time == 32759
        assert all(w.ref.complete(s) and w.ref.completion_tick(s) > 32700 for s in range(2))
        assert w.ref.queue_depths().tolist() == [1 if c == ab else 0 for c in range(4)]
        assert 30000 - sum(w.ref.node_tokens().values()) == 5
    one = feed(make_sim(TOP3, n, sched, engine), [ln for ln in lines if ln != "|"], drain=False, engine=engine)
    assert check(one, TOP3, ws) == 0
    assert (one.time() == 32759).all()
    inc = feed(make_sim(TOP3, n, sched, engine), lines, drain=False, engine=engine)
    same_outputs(one, inc)
    assert check(inc, TOP3, ws) == 0
    replay_same(one)


CUR_TOP = "3\nA 30000\nB 100\nC 0\nA B\nA C\nB A\nC A\n"


def cursor_lines():
    """Rounds of four sends on A -> B, one on B -> A and 6 ticks (A delivers one packet per tick, so
    the queues stay shallow); a snapshot at B after 80 rounds, at A and again at B after 1030."""
    rnd = ["send A B 1", "send A B 2", "send A B 1", "send A B 3", "send B A 1", "tick 6"]
    return (rnd * 80 + ["snapshot B", "send A B 2", "send A C 1"] + rnd * 950
            + ["snapshot A", "send B A 2", "snapshot B", "send A B 4", "send A B 1", "tick 2"])


def test_cursor_width():
    """Regime (oracle, 24 instances: a full wave of 21 and a ragged one): at least 300 token packets
    were delivered on A -> B when snapshot 0 starts recording it and at least 4096 when snapshot 2
    does; at least 1024 on B -> A when snapshot 1 starts (A's two in-link cursors share a register);
    no channel ever holds more than 16 packets.  The recorded intervals (CollectSnapshot) and the ch_msgs / ch_tok statistics
    equal the oracle."""
    n, lines = 24, cursor_lines()
    ev = text_of(lines)
    events = D.parse_events(ev)
    sched = cl.go_delay_schedule(SEED, n, 5200)
    snaps = [k for k, e in enumerate(events) if e[0] == "snapshot"]
    sent = lambda k, s, d: sum(e[:3] == ("send", s, d) for e in events[:k])   # noqa: E731
    assert sum(e[0] == "send" for e in events) + 3 * 4 <= sched.shape[1]
    ws = walks(CUR_TOP, ev, n, schedule=sched)
    for w in ws:
        assert w.overflow is None and w.peak.max() <= 16
        assert sent(snaps[0], "A", "B") - w.depth_before(snaps[0], "A", "B") >= 300
        assert sent(snaps[1], "B", "A") - w.depth_before(snaps[1], "B", "A") >= 1024
        assert sent(snaps[2], "A", "B") - w.depth_before(snaps[2], "A", "B") >= 4096
        assert all(w.ref.complete(s) for s in range(3))
    sim = one_shot(CUR_TOP, ev, n, schedule=sched)
    assert check(sim, CUR_TOP, ws) == 0
    rows = statscheck.Rows([w.ref for w in ws])
    layout = sim.stats_layout(tick_lo=6000, tick_bins=256)
    for sid in range(3):
        got = sim.snapshot_stats(sid, tick_lo=6000, tick_bins=256)
        statscheck.assert_stats_equal(got.raw, statscheck.expected(layout, rows, sid, 0, n), layout, f"snapshot {sid}")
    assert sum(int(rows.ch_msgs[s].sum()) for s in range(3)) > 0     # (something was recorded)
    replay_same(sim)
