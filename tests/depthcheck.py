"""Step the CPU oracle event by event and watch its channel depths (no GPU).

The reference's queue (queue.go:6-28) is unbounded; the node-parallel engine keeps a channel's
queued count in 8 bits (cl_engine.h kMaxQueued = 255) and freezes an instance with
INST_FIFO_OVERFLOW at the push that meets a channel already holding 255 packets.  The oracle has
no such status, so this walk defines the expected one: it replays a program on an OracleSim
through send_tokens / start_snapshot / tick and reads queue_depths()

* before every host push -- a send, and every out-link of a StartSnapshot's broadcast (the
  broadcast pushes one marker on each out-link of the node, so each push meets the depth read
  before the broadcast) -- and stops at the first one that meets 255 packets;
* after every tick, where no depth may exceed 255.  A push inside a tick (a marker broadcast,
  node.go:97-109) that meets a full channel is ambiguous by one packet: the reference pops and
  pushes node by node, the engine pops every channel first (cl_kernels.hip tick(), phases A
  and D).  Only a program built so that the full channel cannot pop in that tick may ask for
  it (in_tick=True): the walk then stops at the tick that left more than 255 packets queued.

The graph engine's channels hold fifo_slots packets (cg_kernels.hip push_entry / push_q): its tests
walk with limit=fifo_slots, and may draw their delays from the counter hash (counter_hash=seed).

The walk ends like readEventsFile (test_common.go:123-137): ticks until every started snapshot
has completed, then maxDelay + 1 more.
"""
import numpy as np

import oracle as O

LIMIT = 255          # cl_engine.h kMaxQueued
EXTRA_TICKS = 6      # maxDelay + 1 (test_common.go:135-137)


def parse_events(text):
    """[("send", src, dest, n) | ("snapshot", node) | ("tick", n)] of an events text."""
    out = []
    for ln in text.split("\n"):
        f = ln.split()
        if not f or ln == "#":
            continue
        if f[0] == "send":
            out.append(("send", f[1], f[2], int(f[3])))
        elif f[0] == "snapshot":
            out.append(("snapshot", f[1]))
        elif f[0] == "tick":
            out.append(("tick", int(f[1]) if len(f) > 1 else 1))
        else:
            raise ValueError(f"unknown event: {ln!r}")
    return out


def channels_of(top):
    """(src, dest) of every channel in the engine's and the oracle's channel order: senders by
    id, each sender's links by dest id (cl_oracle.c orc_queue_depths)."""
    f = top.split()
    n = int(f[0])
    links = f[1 + 2 * n:]
    return sorted(zip(links[0::2], links[1::2]))


class Walk:
    """overflow: (event index, oracle time) of the first push that met 255 packets, or None;
    peak: most packets queued at once per channel (numpy, channel order), a host push counted
    when it is made; before[k]: the depths event k met; channels: [(src, dest)]; ref: the
    OracleSim where the walk stopped."""

    def __init__(self, overflow, peak, before, channels, ref):
        self.overflow, self.peak, self.before, self.channels, self.ref = overflow, peak, before, channels, ref

    def peak_of(self, src, dest):
        return int(self.peak[self.channels.index((src, dest))])

    def depth_before(self, event, src, dest):
        return int(self.before[event][self.channels.index((src, dest))])


def walk(top, events, seed=None, schedule=None, drain=True, max_drain=10000, in_tick=False, limit=LIMIT,
         counter_hash=None):
    """limit: the packets a channel holds (the graph engine's fifo_slots; default the node-parallel
    kernel's 255).  Delays: an explicit schedule, the counter hash of seed `counter_hash`
    (OracleSim.use_counter_hash), else the Go stream of `seed`."""
    ref = O.OracleSim()
    if schedule is not None:
        ref.use_schedule(schedule)
    elif counter_hash is not None:
        ref.use_counter_hash(counter_hash)
    else:
        ref.seed_go(seed)
    assert ref.read_topology_text(top) == 0
    chans = channels_of(top)
    assert len(chans) == ref.num_links
    index = {c: k for k, c in enumerate(chans)}
    out_links = {}
    for k, (s, _) in enumerate(chans):
        out_links.setdefault(s, []).append(k)
    peak = np.zeros(len(chans), dtype=np.int64)
    before = []

    def depths():
        d = ref.queue_depths()
        np.maximum(peak, d, out=peak)
        return d

    def tick(ei):
        """One tick; True when it left more than `limit` packets on a channel (in_tick only)."""
        assert ref.tick() == 0
        d = depths()
        if in_tick and d.max() > limit:
            return True, d
        assert d.max() <= limit, f"event {ei}: a tick left {d.max()} packets on a channel at time {ref.time}"
        return False, d

    for ei, ev in enumerate(parse_events(events) if isinstance(events, str) else events):
        d = depths()
        before.append(d)
        if ev[0] == "send":
            c = index.get((ev[1], ev[2]))
            if c is not None and d[c] >= limit:
                return Walk((ei, ref.time), peak, before, chans, ref)
            assert ref.send_tokens(ev[1], ev[2], ev[3]) == 0, f"event {ei}: send refused"
            if c is not None:
                peak[c] = max(peak[c], d[c] + 1)
        elif ev[0] == "snapshot":
            mine = out_links.get(ev[1], [])
            if any(d[c] >= limit for c in mine):
                return Walk((ei, ref.time), peak, before, chans, ref)
            assert ref.start_snapshot(ev[1])[0] == 0
            for c in mine:
                peak[c] = max(peak[c], d[c] + 1)
        else:
            for k in range(ev[1]):
                over, d = tick(ei)
                if over:
                    return Walk((ei, ref.time), peak, before, chans, ref)
                if not d.any():   # nothing queued: the remaining ticks of this event only pass time
                    for _ in range(ev[1] - k - 1):
                        assert ref.tick() == 0
                    break
    depths()
    if drain:
        waited = 0
        while not all(ref.complete(s) for s in range(ref.num_snapshots)):
            assert waited < max_drain, "the drain would hang"
            over, _ = tick(-1)
            assert not over, "overflow inside the drain"
            waited += 1
        for _ in range(EXTRA_TICKS):
            over, _ = tick(-1)
            assert not over, "overflow inside the drain"
    return Walk(None, peak, before, chans, ref)
