"""Programs that drive the graph engine's tick kernels (cg_kernels.hip) to the limits of their packed
words, and oracle-only probes of the regimes they aim at (no GPU).

Every builder returns a Case: (top text, events text, delay spec, fifo_slots, max_snapshots) and, as
a sixth field, what the case aims at.  The events text may hold FLUSH lines: each part between them
is one readEventsFile call (with its drain), and the engine is flushed after each.  The delay spec is
("schedule", uint8 array) or ("hash", seed).  tests/test_graph_edges_host.py runs the cases on the
oracle alone and asserts the regimes; tests/test_graph_edges_gpu.py runs them on the engine.

What is aimed at (cg_engine.h, cg_kernels.hip):

* creations per node and tick: k_marker numbers the local snapshots a node creates in one tick
  (crn / cre), k_push broadcasts them in creating-sender order -- push_node_lanes sorts up to kRegCre
  = 4 in registers, else walks them (next_creation); push_node_reg pushes in chunks of kRegOd = 8
  out-links; nodes of in-degree above kSmallIndeg = 64 are expanded by the whole k_push grid (BigX);
  expand_range records the tokens later senders (src > s0) delivered in the creation tick;
* the delivery word pp[s].x = (t << 6) | j with out-links 63 and 64 (j = 62, 63);
* the head word hq: ring head (16 bits) | packets queued (16 bits) at fifo_slots = 32768;
* the payload history (hist_needed: a power of two, at least 16) and the payload word 2^31 - 1;
* node blocks of kGThreads = 256 at n = 1, 255, 256, 257, 513.
"""
import collections
import functools

import numpy as np

import depthcheck as D
import graphgen as G
import oracle as O
from graphcheck import Program, _snaps, oracle_program

FLUSH = "#flush"
MAX_DRAIN = 100_000
LOG_RECV_TOKEN, LOG_RECV_MARKER, LOG_START = 2, 3, 4   # include/clsnap.h CL_LOG_*
PAYLOAD_MAX = (1 << 31) - 1                            # cg_engine.h kGPayload

Case = collections.namedtuple("Case", "top events delay fifo_slots max_snapshots aim", defaults=({},))


# ---- running a case on the oracle -----------------------------------------------------------------

def parts(events):
    """The events texts between FLUSH lines."""
    out, cur = [], []
    for ln in events.split("\n"):
        if ln == FLUSH:
            out.append("\n".join(cur) + "\n")
            cur = []
        elif ln:
            cur.append(ln)
    if cur:
        out.append("\n".join(cur) + "\n")
    return out


def whole(events):
    """The events without their FLUSH lines (one text: depthcheck.walk)."""
    return "".join(parts(events))


def oracle_delay(o, delay):
    if delay[0] == "schedule":
        o.use_schedule(delay[1])
    else:
        o.use_counter_hash(delay[1])


def run_oracle(case, log=False):
    """The case on the oracle: one readEventsFile per part (with its drain); a case with synthetic
    traffic (aim["traffic"]) event by event, without a drain."""
    o = O.OracleSim()
    oracle_delay(o, case.delay)
    if log:
        o.log_enable()
    assert o.read_topology_text(case.top) == 0
    if "traffic" in case.aim:
        return _run_traffic(o, case)
    for ev in parts(case.events):
        o.read_events_text(ev, case.aim.get("max_drain", MAX_DRAIN))
    return o


def _run_traffic(o, case):
    """The engine's order: the traffic of step 0 at the start, the traffic of step t
    after tick t, host events in between."""
    seed, thresh, steps = case.aim["traffic"]
    sends = lambda step: o._L.orc_traffic_sends(o._h, seed, thresh, step)  # noqa: E731
    if steps > 0:
        assert sends(0) == 0
    for ev in D.parse_events(case.events):
        if ev[0] == "send":
            assert o.send_tokens(ev[1], ev[2], ev[3]) == 0
        elif ev[0] == "snapshot":
            assert o.start_snapshot(ev[1])[0] == 0
        else:
            for _ in range(ev[1]):
                assert o.tick() == 0
                if o.time < steps:
                    assert sends(o.time) == 0
    return o


def walk(case, **kw):
    """depthcheck.walk of a case with the channel limit fifo_slots."""
    d = {"schedule": case.delay[1]} if case.delay[0] == "schedule" else {"counter_hash": case.delay[1]}
    return D.walk(case.top, whole(case.events), limit=case.fifo_slots, max_drain=MAX_DRAIN, **d, **kw)


@functools.lru_cache(maxsize=None)
def case(builder, *args):
    """builder(*args), built once (builder: a name in this module)."""
    return globals()[builder](*args)


@functools.lru_cache(maxsize=None)
def oracle_of(builder, *args, log=False):
    """The oracle's run of case(builder, *args), computed once and shared; never changed."""
    return run_oracle(case(builder, *args), log=log)


@functools.lru_cache(maxsize=None)
def walk_of(builder, *args, **kw):
    return walk(case(builder, *args), **kw)


# ---- regime probes (oracle log) -------------------------------------------------------------------

def creations(o):
    """{(epoch, node rank): local snapshots created there by a received marker} from the oracle's
    Logger: a received marker for an id the node has not yet seen (nor started) is a creation."""
    seen, out = set(), collections.Counter()
    for ep, kind, node, _, data, _ in o.log():
        if kind == LOG_START:
            seen.add((node, data))
        elif kind == LOG_RECV_MARKER and (node, data) not in seen:
            seen.add((node, data))
            out[(ep, node)] += 1
    return out


def same_tick_tokens(o):
    """[(sid, src rank, node rank, payload, later)]: a token the node received in the tick that
    created its local snapshot sid, from a sender other than the creating one; later = delivered
    after the creating marker (sim.go:76-90 delivers in sender rank order), so the snapshot records
    it (node.go:174-185)."""
    seen, by_tick = set(), collections.defaultdict(lambda: ([], []))
    for ep, kind, node, other, data, _ in o.log():
        if kind == LOG_START:
            seen.add((node, data))
        elif kind == LOG_RECV_MARKER and (node, data) not in seen:
            seen.add((node, data))
            by_tick[(ep, node)][0].append((data, other))
        elif kind == LOG_RECV_TOKEN:
            by_tick[(ep, node)][1].append((other, data))
    out = []
    for (_, node), (cre, tok) in by_tick.items():
        for sid, s0 in cre:
            for src, pay in tok:
                out.append((sid, src, node, pay, src > s0))
    return out


@functools.lru_cache(maxsize=None)
def channels(top):
    """[(src id, dest id)] in channel order."""
    return D.channels_of(top)


def recorded_on(o, top, sid, src, dest):
    """The payloads snapshot sid recorded on channel src -> dest (ids), in delivery order."""
    c = channels(top).index((src, dest))
    _, off, vals = o.collect_channels(sid)
    return vals[off[c]:off[c + 1]].tolist()


# ---- schedules ------------------------------------------------------------------------------------

def out_links(top):
    """{node id: [dest ids in dest order]}"""
    out = {}
    for s, d in D.channels_of(top):
        out.setdefault(s, []).append(d)
    return out


def host_draws(top, events):
    """Delay draws of the host events before the first tick: one per send, one per out-link of a
    StartSnapshot (sim.go:100-102)."""
    links = out_links(top)
    n = 0
    for ev in D.parse_events(whole(events)):
        if ev[0] == "tick":
            break
        n += 1 if ev[0] == "send" else len(links.get(ev[1], []))
    return n


def schedule(top, events, total, mixed):
    """Delay 0 for every host draw before the first tick (so every first packet is deliverable in
    tick 1 and each sender's first link in dest order is the one that delivers), then zeros, or
    (mixed) delays 0-4 from a fixed stream, which make the order of the draws inside a tick
    visible in every later receive time."""
    s = np.zeros(total, dtype=np.uint8)
    if mixed:
        h = host_draws(top, events)
        s[h:] = np.random.default_rng(20240).integers(0, 5, total - h, dtype=np.uint8)
    return s


def topology(nodes, links):
    """nodes: [(id, tokens)], links: [(src id, dest id)]"""
    return f"{len(nodes)}\n" + "".join(f"{i} {t}\n" for i, t in nodes) + "".join(f"{a} {b}\n" for a, b in links)


def text(lines):
    return "".join(ln + "\n" for ln in lines)


TOKEN_PAYLOADS = (7, 11, 13)   # non-unit: the engine keeps the payload history


# ---- 1. creations per node and tick ---------------------------------------------------------------

def complete_case(n=65, tokens=False, mixed=False):
    """(a) The complete digraph on n nodes (n = 65: out- and in-degree 64, out-links 63 and 64 in
    use).  Every node starts a snapshot, then tick 1: every sender's first link in dest order points
    at the lowest-ranked node, which creates n - 1 local snapshots in that tick.  tokens: nodes 1, n
    // 2 and n - 1 first send it a token, which they deliver in tick 1 instead of their marker --
    from below, between and above the creating senders."""
    ids = [f"n{r:03d}" for r in range(n)]
    top = topology([(i, 100) for i in ids], [(a, b) for a in ids for b in ids if a != b])
    senders = [1, n // 2, n - 1] if tokens else []
    ev = [f"send {ids[r]} {ids[0]} {p}" for r, p in zip(senders, TOKEN_PAYLOADS)]
    ev += [f"snapshot {i}" for i in ids] + ["tick 1"]
    events = text(ev)
    total = len(senders) + n * n * (n - 1)
    return Case(top, events, ("schedule", schedule(top, events, total, mixed)), 128, n,
                {"node": 0, "tick": 1, "creations": n - 1 - len(senders), "token_senders": senders})


def hub_case(leaves=129, tokens=False, mixed=False):
    """(b), (c) A hub ranked first with `leaves` leaves, each with a link to the hub and to the next
    leaf; the hub links to the first min(64, leaves) of them.  Every leaf starts a snapshot, then
    tick 1: every leaf's first link in dest order is the hub, which creates one local snapshot per
    leaf in that tick -- in-degree 64 through the creating block's expansion, 65 and more through
    the grid-wide one (kSmallIndeg).  tokens: as in complete_case, from the first, the middle and
    the last leaf."""
    hub = "h000"
    lv = [f"l{r:03d}" for r in range(1, leaves + 1)]
    links = [(x, hub) for x in lv] + [(lv[k], lv[(k + 1) % leaves]) for k in range(leaves)] + \
        [(hub, x) for x in lv[:min(64, leaves)]]
    top = topology([(hub, 100)] + [(x, 100) for x in lv], links)
    senders = [1, (leaves + 1) // 2, leaves] if tokens else []       # ranks (the hub is rank 0)
    ev = [f"send {lv[r - 1]} {hub} {p}" for r, p in zip(senders, TOKEN_PAYLOADS)]
    ev += [f"snapshot {x}" for x in lv] + ["tick 1"]
    events = text(ev)
    total = len(senders) + leaves * len(links)
    return Case(top, events, ("schedule", schedule(top, events, total, mixed)), 256, leaves,
                {"node": 0, "tick": 1, "creations": leaves - len(senders), "token_senders": senders})


def star_case(k, d, tokens=False, mixed=False):
    """(d) Exactly k local snapshots created at the centre m0 in tick 1, each broadcast on d
    out-links.  The k creating senders rank on both sides of the centre (b1, b2 < m0 < s1, ...); a0,
    c0 and t0 rank below, between and above them and (tokens) send the centre a token that arrives in
    the same tick.  The centre links to z01..z{d}; z01 links back to every sender and the other z
    to z01, so every snapshot completes."""
    cre = ["b1", "b2", "s1", "s2", "s3"]
    cre = {1: cre[:1], 4: cre[:4], 5: cre}[k]
    extra = ["a0", "c0", "t0"]
    zs = [f"z{j:02d}" for j in range(1, d + 1)]
    nodes = sorted(cre + extra + ["m0"] + zs)
    links = [(x, "m0") for x in cre + extra] + [("m0", z) for z in zs] + [(zs[0], x) for x in cre + extra] + \
        [(z, zs[0]) for z in zs[1:]]
    top = topology([(x, 100) for x in nodes], links)
    ev = [f"send {x} m0 {p}" for x, p in zip(extra, TOKEN_PAYLOADS)] if tokens else []
    ev += [f"snapshot {x}" for x in cre] + ["tick 1"]
    events = text(ev)
    total = len(ev) + k * len(links)
    return Case(top, events, ("schedule", schedule(top, events, total, mixed)), 16, k,
                {"node": nodes.index("m0"), "tick": 1, "creations": k,
                 "token_senders": [nodes.index(x) for x in extra] if tokens else []})


def skew_case(tokens=False, mixed=False):
    """Four creations at the centre m0 in tick 1 whose creating senders reach it out of rank order.
    a1 and a2 (ranks 1, 2: the first wave of the pick block) hold 63 out-links each and deliver on
    the last one, so their scan of 62 undeliverable heads (delay 1) ends after g1 and g2 (ranks 66,
    67: the second wave, one out-link each) have delivered: k_pick lists the markers, and k_marker
    numbers the creations, as they arrive.  Nothing in the result may depend on that order: the
    broadcasts go out in creating-sender order (the kRegCre sorting network of push_node_lanes, the
    next_creation walk elsewhere).  The fillers f01..f62 link to z01, which links back to every
    sender; tokens as in star_case (f99, rank 65, between the two pairs of creating senders)."""
    fill = [f"f{j:02d}" for j in range(1, 63)]
    cre, extra, zs = ["a1", "a2", "g1", "g2"], ["a0", "f99", "t0"], [f"z{j:02d}" for j in range(1, 10)]
    nodes = sorted(cre + extra + fill + ["m0"] + zs)
    assert [nodes.index(x) for x in cre + extra] == [1, 2, 66, 67, 0, 65, 69] and nodes.index("m0") == 68
    links = [(x, "m0") for x in cre + extra] + [(a, f) for a in cre[:2] for f in fill] + [(f, zs[0]) for f in fill] + \
        [("m0", z) for z in zs] + [(zs[0], x) for x in cre + extra] + [(z, zs[0]) for z in zs[1:]]
    top = topology([(x, 100) for x in nodes], links)
    ev = [f"send {x} m0 {p}" for x, p in zip(extra, TOKEN_PAYLOADS)] if tokens else []
    ev += [f"snapshot {x}" for x in cre] + ["tick 1"]
    events = text(ev)
    s = schedule(top, events, len(ev) + 4 * len(links), mixed)
    first = len(ev) - 5                     # draws of the token sends
    for a in range(2):                      # a1, a2: delay 1 on every link but the last (to m0)
        s[first + 63 * a:first + 63 * a + 62] = 1
    return Case(top, events, ("schedule", s), 16, 4,
                {"node": nodes.index("m0"), "tick": 1, "creations": 4,
                 "token_senders": [nodes.index(x) for x in extra] if tokens else []})


def last_link_case(link, mixed=False):
    """The delivery word's out-index at 62 and 63 where k_push decodes it (pk & 63): m0 has 64
    out-links, all queues empty but number `link` (63 or 64), which holds a token due in tick 1.  In
    that tick a0 (ranked below m0) delivers a marker that creates a local snapshot at m0, so the
    reference's scan at m0's turn peeks the link - 1 queues its broadcast has just made non-empty
    before it delivers on that link (sim.go:82-84)."""
    zs = [f"z{j:02d}" for j in range(1, 65)]
    top = topology([("a0", 10), ("m0", 10)] + [(z, 10) for z in zs],
                   [("a0", "m0")] + [("m0", z) for z in zs] + [(z, "a0") for z in zs])
    events = text([f"send m0 {zs[link - 1]} 3", "snapshot a0", "tick 1"])
    return Case(top, events, ("schedule", schedule(top, events, 2 + 130, mixed)), 16, 1,
                {"node": 1, "tick": 1, "creations": 1, "token_senders": [], "link": link})


# ---- 2., 3. ring and count field, overflow --------------------------------------------------------

RING_TOP = "3\nA 200000\nB 50\nC 0\nA B\nB A\nB C\nC A\n"
RING_HASH = 77


def _amount(i):
    return 1 + i % 3


def fill_case(slots, over=False):
    """slots - 1 sends on A -> B, then A starts a snapshot: its marker is packet number `slots`.  A
    token from B is on its way to A, so the snapshot has something to record.  over: `slots` sends
    fill the channel and one more send meets it full; the events after it must not run."""
    ev = ["send B A 5"]
    if over:
        ev += [f"send A B {_amount(i)}" for i in range(slots)] + ["send A B 2", "tick 3", "snapshot A", "tick 2"]
    else:
        ev += [f"send A B {_amount(i)}" for i in range(slots - 1)] + ["snapshot A"]
    return Case(RING_TOP, text(ev), ("hash", RING_HASH), slots, 2,
                {"channel": ("A", "B"), "overflow_event": slots + 1 if over else None, "by": "send"})


def wrap_case(slots, over=False):
    """`slots` sends fill A -> B; ticks pop at least min(100, slots / 2) packets (head > 0); the
    channel is refilled to one below full and A's StartSnapshot marker fills it again, so head + count
    crosses the end of the ring with never more than `slots` queued.  over: refilled to full, and the
    StartSnapshot broadcast meets the full channel."""
    ev = [f"send A B {_amount(i)}" for i in range(slots)]
    o = O.OracleSim()
    o.use_counter_hash(RING_HASH)
    assert o.read_topology_text(RING_TOP) == 0
    for ln in ev:
        f = ln.split()
        assert o.send_tokens(f[1], f[2], int(f[3])) == 0
    c = D.channels_of(RING_TOP).index(("A", "B"))
    want, ticks = max(1, min(100, slots // 2)), 0
    while slots - o.queue_depths()[c] < want:
        assert o.tick() == 0
        ticks += 1
    popped = int(slots - o.queue_depths()[c])
    assert 0 < popped < slots
    refill = popped if over else popped - 1
    ev += [f"tick {ticks}"] + [f"send A B {_amount(i)}" for i in range(refill)] + ["snapshot A"]
    if over:
        ev += ["tick 2", "send A B 1", "tick 2"]
    return Case(RING_TOP, text(ev), ("hash", RING_HASH), slots, 2,
                {"channel": ("A", "B"), "pushed": slots + refill + 1, "popped": popped,
                 "overflow_event": slots + 1 + refill if over else None, "by": "snapshot"})


def in_tick_overflow_case(slots):
    """`slots` tokens queued on A -> B with delay 4 (none can be delivered before tick 5); C's
    StartSnapshot marker reaches A in tick 1 and A's broadcast meets the full channel inside the tick
    (depthcheck in_tick=True: the full channel cannot pop in that tick)."""
    top = "3\nA 1000\nB 0\nC 0\nA B\nB C\nC A\n"
    ev = [f"send A B {_amount(i)}" for i in range(slots)] + ["snapshot C", "tick 1", "tick 4", "send C A 1"]
    sched = np.zeros(slots + 64, dtype=np.uint8)
    sched[:slots] = 4
    return Case(top, text(ev), ("schedule", sched), slots, 1, {"overflow_event": slots + 1, "time": 1})


# ---- 4. payload history ---------------------------------------------------------------------------

HIST_TOP = "3\nA 100000\nB 0\nC 0\nA B\nB A\nB C\nC A\n"


def hist_case(sends, split=None):
    """B starts a snapshot, then `sends` non-unit sends go out on A -> B: B records them all until A's
    marker, which is queued behind them, arrives -- a span from the first to the last used history
    slot (hist_needed: `sends` rounded up to a power of two, at least 16).  split: the sends after
    the first `split` follow a flush and a second snapshot at B, so the history is reallocated
    between two flushes and the run replayed."""
    pay = [2 + i for i in range(sends)]
    first = sends if split is None else split
    ev = ["snapshot B"] + [f"send A B {p}" for p in pay[:first]]
    if split is not None:
        ev += [FLUSH, "snapshot B"] + [f"send A B {p}" for p in pay[first:]]
    want = [pay[:first]] + ([pay[first:]] if split is not None else [])
    return Case(HIST_TOP, text(ev), ("hash", 31), 64, 2, {"channel": ("A", "B"), "recorded": want})


TRAFFIC_STEPS = 12


def traffic_hist_case(sends):
    """`sends` non-unit host sends on A -> B and TRAFFIC_STEPS steps of synthetic traffic in which
    every node sends one token at every step (threshold 2^32 - 1; A's only out-link is B):
    hist_needed bounds the channel by sends + TRAFFIC_STEPS, and exactly that many tokens are
    delivered on it -- 20 + 12 = 32 fills a history of 32, 21 + 12 grows it to 64.  B's first
    snapshot records from the first slot; its second, started while the last traffic tokens are
    still queued, records the last one.  Event by event, no drain (run_oracle)."""
    top = "2\nA 100000\nB 1000\nA B\nB A\n"
    ev = ["snapshot B"] + [f"send A B {2 + i}" for i in range(sends)] + \
        [f"tick {sends + TRAFFIC_STEPS - 4}", "snapshot B", "tick 40"]
    return Case(top, text(ev), ("hash", 57), 64, 2,
                {"channel": ("A", "B"), "traffic": (4242, 0xffffffff, TRAFFIC_STEPS),
                 "delivered": sends + TRAFFIC_STEPS})


# ---- 5. payload word ------------------------------------------------------------------------------

def payload_case():
    """A holds 2^31 - 1 tokens and sends them all in one packet (one bit below kGMarker) to B, which
    has just started a snapshot and records the packet; later B forwards it back while A's snapshot
    records B -> A.  All delays 0."""
    top = f"3\nA {PAYLOAD_MAX}\nB 0\nC 0\nA B\nB A\nB C\nC A\n"
    ev = ["snapshot B", f"send A B {PAYLOAD_MAX}", "tick 4", "snapshot A", f"send B A {PAYLOAD_MAX}"]
    return Case(top, text(ev), ("schedule", np.zeros(64, dtype=np.uint8)), 16, 2,
                {"recorded": [(0, ("A", "B")), (1, ("B", "A"))]})


# ---- 6. node-block edges --------------------------------------------------------------------------

def block_program(n):
    """A regular_program-style run (traffic, three snapshots, then the drain) on a 3-out regular
    digraph of n nodes: n = 255, 256, 257 and 513 put the last node block at 255, 256, 1 and 1
    nodes."""
    seed = 300 + n
    src, dst = G.regular_graph(n, 3, seed)
    ss, sr = _snaps(n, ((2, None), (2, n - 1), (6, None)), seed)
    return Program(np.full(n, 20), src, dst, 24, traffic_seed=seed + 1, thresh=1 << 30, traffic_steps=24,
                   snap_step=ss, snap_rank=sr, delay_seed=seed + 2, fifo_slots=64)


@functools.lru_cache(maxsize=None)
def block_oracle(n):
    """(program, its drained oracle run), computed once."""
    p = block_program(n)
    return p, oracle_program(p, drain=True)


def single_node_case():
    """One node, no channel (the engine sizes its channel arrays for max(e, 1)), which starts a
    snapshot.  Nothing ever notifies a node without in-links (node.go:149-171 runs on a marker), so
    the reference's drain loops forever: HANG after max_drain = 40 waiting ticks."""
    return Case("1\nA 5\n", "snapshot A\ntick 2\n", ("hash", 5), 16, 1, {"max_drain": 40})


def isolated_ranks_case(start):
    """300 nodes, links r -> r + 1 and r -> r + 7 (mod 300), except that rank 255 (the last node of
    block 0) has no out-link and rank 256 (the first of block 1) no in-link.  A snapshot started at
    rank 256 reaches every node, one started elsewhere every node but rank 256; neither completes at
    rank 256 (no in-link, no marker), so the drain hangs (max_drain 200) in two different states."""
    n = 300
    ids = [f"v{r:03d}" for r in range(n)]
    links = [(r, (r + k) % n) for r in range(n) for k in (1, 7) if r != 255 and (r + k) % n != 256]
    top = topology([(i, 10) for i in ids], [(ids[a], ids[b]) for a, b in links])
    ev = [f"send {ids[r]} {ids[(r + 1) % n]} {2 + r % 3}" for r in (3, 250, 254, 256, 299)] + \
        [f"snapshot {ids[start]}", "tick 2", f"send {ids[256]} {ids[257]} 3"]
    return Case(top, text(ev), ("hash", 9), 16, 1, {"max_drain": 200})


# ---- the cases both test files run ----------------------------------------------------------------

# (tokens in flight, mixed delays after the host draws)
VARIANTS = [(False, False), (True, True)]
CREATION_CASES = [("complete_case", 65), ("hub_case", 129), ("hub_case", 64), ("hub_case", 65)] + \
    [("star_case", k, d) for k in (1, 4, 5) for d in (1, 8, 9, 16)]
CREATION_CASES.append(("skew_case",))
CREATION_RUNS = [c + v for c in CREATION_CASES for v in VARIANTS] + \
    [("last_link_case", link, mixed) for link in (63, 64) for mixed in (False, True)]
RING_SLOTS = (2, 16, 32768)
RING_CASES = [(b, s) for s in RING_SLOTS for b in ("fill_case", "wrap_case")]
HIST_CASES = [("hist_case", 16), ("hist_case", 17), ("hist_case", 17, 16), ("hist_case", 32), ("hist_case", 33),
              ("hist_case", 33, 32), ("traffic_hist_case", 20), ("traffic_hist_case", 21)]
BLOCK_SIZES = (255, 256, 257, 513)
STATE_CASES = [("single_node_case",), ("isolated_ranks_case", 256), ("isolated_ranks_case", 0)]


def case_id(c):
    return "-".join(str(int(x)) if isinstance(x, bool) else str(x) for x in c).replace("_case", "")
