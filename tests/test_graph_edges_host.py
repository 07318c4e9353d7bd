"""The graph-engine edge cases of tests/graphedges.py on the CPU oracle alone (no GPU): every case
still reaches the regime it exists for -- creations per node and tick, tokens delivered in the
creation tick on both sides of the creating sender, channel peaks equal to fifo_slots, the overflow
event and its time, history slots used, the recorded 2^31 - 1, the node-block sizes.
tests/test_graph_edges_gpu.py runs the same cases on the engine."""
import numpy as np
import pytest

import depthcheck as D
import graphedges as E
import oracle as O


def complete(o):
    return o.status == 0 and o.num_snapshots > 0 and all(o.complete(s) for s in range(o.num_snapshots))


# ---- 1. creations per node and tick ---------------------------------------------------------------

@pytest.mark.parametrize("run", E.CREATION_RUNS, ids=E.case_id)
def test_creations_per_node_and_tick(run):
    c = E.case(*run)
    o = E.oracle_of(*run, log=True)
    assert complete(o) and o.num_snapshots == c.max_snapshots
    cre = E.creations(o)
    most = max(cre.values())
    assert most == c.aim["creations"]
    assert cre[(c.aim["tick"], c.aim["node"])] == most          # at the node and in the tick aimed at
    ids = o.node_ids()
    if not c.aim["token_senders"]:
        assert o.counters()["recorded"] == 0
        return
    assert o.counters()["recorded"] > 0
    # tokens delivered to the colliding node in the creation tick: from below, between (more than one
    # creating sender) and above the creating senders; recorded exactly by the snapshots whose
    # creating sender ranks below the token's
    st = [x for x in E.same_tick_tokens(o) if x[2] == c.aim["node"]]
    assert sorted({x[1] for x in st}) == sorted(c.aim["token_senders"])
    later, earlier = [x for x in st if x[4]], [x for x in st if not x[4]]
    assert later and earlier
    for sid, src, node, pay, was_later in st:
        assert (pay in E.recorded_on(o, c.top, sid, ids[src], ids[node])) == was_later
    lo, mid, hi = c.aim["token_senders"]
    assert not any(x[4] for x in st if x[1] == lo) and all(x[4] for x in st if x[1] == hi)
    if most > 1:
        assert {x[4] for x in st if x[1] == mid} == {True, False}


def test_creation_cases_reach_the_packed_limits():
    """Out-links 63 and 64 (j = 62, 63 of the delivery word) deliver, in-degrees 64 and 65 both
    occur, and the figures the cases were sized with still hold."""
    o = E.oracle_of("complete_case", 65, False, False, log=True)
    top = E.case("complete_case", 65, False, False).top
    ids = o.node_ids()
    links = E.out_links(top)
    assert all(len(v) == 64 for v in links.values())
    used = {links[ids[other]].index(ids[node]) for _, kind, node, other, _, _ in o.log()
            if kind in (E.LOG_RECV_TOKEN, E.LOG_RECV_MARKER)}
    assert used == set(range(64))
    assert (o.counters()["push"], o.time) == (270400, 5254)
    o = E.oracle_of("hub_case", 129, False, False, log=True)
    assert (o.counters()["push"], o.time) == (41538, 8263)
    for leaves in (64, 65, 129):
        top = E.case("hub_case", leaves, False, False).top
        assert sum(1 for _, d in E.channels(top) if d == "h000") == leaves
        assert len(E.out_links(top)["h000"]) == 64


@pytest.mark.parametrize("link", [63, 64])
def test_last_links_deliver_in_a_creation_tick(link):
    """m0 delivers on out-link 63 / 64 (j = 62, 63) in the tick in which a lower-ranked sender's
    marker created a local snapshot at it, and peeked every queue before that link."""
    o = E.oracle_of("last_link_case", link, False, log=True)
    ids = o.node_ids()
    a0, m0, z = ids.index("a0"), ids.index("m0"), ids.index(f"z{link:02d}")
    tick1 = [(kind, node, other) for ep, kind, node, other, _, _ in o.log() if ep == 1]
    assert (E.LOG_RECV_MARKER, m0, a0) in tick1 and (E.LOG_RECV_TOKEN, z, m0) in tick1 and a0 < m0
    links = E.out_links(E.case("last_link_case", link, False).top)["m0"]
    assert len(links) == 64 and links.index(f"z{link:02d}") == link - 1


def test_skew_case_scans_62_links_first():
    """a1 and a2 deliver on the last of 63 out-links in tick 1, g1 and g2 on their only one."""
    c = E.case("skew_case", False, False)
    links = E.out_links(c.top)
    assert [len(links[x]) for x in ("a1", "a2", "g1", "g2")] == [63, 63, 1, 1]
    assert links["a1"][-1] == links["a2"][-1] == "m0"
    assert c.delay[1][:126].tolist() == ([1] * 62 + [0]) * 2


# ---- 2. ring and count field ----------------------------------------------------------------------

@pytest.mark.parametrize("run", E.RING_CASES, ids=E.case_id)
def test_ring_filled_exactly(run):
    c = E.case(*run)
    w = E.walk_of(*run)
    assert w.overflow is None
    assert w.peak_of(*c.aim["channel"]) == c.fifo_slots
    assert complete(w.ref)
    if run[0] == "wrap_case":
        assert c.aim["pushed"] > c.fifo_slots and 0 < c.aim["popped"] < c.fifo_slots
    o = E.oracle_of(*run)            # readEventsFile agrees with the walk
    assert (o.status, o.time, o.counters()) == (0, w.ref.time, w.ref.counters())


# ---- 3. overflow ----------------------------------------------------------------------------------

@pytest.mark.parametrize("run", [c + (True,) for c in E.RING_CASES], ids=E.case_id)
def test_one_more_push_overflows(run):
    c = E.case(*run)
    w = E.walk_of(*run, drain=False)
    ev = D.parse_events(c.events)
    k = c.aim["overflow_event"]
    assert w.overflow is not None and w.overflow[0] == k
    assert ev[k][0] == c.aim["by"]
    assert w.depth_before(k, *c.aim["channel"]) == c.fifo_slots
    assert w.peak_of(*c.aim["channel"]) == c.fifo_slots
    assert any(e[0] == "tick" for e in ev[k + 1:])      # later events exist, and must not run
    assert w.overflow[1] == w.ref.time == (0 if run[0] == "fill_case" else ev[c.fifo_slots][1])


@pytest.mark.parametrize("slots", [2, 16])
def test_in_tick_overflow(slots):
    c = E.case("in_tick_overflow_case", slots)
    w = E.walk_of("in_tick_overflow_case", slots, drain=False, in_tick=True)
    assert w.overflow == (c.aim["overflow_event"], c.aim["time"])
    assert w.peak_of("A", "B") == slots + 1
    # the full channel cannot pop in that tick: every packet on it is due at tick 5
    assert set(c.delay[1][:slots].tolist()) == {4}


# ---- 4. payload history ---------------------------------------------------------------------------

@pytest.mark.parametrize("run", E.HIST_CASES, ids=E.case_id)
def test_history_slots_used(run):
    c = E.case(*run)
    o = E.oracle_of(*run)
    assert complete(o) and o.num_snapshots == 2 - (len(run) == 2 and run[0] == "hist_case")
    rec = [E.recorded_on(o, c.top, s, *c.aim["channel"]) for s in range(o.num_snapshots)]
    if run[0] == "hist_case":
        assert rec == c.aim["recorded"]                 # from the first to the last token delivered
        assert sum(len(r) for r in rec) == run[1]
    else:
        # every token delivered on the channel is recorded by one of the two snapshots: the step-0
        # traffic token in the first history slot, the last traffic token in the last
        assert sum(len(r) for r in rec) == c.aim["delivered"] and rec[0][0] == 1 and rec[1]
        assert rec[0][1:run[1] + 1] == [2 + i for i in range(run[1])]
        assert o.queue_depths().max() == 0


# ---- 5. payload word ------------------------------------------------------------------------------

def test_payload_word_recorded():
    c = E.case("payload_case")
    o = E.oracle_of("payload_case")
    assert complete(o) and o.num_snapshots == 2
    for sid, ch in c.aim["recorded"]:
        assert E.recorded_on(o, c.top, sid, *ch) == [2**31 - 1]
        tok, _, vals = o.collect_channels(sid)
        assert tok.sum() + vals.sum() == 2**31 - 1      # the cut is consistent
    assert o.node_tokens() == {"A": 2**31 - 1, "B": 0, "C": 0}


# ---- 6. node-block edges --------------------------------------------------------------------------

@pytest.mark.parametrize("n", E.BLOCK_SIZES)
def test_block_programs_complete(n):
    p, o = E.block_oracle(n)
    assert p.n == n and np.bincount(p.src, minlength=n).max() == 3
    assert complete(o) and o.num_snapshots == 3
    c = o.counters()
    assert c["recorded"] > 0 and c["pop_tok"] > n


@pytest.mark.parametrize("run", E.STATE_CASES, ids=E.case_id)
def test_nodes_without_links_hang(run):
    c = E.case(*run)
    o = E.oracle_of(*run)
    assert o.status == O.HANG and not o.complete(0)
    if run[0] == "isolated_ranks_case":
        src = [s for s, _ in E.channels(c.top)]
        dst = [d for _, d in E.channels(c.top)]
        assert "v255" not in src and "v256" not in dst and "v255" in dst and "v256" in src
        tok, _, _ = o.collect_channels(0)
        assert (tok[256] >= 0) == (run[1] == 256)        # the marker wave never reaches rank 256
        assert (tok >= 0).sum() == (300 if run[1] == 256 else 299)
