"""The graph engine's tick kernels (cg_kernels.hip) at the limits of their packed words, against the
oracle: the cases of tests/graphedges.py (whose regimes tests/test_graph_edges_host.py asserts on the
oracle alone) on GraphSim, bit for bit -- status, time, node tokens, completion ticks, token maps,
per-channel recorded payloads and all counters (graphcheck.compare); wherever snapshots complete also
the content digest, the per-snapshot table digests and the sparse collect.

* creations per node and tick: 1, 4, 5 (the kRegCre = 4 sorting network and the next_creation walk of
  push_node_lanes, out-degrees 1, 8, 9 and 16 around push_node_reg's chunks of kRegOd = 8), 64 at
  in-degree 64 and 65 at in-degree 65 (kSmallIndeg), 129 on the grid-wide expansion, with tokens
  that arrive in the creation tick from senders below, between and above the creating ones
  (expand_range's same-tick rule) and with out-links 63 and 64 of the delivery word in use; creating
  senders that arrive out of rank order (skew_case) and a delivery on out-link 63 / 64 in a creation
  tick (last_link_case: pk & 63 in k_push);
* the head word's 16-bit count at fifo_slots = 32768 (and 2, 16): filled exactly, wrapped, and one
  push more (FIFO_OVERFLOW: where the run froze);
* the payload history at 16 / 17 and 32 / 33 sends, grown between two flushes, with traffic steps;
* the payload word 2^31 - 1; node blocks at n = 1, 255, 256, 257, 513 and nodes without links.

Reference: sim.go:71-95 (Tick), sim.go:105-123 (StartSnapshot), node.go:97-131, node.go:149-185,
queue.go:6-28 (unbounded: the expected overflow is depthcheck's).
"""
import numpy as np
import pytest

import depthcheck as D
import graphedges as E
from graphcheck import cl, clg, compare, digest_from_oracle, engine_program

pytestmark = pytest.mark.gpu

LANES = [0, 1, 4]


# ---- drivers ------------------------------------------------------------------------------------

def run_engine(case, lanes=0):
    g = clg.GraphSim(fifo_slots=case.fifo_slots, max_snapshots=case.max_snapshots,
                     max_drain_ticks=case.aim.get("max_drain", E.MAX_DRAIN))
    g.set_push_lanes(lanes)
    g.read_topology_text(case.top)
    if case.delay[0] == "schedule":
        g.set_delay_schedule(case.delay[1])
    else:
        g.set_delay_hash(case.delay[1])
    if "traffic" in case.aim:             # event by event, no drain (graphedges.run_oracle)
        g.set_traffic(*case.aim["traffic"])
        for ev in D.parse_events(case.events):
            if ev[0] == "send":
                g.ProcessEvent(cl.PassTokenEvent(ev[1], ev[2], ev[3]))
            elif ev[0] == "snapshot":
                g.StartSnapshot(ev[1])
            else:
                g.Tick(ev[1])
        g.flush()
        return g
    for ev in E.parts(case.events):
        g.read_events_text(ev)
        g.flush()
    return g


def full_compare(g, o):
    """graphcheck.compare, and for the completed snapshots the digest three ways and the sparse
    collect against the dense one."""
    compare(g, o)
    done = [s for s in range(o.num_snapshots) if o.complete(s)]
    if not done:
        return
    assert g.checksums()["digest"] == digest_from_oracle(o)
    rows = g.snapshot_table().rows
    want = [digest_from_oracle(o, [s]) if o.complete(s) else 0 for s in range(o.num_snapshots)]
    np.testing.assert_array_equal(rows["digest"][:o.num_snapshots], np.array(want, dtype=np.int64))
    sp = g.collect_sparse(tokens=True)
    for s in done:
        for a, b in zip(sp.dense(s, g.num_channels), g.collect_arrays(s)):
            np.testing.assert_array_equal(a, b)
        assert sp.digest(s, g.num_nodes, g.num_channels) == want[s]


def rerun_poisoned(g, o):
    """A rerun into result planes filled with 0xA5 reproduces the run."""
    g.poison_outputs()
    g.rerun()
    g.synchronize()
    full_compare(g, o)


def check(run, lanes=0, poisoned=False):
    g = run_engine(E.case(*run), lanes)
    o = E.oracle_of(*run)
    full_compare(g, o)
    if poisoned:
        rerun_poisoned(g, o)
    return g, o


# ---- 1. creations per node and tick ---------------------------------------------------------------

@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("run", E.CREATION_RUNS, ids=E.case_id)
def test_creations_per_node_and_tick(run, lanes):
    g, o = check(run, lanes, poisoned=run == ("star_case", 5, 9, True, True))
    assert g.status() == 0
    sums = g.checksums()
    assert sums["completed"] == o.num_snapshots and sums["cut_residual"] == 0 and sums["final_residual"] == 0


# ---- 2. ring and count field ----------------------------------------------------------------------

# (the full-size ring runs on the automatic push path only: its pushes inside ticks are four markers)
@pytest.mark.parametrize("run,lanes", [(c, ln) for c in E.RING_CASES for ln in (LANES if c[1] < 32768 else [0])],
                         ids=lambda x: E.case_id(x) if isinstance(x, tuple) else f"lanes{x}")
def test_ring_filled_exactly(run, lanes):
    g, _ = check(run, lanes, poisoned=run == ("wrap_case", 16) and lanes == 0)
    sums = g.checksums()
    assert g.status() == 0 and sums["completed"] == 1 and sums["cut_residual"] == 0 and sums["final_residual"] == 0


# ---- 3. overflow ----------------------------------------------------------------------------------

@pytest.mark.parametrize("run", [c + (True,) for c in E.RING_CASES], ids=E.case_id)
def test_one_more_push_freezes_the_run_there(run):
    """The push that meets a full channel is not made and freezes the run: status
    FIFO_OVERFLOW, the time of the last tick that ran, no later event executed.  A StartSnapshot that
    freezes leaves the node tokens as they were; a send has debited its sender before the push
    (node.go:118-124 order), and those tokens are on no channel."""
    c = E.case(*run)
    w = E.walk_of(*run, drain=False)
    g = run_engine(c)
    assert g.status() == cl.INST_FIFO_OVERFLOW
    assert g.time() == w.overflow[1]
    want = dict(w.ref.node_tokens())
    ev = D.parse_events(c.events)[w.overflow[0]]
    if ev[0] == "send":
        want[ev[1]] -= ev[3]
    assert g.node_tokens() == want
    gc, oc = g.counters(), w.ref.counters()
    for k in ("push", "peek", "pop_tok", "pop_mk", "recorded", "completed"):
        assert gc[k] == oc[k], k                        # the walk stopped before the failing event
    assert all(g.snapshot_tick(s) == -1 for s in range(g.num_snapshots))


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("slots", [2, 16])
def test_in_tick_overflow_status(slots, lanes):
    g = run_engine(E.case("in_tick_overflow_case", slots), lanes)
    assert g.status() == cl.INST_FIFO_OVERFLOW


# ---- 4. payload history ---------------------------------------------------------------------------

@pytest.mark.parametrize("run", E.HIST_CASES, ids=E.case_id)
def test_history_slots(run):
    c = E.case(*run)
    g, o = check(run, poisoned=run == ("hist_case", 17, 16))
    assert g.status() == 0                              # never kGStatusHistOverflow
    ch = E.channels(c.top).index(c.aim["channel"])
    for s in range(o.num_snapshots):
        _, off, msg = g.collect_arrays(s)
        assert msg[off[ch]:off[ch + 1]].tolist() == E.recorded_on(o, c.top, s, *c.aim["channel"])


# ---- 5. payload word ------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", LANES)
def test_payload_word(lanes):
    c = E.case("payload_case")
    g, o = check(("payload_case",), lanes, poisoned=lanes == 0)
    sums = g.checksums()
    assert g.status() == 0 and sums["cut_residual"] == 0 and sums["final_residual"] == 0
    for sid, chan in c.aim["recorded"]:
        ch = E.channels(c.top).index(chan)
        _, off, msg = g.collect_arrays(sid)
        assert msg[off[ch]:off[ch + 1]].tolist() == [2**31 - 1]
    assert g.snapshot_table().digest_sum() == sums["digest"]


# ---- 6. node-block edges --------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("n", E.BLOCK_SIZES)
def test_block_sizes(n, lanes):
    p, o = E.block_oracle(n)
    g = engine_program(p, lanes=lanes, drain=True)
    full_compare(g, o)
    sums = g.checksums()
    assert g.status() == 0 and sums["completed"] == 3 and sums["cut_residual"] == 0 and sums["final_residual"] == 0
    if n == 257 and lanes == 0:
        rerun_poisoned(g, o)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("run", E.STATE_CASES, ids=E.case_id)
def test_nodes_without_links(run, lanes):
    g, o = check(run, lanes)
    assert g.status() == cl.INST_HANG
    for s in range(o.num_snapshots):                    # the frozen marker wave, node by node
        stok = g.snapshot_table().rows["nodes_created"][s]
        assert stok == (o.collect_channels(s)[0] >= 0).sum()
