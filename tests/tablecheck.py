"""Expected per-snapshot summary table (graph.py SNAP_ROW_DTYPE, include/clgraph.h
cl_graph_snap_row) restated from the CPU oracle alone.

TEST HELPER.  Everything comes from an OracleSim that ran with its Logger on:
  collect_channels(sid)  recorded node tokens (-1: no local snapshot), channel CSR, payloads;
  completion_tick(sid)   the completion tick;
  log()                  the LOG_START record (epoch, node) of every snapshot, and per node the
                         epoch of the first LOG_RECV_MARKER(sid) delivered to it;
  graphcheck.digest_of   the snapshot's term of CL_GSUM_DIGEST.
All comparisons against the engine are exact."""
import functools
import os

import numpy as np

import graphcheck as GC
import oracle as O
from snapcheck import TEST_DATA

LOG_RECV_MARKER, LOG_START = 3, 4          # include/clsnap.h CL_LOG_*
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
DTYPE = GC.clg.SNAP_ROW_DTYPE
PROGRESS = ("sid", "initiator", "start_tick", "complete_tick", "nodes_created", "last_create_tick", "node_tokens",
            "min_node_tokens", "max_node_tokens")
CHANNEL = ("rec_msgs", "rec_tokens", "rec_channels", "max_ch_msgs", "digest")


def creation_epochs(o):
    """(initiator[S], start[S], epoch[S, N]): epoch[sid, v] = Logger epoch at which node v
    created its local snapshot of sid (-1: it has none)."""
    n, s = len(o.node_ids()), o.num_snapshots
    init = np.full(s, -1, dtype=np.int64)
    start = np.full(s, -1, dtype=np.int64)
    ep = np.full((s, n), -1, dtype=np.int64)
    for epoch, kind, node, _, data, _ in o.log():
        if kind == LOG_START:
            init[data], start[data], ep[data, node] = node, epoch, epoch
        elif kind == LOG_RECV_MARKER and ep[data, node] < 0:
            ep[data, node] = epoch
    return init, start, ep


def expected_table(o):
    """The table of every snapshot of a finished oracle run (Logger on)."""
    init, start, ep = creation_epochs(o)
    rows = np.zeros(o.num_snapshots, dtype=DTYPE)
    for sid in range(o.num_snapshots):
        tok, off, vals = o.collect_channels(sid)
        made = tok >= 0
        # the Logger and the local snapshots agree on which nodes hold one
        np.testing.assert_array_equal(made, ep[sid] >= 0)
        r = rows[sid]
        r["sid"], r["initiator"], r["start_tick"] = sid, init[sid], start[sid]
        r["complete_tick"] = o.completion_tick(sid) if o.complete(sid) else -1
        r["nodes_created"] = made.sum()
        r["last_create_tick"] = ep[sid][made].max() if made.any() else -1
        r["node_tokens"] = tok[made].sum()
        r["min_node_tokens"] = tok[made].min() if made.any() else I64_MAX
        r["max_node_tokens"] = tok[made].max() if made.any() else I64_MIN
        if o.complete(sid):
            cnt = np.diff(off)
            r["rec_msgs"], r["rec_tokens"] = cnt.sum(), vals.sum()
            r["rec_channels"] = (cnt > 0).sum()
            r["max_ch_msgs"] = cnt.max() if cnt.size else 0
            r["digest"] = GC.digest_of(sid, tok, off, vals)
    return rows


def assert_rows_equal(got, want, fields=None):
    """Field by field, exact."""
    assert got.shape == want.shape, (got.shape, want.shape)
    for f in fields or DTYPE.names:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"field {f}")


def total_tokens(p):
    return int(np.sum(p.tokens))


def scenario_oracle_logged(top, events, seed):
    """graphcheck.scenario_oracle with the Logger on."""
    o = O.OracleSim()
    o.seed_go(seed)
    o.log_enable()
    assert o.read_topology(os.path.join(TEST_DATA, top)) == 0
    o.read_events(os.path.join(TEST_DATA, events))
    return o


def powerlaw(steps=70):
    return GC.powerlaw_program(2000, steps, 12, fifo_slots=512)


@functools.lru_cache(maxsize=None)
def powerlaw_drained():
    """(program, oracle with the Logger on, expected rows) of the drained power-law run."""
    p = powerlaw()
    o = GC.oracle_program(p, drain=True, log=True)
    return p, o, expected_table(o)


def mixed(o):
    """At least one snapshot complete and one incomplete with a marker wave under way."""
    n = len(o.node_ids())
    done = [o.complete(s) for s in range(o.num_snapshots)]
    part = [not d and 0 < int((o.collect_channels(s)[0] >= 0).sum()) < n for s, d in enumerate(done)]
    return any(done) and any(part)


@functools.lru_cache(maxsize=None)
def powerlaw_undrained():
    """The same program (70 steps of traffic, 12 snapshots) ticked on without a drain and
    stopped at the tick at which the drained oracle run completes its first snapshot: others
    are then still spreading.  (program, oracle with the Logger on, expected rows); the
    caller asserts mixed(o)."""
    p0, _, rows = powerlaw_drained()
    p = powerlaw(int(rows["complete_tick"].min()))
    p.traffic_steps = p0.traffic_steps
    o = GC.oracle_program(p, log=True)
    return p, o, expected_table(o)
