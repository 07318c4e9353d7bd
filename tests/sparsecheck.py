"""Expected sparse packed collect (graph.py SparseSnapshots, include/clgraph.h
cl_graph_collect_sparse) restated from the CPU oracle alone.

TEST HELPER.  Everything comes from an OracleSim:
  collect_channels(sid)  recorded node tokens, channel CSR (channels in (src, dest) rank order:
                         the channel index of GraphSim.channels()), payloads;
  complete(sid)          whether the snapshot completed;
and, for a part of a partitioned run, the channel list's destination ranks (`dst`, the program's
topology: the oracle has no accessor for it).  All comparisons against the engine are exact."""
import numpy as np

import graphcheck as GC

FIELDS = ("complete", "row_offsets", "channel", "count", "msg_offsets", "msg_tokens", "tokens")


def expected_sparse(o, sid_lo, sid_hi, node_lo=0, node_hi=None, dst=None, complete=None):
    """SparseSnapshots of the snapshots [sid_lo, sid_hi) of a finished oracle run, restricted to
    the nodes [node_lo, node_hi) and the channels into them (dst[c] = destination rank of
    channel c; needed for a proper part only).  A channel is kept when it recorded at least one
    message.  `complete` is the oracle's completion of the whole snapshot unless the caller
    passes the flags of [sid_lo, sid_hi) to assume: a part of a partitioned run completes a
    snapshot when its own nodes have, and the oracle's local snapshots of those nodes (node
    tokens, the closed recordings of the channels into them) are final from then on."""
    n = len(o.node_ids())
    node_hi = n if node_hi is None else node_hi
    if (node_lo, node_hi) != (0, n):
        assert dst is not None and len(dst) == o.num_links
        owned = (np.asarray(dst) >= node_lo) & (np.asarray(dst) < node_hi)
    else:
        owned = np.ones(o.num_links, dtype=bool)
    ns = sid_hi - sid_lo
    flags = [o.complete(sid) for sid in range(sid_lo, sid_hi)] if complete is None else list(complete)
    assert len(flags) == ns
    complete = np.zeros(ns, dtype=np.int32)
    row_offsets = np.zeros(ns + 1, dtype=np.int64)
    tokens = np.full((ns, node_hi - node_lo), -1, dtype=np.int32)
    chan, cnt, msgs = [], [], []
    for r, sid in enumerate(range(sid_lo, sid_hi)):
        row_offsets[r + 1] = row_offsets[r]
        if not flags[r]:
            continue
        complete[r] = 1
        tok, off, vals = o.collect_channels(sid)
        tokens[r] = tok[node_lo:node_hi]
        c = np.diff(off)
        keep = np.nonzero((c > 0) & owned)[0]
        chan.append(keep.astype(np.int32))
        cnt.append(c[keep].astype(np.int32))
        msgs.extend(vals[off[k]:off[k + 1]] for k in keep)
        row_offsets[r + 1] += keep.size
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)  # noqa: E731
    return GC.clg.SparseSnapshots(sid_lo, complete, row_offsets, cat(chan, np.int32), cat(cnt, np.int32),
                                  cat(msgs, np.int32), tokens, node_lo, node_hi)


def assert_sparse_equal(got, want, tokens=True, payloads=True, rows=None):
    """Field by field, exact.  rows: compare only these rows (indices into the sid range) --
    their completion, entries, payloads and token rows."""
    assert (got.sid_lo, got.node_lo, got.node_hi) == (want.sid_lo, want.node_lo, want.node_hi)
    assert len(got) == len(want)
    if rows is not None:
        for r in rows:
            sid = got.sid_lo + r
            assert got.complete[r] == want.complete[r], sid
            gc, gn, gp = got.entries(sid)
            wc, wn, wp = want.entries(sid)
            np.testing.assert_array_equal(gc, wc, err_msg=f"channel of sid {sid}")
            np.testing.assert_array_equal(gn, wn, err_msg=f"count of sid {sid}")
            if payloads:
                assert len(gp) == len(wp)
                for a, b in zip(gp, wp):
                    np.testing.assert_array_equal(a, b, err_msg=f"payloads of sid {sid}")
            if tokens:
                np.testing.assert_array_equal(got.tokens[r], want.tokens[r], err_msg=f"tokens of sid {sid}")
        return
    for f in FIELDS:
        if (f == "tokens" and not tokens) or (f == "msg_tokens" and not payloads):
            continue
        a, b = getattr(got, f), getattr(want, f)
        assert a is not None, f
        assert a.dtype == b.dtype, (f, a.dtype, b.dtype)
        np.testing.assert_array_equal(a, b, err_msg=f"field {f}")
