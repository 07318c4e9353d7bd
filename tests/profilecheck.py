"""Expected node and channel profile over a snapshot range (graph.py SnapshotProfile,
include/clgraph.h cl_graph_snapshot_profile) restated from the CPU oracle alone.

TEST HELPER.  Everything comes from an OracleSim that ran with its Logger on:
  sparsecheck.expected_sparse   per snapshot the recorded node tokens and, per channel into the
                                nodes asked for, the recorded messages and their payloads;
  tablecheck.creation_epochs    the start epoch of every snapshot and the creation epoch of every
                                (snapshot, node).
The rest is the arithmetic of clgraph.h, written with numpy over dense [rows, channels] tables.
All comparisons against the engine are exact."""
import functools

import numpy as np

import graphcheck as GC
import sparsecheck as S
import tablecheck as T

clg = GC.clg
PF = {f: i for i, f in enumerate(clg.PROFILE_HEAD)}
I64_MAX, I64_MIN = T.I64_MAX, T.I64_MIN
NODE_IDENTITY = (0, 0, I64_MAX, I64_MIN, 0, I64_MIN, 0, 0)


@functools.lru_cache(maxsize=8)
def _epochs(o):
    """tablecheck.creation_epochs(o), read from the Logger once per oracle run."""
    return T.creation_epochs(o)


def expected_profile(o, sid_lo, sid_hi, use=None, min_msgs=1, msg_bins=64, msg_width=1, origins=None, nodes=True,
                     unit_payloads=1, node_lo=0, node_hi=None, dst=None, complete=None):
    """SnapshotProfile of the snapshots [sid_lo, sid_hi) of a finished oracle run over the nodes
    [node_lo, node_hi) and the channels into them (dst, complete: as for expected_sparse; the
    node rows' in_msgs / in_tokens need dst -- the program's topology -- in every case).  A row
    is used where the mask `use` allows it (None: everywhere) and the snapshot is complete.
    unit_payloads: the head word the engine reports (1 where the program never sends more than one
    token at once); the oracle cannot tell."""
    n, e = len(o.node_ids()), o.num_links
    node_hi = n if node_hi is None else node_hi
    ns = sid_hi - sid_lo
    sp = S.expected_sparse(o, sid_lo, sid_hi, node_lo, node_hi, dst, complete)
    owned = np.ones(e, dtype=bool) if (node_lo, node_hi) == (0, n) else \
        (np.asarray(dst) >= node_lo) & (np.asarray(dst) < node_hi)
    used = sp.complete.copy()
    if use is not None:
        used &= (np.asarray(use).reshape(-1) != 0).astype(np.int32)
    rows = np.nonzero(used)[0]
    # k[r, c], t[r, c]: messages and payload sum snapshot sid_lo + r recorded on channel c
    k = np.zeros((ns, e), dtype=np.int64)
    t = np.zeros((ns, e), dtype=np.int64)
    for r in rows:
        a, b = int(sp.row_offsets[r]), int(sp.row_offsets[r + 1])
        if b > a:                            # (every entry holds a message: the segments are not empty)
            k[r, sp.channel[a:b]] = sp.count[a:b]
            t[r, sp.channel[a:b]] = np.add.reduceat(sp.msg_tokens[:sp.msg_offsets[b]].astype(np.int64),
                                                    sp.msg_offsets[a:b])
    ku, tu = k[rows], t[rows]
    msgs, tokens = ku.sum(axis=0), tu.sum(axis=0)
    snaps = (ku > 0).sum(axis=0)
    peak = ku.max(axis=0) if rows.size else np.zeros(e, dtype=np.int64)
    # the lowest used sid that attains the peak, -1 where nothing was recorded
    peak_sid = np.full(e, -1, dtype=np.int64)
    if rows.size:
        first = (ku == peak[None, :]).argmax(axis=0)
        peak_sid = np.where(msgs > 0, sid_lo + rows[first], -1)
    head = np.zeros(len(clg.PROFILE_HEAD), dtype=np.int64)
    keep = np.nonzero(owned & (msgs >= min_msgs))[0]
    for f, v in (("n_sids", ns), ("n_used", rows.size), ("node_lo", node_lo), ("node_hi", node_hi),
                 ("channels", owned.sum()), ("active", (owned & (msgs > 0)).sum()), ("entries", keep.size),
                 ("msgs", msgs[owned].sum()), ("tokens", tokens[owned].sum()),
                 ("max_msgs", msgs[owned].max() if owned.any() else 0),
                 ("max_peak", peak[owned].max() if owned.any() else 0),
                 ("max_snaps", snaps[owned].max() if owned.any() else 0), ("unit_payloads", unit_payloads)):
        head[PF[f]] = v
    if ns == 0:
        head[:] = 0
        head[PF["node_lo"]], head[PF["node_hi"]] = node_lo, node_hi
    hist = np.zeros(msg_bins, dtype=np.int64)
    if ns:
        hist += np.bincount(np.minimum(msgs[owned] // msg_width, msg_bins - 1), minlength=msg_bins)
    entries = np.zeros(keep.size if ns else 0, dtype=clg.PROFILE_ENTRY_DTYPE)
    if ns:
        entries["channel"], entries["snaps"], entries["peak"] = keep, snaps[keep], peak[keep]
        entries["peak_sid"], entries["msgs"], entries["tokens"] = peak_sid[keep], msgs[keep], tokens[keep]
    node = None
    if nodes:
        _, start, ep = _epochs(o)
        org = start[sid_lo:sid_hi] if origins is None else np.asarray(origins, dtype=np.int64)
        node = np.zeros(node_hi - node_lo, dtype=clg.PROFILE_NODE_DTYPE)
        node[:] = NODE_IDENTITY
        if rows.size:
            tok = sp.tokens[rows].astype(np.int64)                          # [used, nodes]
            assert (tok >= 0).all()                                         # a used snapshot is complete
            lat = ep[sid_lo + rows][:, node_lo:node_hi] - org[rows][:, None]
            node["tok_sum"], node["tok_sumsq"] = tok.sum(axis=0), (tok * tok).sum(axis=0)
            node["tok_min"], node["tok_max"] = tok.min(axis=0), tok.max(axis=0)
            node["lat_sum"], node["lat_max"] = lat.sum(axis=0), lat.max(axis=0)
            assert dst is not None and len(dst) == e, "the node rows need the channels' destination ranks"
            at = np.asarray(dst, dtype=np.int64)[owned] - node_lo
            np.add.at(node["in_msgs"], at, msgs[owned])
            np.add.at(node["in_tokens"], at, tokens[owned])
    return clg.SnapshotProfile(sid_lo, used, head, hist, entries, node,
                               None if origins is None else np.asarray(origins, dtype=np.int64), msg_width, min_msgs)


def assert_profile_equal(got, want, nodes=True):
    """Field by field, exact; then the objects' own ==."""
    assert (got.sid_lo, got.spec) == (want.sid_lo, want.spec)
    np.testing.assert_array_equal(got.used, want.used, err_msg="used")
    for f, i in PF.items():
        assert got.head[i] == want.head[i], (f, int(got.head[i]), int(want.head[i]))
    np.testing.assert_array_equal(got.hist, want.hist, err_msg="hist")
    assert got.entries.dtype == want.entries.dtype == clg.PROFILE_ENTRY_DTYPE
    for f in clg.PROFILE_ENTRY_DTYPE.names:
        np.testing.assert_array_equal(got.entries[f], want.entries[f], err_msg=f"entries.{f}")
    if nodes:
        assert got.node is not None and want.node is not None
        for f in clg.PROFILE_NODE_FIELDS:
            np.testing.assert_array_equal(got.node[f], want.node[f], err_msg=f"node.{f}")
    else:
        assert got.node is None
    assert (got.origins is None) == (want.origins is None)
    if got.origins is not None:
        np.testing.assert_array_equal(got.origins, want.origins, err_msg="origins")
    if nodes == (want.node is not None):
        assert got == want
