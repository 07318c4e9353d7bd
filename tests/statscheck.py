"""Expected values of ChandyLamportSim.snapshot_stats, computed in numpy from the oracle.

One OracleSim per instance (seed REFERENCE_SEED + i); the flat int64 array is rebuilt field by
field from `status`, `complete(sid)`, `completion_tick(sid)` and `collect_channels(sid)` (already
in channel order), in the layout cl_stats_layout_of reports.
"""
import functools

import numpy as np

import oracle as O
from enginecheck import oracle_run

I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min

# A 5-node ring, max in-degree 1: a node record has 2 words, an instance's 10 record words are
# staged in LDS with scalar loads (rw % 4 != 0).  R2 starts with one token, so many instances
# end with insufficient tokens.  Shared by the statistics, census and select tests.
RING_TOP = "5\nR0 6\nR1 6\nR2 1\nR3 6\nR4 6\nR0 R1\nR1 R2\nR2 R3\nR3 R4\nR4 R0\n"
_RND = "send R0 R1 1\nsend R1 R2 2\nsend R3 R4 1\nsend R0 R1 1\ntick 1\n"
RING_EVENTS = (_RND * 2 + "snapshot R2\n" + "send R4 R0 1\nsend R2 R3 1\ntick 1\n" * 2
               + "snapshot R0\nsend R0 R1 1\nsend R2 R3 1\ntick 2\n")


class Rows:
    """Per-instance oracle results of one scenario: status[n], and per snapshot id the sample
    flags done[n], completion ticks tick[n], tokenMap rows node[n, N], per-channel message counts
    ch_msgs[n, C] and token sums ch_tok[n, C] (zero rows outside the sample)."""

    def __init__(self, refs):
        self.n = len(refs)
        self.status = np.array([r.status for r in refs], dtype=np.int64)
        self.n_sids = max((r.num_snapshots for r in refs), default=0)
        self.done, self.tick, self.node, self.ch_msgs, self.ch_tok = [], [], [], [], []
        n_nodes = len(refs[0].node_ids()) if refs else 0
        n_ch = refs[0].num_links if refs else 0
        for sid in range(self.n_sids):
            done = np.zeros(self.n, dtype=bool)
            tick = np.zeros(self.n, dtype=np.int64)
            node = np.zeros((self.n, n_nodes), dtype=np.int64)
            msgs = np.zeros((self.n, n_ch), dtype=np.int64)
            tok = np.zeros((self.n, n_ch), dtype=np.int64)
            for i, r in enumerate(refs):
                done[i] = r.status == O.OK and sid < r.num_snapshots and r.complete(sid)
                if not done[i]:
                    continue
                tick[i] = r.completion_tick(sid)
                t, off, vals = r.collect_channels(sid)
                node[i] = t
                msgs[i] = np.diff(off)
                tok[i] = np.diff(np.concatenate(([0], np.cumsum(vals)))[off])
            self.done.append(done), self.tick.append(tick)
            self.node.append(node), self.ch_msgs.append(msgs), self.ch_tok.append(tok)


@functools.lru_cache(maxsize=None)
def scenario_rows(top, events, n):
    """Rows of n instances of a (topology, events) scenario (names under test_data or texts);
    computed once and shared by the tests that need it."""
    return Rows([oracle_run(top, events, seed=O.REFERENCE_SEED + i) for i in range(n)])


def expected(layout, rows, sid, lo, hi):
    """The flat array cl_snapshot_stats must return for instances [lo, hi) of `rows`."""
    L = layout
    N, C, T, M = L["n_nodes"], L["n_channels"], L["tick_bins"], L["msg_bins"]
    raw = np.zeros(L["total_words"], dtype=np.int64)
    raw[L["min_begin"]:L["min_end"]] = I64_MAX
    raw[L["max_begin"]:L["max_end"]] = I64_MIN
    raw[L["instances"]] = hi - lo
    raw[L["ok"]] = int((rows.status[lo:hi] == O.OK).sum())
    if sid >= rows.n_sids:  # (no oracle run got as far as starting it)
        return raw
    pick = np.flatnonzero(rows.done[sid][lo:hi]) + lo
    raw[L["sample"]] = pick.size
    if pick.size == 0:
        return raw

    def moments(base, x):
        """x[sample, k] int64: sum, sum of squares modulo 2**64, min, max per column."""
        k = x.shape[1]
        u = x.astype(np.uint64)
        raw[L[base + "_sum"]:L[base + "_sum"] + k] = u.sum(axis=0, dtype=np.uint64).view(np.int64)
        raw[L[base + "_sumsq"]:L[base + "_sumsq"] + k] = (u * u).sum(axis=0, dtype=np.uint64).view(np.int64)
        raw[L["min_" + base]:L["min_" + base] + k] = x.min(axis=0)
        raw[L["max_" + base]:L["max_" + base] + k] = x.max(axis=0)

    tick, node = rows.tick[sid][pick], rows.node[sid][pick]
    msgs, tok = rows.ch_msgs[sid][pick], rows.ch_tok[sid][pick]
    assert node.shape[1] == N and msgs.shape[1] == C
    moments("tick", tick[:, None])
    raw[L["tick_hist"]:L["tick_hist"] + T] = np.bincount(np.clip(tick - L["tick_lo"], 0, T - 1), minlength=T)
    moments("msgs", msgs.sum(axis=1)[:, None])
    moments("inflight", tok.sum(axis=1)[:, None])
    moments("node", node)
    moments("ch_msgs", msgs)
    moments("ch_tok", tok)
    hist = np.zeros((C, M), dtype=np.int64)
    np.add.at(hist, (np.arange(C)[None, :].repeat(pick.size, 0), np.minimum(msgs, M - 1)), 1)
    raw[L["ch_msg_hist"]:L["ch_msg_hist"] + C * M] = hist.ravel()
    return raw


def assert_stats_equal(got, want, layout, what=""):
    """Every field of every section exactly; names the first field that differs."""
    if np.array_equal(got, want):
        return
    bad = int(np.flatnonzero(got != want)[0])
    starts = sorted((off, name) for name, off in layout.items()
                    if name not in ("n_nodes", "n_channels", "tick_lo", "tick_bins", "msg_bins", "total_words")
                    and not name.endswith(("_begin", "_end")))
    name, off = "?", 0
    for o, nm in starts:
        if o <= bad:
            name, off = nm, o
    raise AssertionError(f"{what}: {int((got != want).sum())} words differ; first at {name}[{bad - off}]: "
                         f"got {got[bad]}, expected {want[bad]}")
