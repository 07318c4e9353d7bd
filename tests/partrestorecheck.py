"""Helpers for the tests of a partitioned run that begins in a restored cut
(cl_graph_part_begin_seeded, PartitionedGraphSim.from_cut / restore / cut).

TEST HELPER.  The numpy statement of a rank's share of a cut, and what the worker processes and
the parent of test_graph_part_restore_gpu.py both need.  A rank owns the queues of its nodes'
out-channels; channels are ordered by (src rank, dest rank), so with out_off the exclusive prefix
of the out-degrees the rank of nodes [lo, hi) owns the channels [out_off[lo], out_off[hi]), and of
a cut's ascending entries the slice between the first entries at or above either bound.  Nothing
here calls the code under test."""
import numpy as np


def out_offsets(n, src):
    """out_off[n + 1] of a channel list in channel order (src ascending)."""
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(np.asarray(src, dtype=np.int64), minlength=n), out=off[1:])
    return off


def spans(n, world):
    """[(lo, hi)] per rank: equal runs of 256-node blocks, as PartitionedGraphSim splits them."""
    blocks = -(-n // 256)
    span = -(-blocks // world) * 256
    return [(min(n, r * span), min(n, (r + 1) * span)) for r in range(world)]


def share(channel, count, out_off, lo, hi):
    """(e_lo, e_hi, m_lo, m_hi) of the rank that owns nodes [lo, hi)."""
    channel = np.asarray(channel, dtype=np.int64)
    moff = np.concatenate([[0], np.cumsum(np.asarray(count, dtype=np.int64))])
    e_lo = int(np.searchsorted(channel, out_off[lo], side="left"))
    e_hi = int(np.searchsorted(channel, out_off[hi], side="left"))
    return e_lo, e_hi, int(moff[e_lo]), int(moff[e_hi])


def brute_share(channel, count, src, lo, hi):
    """The same by walking the entries: those whose channel's sender is in [lo, hi), which must be
    consecutive, and the messages before and through them."""
    mine = [i for i, c in enumerate(channel) if lo <= src[c] < hi]
    before = sum(1 for c in channel if src[c] < lo)
    assert mine == list(range(before, before + len(mine)))
    m_lo = sum(int(count[i]) for i in range(before))
    return before, before + len(mine), m_lo, m_lo + sum(int(count[i]) for i in mine)


def assert_shares_tile(shares, n_entries, n_msgs):
    """The ranks' shares in rank order cover [0, n_entries) and [0, n_msgs) without gap or overlap."""
    e, m = 0, 0
    for e_lo, e_hi, m_lo, m_hi in shares:
        assert (e_lo, m_lo) == (e, m) and e_hi >= e_lo and m_hi >= m_lo, shares
        e, m = e_hi, m_hi
    assert (e, m) == (n_entries, n_msgs), shares
