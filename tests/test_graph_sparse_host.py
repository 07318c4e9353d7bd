"""CPU-only tests of the graph engine's sparse packed collect: the exported symbols and the
info record against include/clgraph.h, the argument checks and the empty range (answered
without a device), the loud failure without a GPU, and SparseSnapshots' host functions
(merge, dense, digest, snapshot) on hand-made objects."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import graphcheck as GC
from snapcheck import ROOT, TEST_DATA

cl, clg = GC.cl, GC.clg
SS = clg.SparseSnapshots


def test_symbols_signatures_and_info_layout():
    L = clg.glib()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert L.cl_graph_collect_sparse.argtypes == [vp, i32, i32, vp, vp, vp, vp, i64, vp, i64, vp, vp]
    assert L.cl_graph_sparse_time.argtypes == [vp, vp]
    assert L.cl_graph_collect_sparse.restype == L.cl_graph_sparse_time.restype == C.c_int
    assert clg.SPARSE_INFO_DTYPE.itemsize == 64
    text = open(os.path.join(ROOT, "include", "clgraph.h")).read()
    body = re.search(r"typedef struct cl_graph_sparse_info \{(.*?)\} cl_graph_sparse_info;", text, re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"^\s*int64_t\s+([\w, ]+);", body, re.M) for f in decl.split(",")]
    assert fields == list(clg.SPARSE_INFO_DTYPE.names)
    assert [clg.SPARSE_INFO_DTYPE.fields[f][1] for f in fields] == [8 * i for i in range(8)]
    assert hasattr(clg.GraphSim, "collect_sparse") and hasattr(clg.GraphSim, "sparse_time")
    assert hasattr(clg.PartitionedGraphSim, "collect_sparse")


def small_graph():
    g = clg.GraphSim()
    g.read_topology_file(os.path.join(TEST_DATA, "2nodes.top"))
    g.StartSnapshot("N1")
    g.Tick(1)
    return g


def test_invalid_arguments_are_answered_without_a_device():
    g = small_graph()                        # one snapshot, nothing flushed
    L, h = g._L, g._h
    info = np.zeros(1, dtype=clg.SPARSE_INFO_DTYPE)
    a = np.zeros(4, dtype=np.int32)
    p = cl._p
    call = lambda lo, hi, ch, cn, ecap, msg, mcap, inf: L.cl_graph_collect_sparse(  # noqa: E731
        h, lo, hi, None, None, ch, cn, ecap, msg, mcap, None, inf)
    assert call(0, 1, None, None, 0, None, 0, None) == cl.E_INVALID          # null info
    for lo, hi in ((-1, 1), (1, 0), (0, 2), (2, 2)):
        assert call(lo, hi, None, None, 0, None, 0, p(info)) == cl.E_INVALID, (lo, hi)
    assert call(0, 1, p(a), p(a), -1, None, 0, p(info)) == cl.E_INVALID      # negative caps
    assert call(0, 1, None, None, 0, p(a), -1, p(info)) == cl.E_INVALID
    assert call(0, 1, None, p(a), 4, None, 0, p(info)) == cl.E_INVALID       # null entry arrays, ent_cap > 0
    assert call(0, 1, p(a), None, 4, None, 0, p(info)) == cl.E_INVALID
    t = C.c_double(0)
    assert L.cl_graph_sparse_time(h, C.byref(t)) == cl.E_STATE               # nothing has run
    assert L.cl_graph_sparse_time(h, None) == cl.E_INVALID


def test_empty_range_needs_no_device():
    g = small_graph()
    for lo in (0, 1):
        rc, info = g._collect_sparse(lo, lo)
        assert rc == 0
        assert [int(info[f]) for f in clg.SPARSE_INFO_FIELDS] == [0, 0, 0, 0, 0, 0, 2, 0]
    s = g.collect_sparse(1, 1, tokens=True)
    assert len(s) == 0 and s.n_entries == 0 and s.row_offsets.tolist() == [0]
    assert s.tokens.shape == (0, 2) and (s.node_lo, s.node_hi) == (0, 2)


def test_no_gpu_fails_loudly():
    """Like every other result query: no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    g = small_graph()
    with pytest.raises(cl.ClSnapError) as e:
        g.collect_sparse()
    assert e.value.code == cl.E_DEVICE


# Two parts of a 4-node run over 6 channels: part A owns nodes [0, 2), part B [2, 4); the parts'
# channels interleave.  Snapshot 5 is complete on both, 6 on A only, 7 on both without entries.
def hand_parts():
    a = SS(5, [1, 1, 1], [0, 2, 3, 3], [1, 4, 4], [2, 1, 3], [7, 8, 9, 1, 1, 1],
           [[10, 11], [12, 13], [14, 15]], 0, 2)
    b = SS(5, [1, 0, 1], [0, 3, 3, 3], [0, 3, 5], [1, 2, 1], [3, 4, 5, 6], [[20, 21], [-1, -1], [24, 25]], 2, 4)
    return a, b


def test_merge_sorts_interleaved_channels_per_sid():
    a, b = hand_parts()
    for parts in ((a, b), (b, a)):
        m = SS.merge(parts)
        assert (m.sid_lo, m.node_lo, m.node_hi) == (5, 0, 4)
        assert m.complete.tolist() == [1, 0, 1]
        assert m.row_offsets.tolist() == [0, 5, 5, 5]
        assert m.channel.tolist() == [0, 1, 3, 4, 5]
        assert m.count.tolist() == [1, 2, 2, 1, 1]
        assert m.msg_offsets.tolist() == [0, 1, 3, 5, 6, 7]
        assert m.msg_tokens.tolist() == [3, 7, 8, 4, 5, 9, 6]
        assert m.tokens.tolist() == [[10, 11, 20, 21], [-1, -1, -1, -1], [14, 15, 24, 25]]
        assert m.channel.dtype == m.count.dtype == m.msg_tokens.dtype == m.tokens.dtype == np.int32
    assert SS.merge((a, b)) == SS.merge((b, a)) and SS.merge((a, b)) != a
    assert SS.merge([a]) == a


def test_merge_drops_a_sid_that_one_part_has_not_completed():
    a, b = hand_parts()
    m = SS.merge((a, b))
    ch, cnt, pay = m.entries(6)              # complete on part A (one entry there), not on B
    assert m.complete[1] == 0 and ch.size == 0 and cnt.size == 0 and pay == []
    assert (m.tokens[1] == -1).all()
    with pytest.raises(cl.ClSnapError) as e:
        m.dense(6, 6)
    assert e.value.code == cl.E_NOT_COMPLETE
    ch, cnt, pay = m.entries(7)
    assert m.complete[2] == 1 and ch.size == 0 and pay == []
    # without payloads or tokens on one part the merge carries none
    nb = SS(5, b.complete, b.row_offsets, b.channel, b.count, None, None, 2, 4)
    m2 = SS.merge((a, nb))
    assert m2.msg_tokens is None and m2.tokens is None and m2.channel.tolist() == m.channel.tolist()


def test_merge_refuses_other_sids_and_gaps():
    a, b = hand_parts()
    with pytest.raises(ValueError):
        SS.merge((a, SS(6, b.complete, b.row_offsets, b.channel, b.count, b.msg_tokens, b.tokens, 2, 4)))
    with pytest.raises(ValueError):
        SS.merge((a, SS(5, b.complete, b.row_offsets, b.channel, b.count, b.msg_tokens, b.tokens.reshape(3, 2), 3, 5)))
    with pytest.raises(ValueError):
        SS(5, [1], [0, 2], [1], [1])         # row_offsets past the entries


def test_dense_and_digest_agree_with_the_dense_digest():
    a, b = hand_parts()
    m = SS.merge((a, b))
    for sid in (5, 7):
        tok, off, msg = m.dense(sid, 6)
        assert tok.dtype == off.dtype == msg.dtype == np.int64
        assert m.digest(sid, 4, 6) == GC.digest_of(sid, tok, off, msg)
    tok, off, msg = m.dense(5, 6)
    assert tok.tolist() == [10, 11, 20, 21]
    assert off.tolist() == [0, 1, 3, 3, 5, 6, 7] and msg.tolist() == [3, 7, 8, 4, 5, 9, 6]
    assert m.dense(7, 6)[1].tolist() == [0] * 7 and m.dense(7, 6)[2].size == 0
    # the digest depends on every part of the content
    assert m.digest(5, 4, 6) != m.digest(7, 4, 6)
    big = SS(0, [1], [0, 1], [2], [2], [2**31 - 1, 2**31 - 1], [[-5, 7]], 0, 2)     # sums wrap at 32 bits
    tok, off, msg = big.dense(0, 3)
    assert big.digest(0, 2, 3) == GC.digest_of(0, tok, off, msg)
    with pytest.raises(ValueError):
        a.digest(5, 4, 6)                    # a part: not every node's tokens
    with pytest.raises(IndexError):
        m.entries(8)


class FakeSim:
    def node_ids(self):
        return ["N0", "N1", "N2", "N3"]

    def channels(self):
        return (np.array([0, 0, 1, 2, 3, 3], dtype=np.int32), np.array([2, 1, 0, 3, 0, 2], dtype=np.int32))


def test_snapshot_orders_messages_by_dest_src_delivery():
    a, b = hand_parts()
    s = SS.merge((a, b)).snapshot(5, FakeSim())
    assert s.id == 5 and s.tokenMap == {"N0": 10, "N1": 11, "N2": 20, "N3": 21}
    assert [m.astuple() for m in s.messages] == [("N3", "N0", 9), ("N0", "N1", 7), ("N0", "N1", 8), ("N0", "N2", 3),
                                                 ("N3", "N2", 6), ("N2", "N3", 4), ("N2", "N3", 5)]
