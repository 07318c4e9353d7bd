"""CPU-only tests of the restore from a host-held cut (cl_graph_restore_cut, GraphSim.restore_cut,
SnapshotCut, topology_key): the exported symbol and the cl_graph_cut record against
include/clgraph.h, every error that is answered before any device work, and the pure host parts
-- SnapshotCut with its file round trip, SparseSnapshots.cut on synthetic objects, the topology
key.  (A partitioned template can only be made with a device: that error is in the GPU file.)"""
import ctypes as C
import hashlib
import os
import re
import struct

import numpy as np
import pytest

import graphcheck as GC
from snapcheck import ROOT, TEST_DATA

cl, clg = GC.cl, GC.clg
POISON = 0xdead


def test_symbol_signature_and_record_layout():
    L = clg.glib()
    assert L.cl_graph_restore_cut.argtypes == [C.c_void_p, C.POINTER(clg.GraphCut), C.POINTER(C.c_void_p)]
    assert L.cl_graph_restore_cut.restype == C.c_int
    assert C.sizeof(clg.GraphCut) == 64
    text = open(os.path.join(ROOT, "include", "clgraph.h")).read()
    body = re.search(r"typedef struct cl_graph_cut \{(.*?)\} cl_graph_cut;", text, re.S).group(1)
    decl = re.findall(r"^\s*(int64_t|const int32_t\*)\s+(\w+);", body, re.M)
    assert [name for _, name in decl] == [f for f, _ in clg.GraphCut._fields_]
    ctype = {"int64_t": C.c_int64, "const int32_t*": C.POINTER(C.c_int32)}
    assert [ctype[t] for t, _ in decl] == [t for _, t in clg.GraphCut._fields_]
    assert [getattr(clg.GraphCut, f).offset for f, _ in clg.GraphCut._fields_] == [8 * i for i in range(8)]
    assert re.search(r"int cl_graph_restore_cut\(cl_graph\* topo, const cl_graph_cut\* cut, cl_graph\*\* out\);", text)
    for name in ("cut", "restore_cut", "from_cut", "topology_key"):
        assert hasattr(clg.GraphSim, name)
    assert hasattr(clg.SparseSnapshots, "cut")


def template():
    """The 2-node topology (2 channels), never run."""
    g = clg.GraphSim()
    g.read_topology_file(os.path.join(TEST_DATA, "2nodes.top"))
    return g


def i32(*v):
    return np.array(v, dtype=np.int32)


def record(tokens=i32(1, 0), channel=i32(0), count=i32(2), msgs=i32(1, 1), n_nodes=None, n_entries=None, n_msgs=None):
    """A cl_graph_cut over the given arrays (None: a NULL pointer); the lengths default to the arrays'."""
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    size = lambda a: 0 if a is None else a.size  # noqa: E731
    rec = clg.GraphCut(7, size(tokens) if n_nodes is None else n_nodes, ptr(tokens),
                       size(channel) if n_entries is None else n_entries, ptr(channel), ptr(count),
                       size(msgs) if n_msgs is None else n_msgs, ptr(msgs))
    rec._keep = (tokens, channel, count, msgs)
    return rec


def call(g, rec):
    out = C.c_void_p(POISON)
    rc = g._L.cl_graph_restore_cut(g._h, None if rec is None else C.byref(rec), C.byref(out))
    assert out.value is None, "*out must be reset to NULL"
    return rc


def test_a_valid_record_reaches_the_device_step():
    """The control of the cases below: nothing on the host refuses the record they vary.  Without a
    device the call then fails in the device step; with one it succeeds."""
    g = template()
    assert (g.num_nodes, g.num_channels) == (2, 2)
    out = C.c_void_p(POISON)
    rc = g._L.cl_graph_restore_cut(g._h, C.byref(record()), C.byref(out))
    assert rc in (cl.E_DEVICE, 0)
    if rc == 0:
        g._L.cl_graph_destroy(out)
    else:
        assert out.value is None


@pytest.mark.parametrize("name,kw", [
    ("negative n_nodes", dict(n_nodes=-1)),
    ("negative n_entries", dict(n_entries=-1)),
    ("negative n_msgs", dict(n_msgs=-1)),
    ("null tokens", dict(tokens=None, n_nodes=2)),
    ("null channel", dict(channel=None, n_entries=1)),
    ("null count", dict(count=None, n_entries=1)),
    ("n_nodes below N", dict(tokens=i32(1))),
    ("n_nodes above N", dict(tokens=i32(1, 0, 0))),
    ("n_entries above E", dict(channel=i32(0, 1, 2), count=i32(1, 1, 1), msgs=i32(1, 1, 1))),
    ("n_msgs below n_entries", dict(channel=i32(0, 1), count=i32(1, 1), msgs=i32(1))),
    ("n_msgs above n_entries * 32768", dict(msgs=None, n_msgs=32769)),
    ("messages without entries", dict(channel=None, count=None, n_entries=0, msgs=i32(1))),
])
def test_invalid_records_are_answered_without_a_device(name, kw):
    g = template()
    assert call(g, record(**kw)) == cl.E_INVALID, name
    assert cl.lib().cl_last_error()


def test_null_handles_and_state_errors_are_answered_without_a_device():
    g = template()
    L = g._L
    out = C.c_void_p(POISON)
    assert L.cl_graph_restore_cut(None, C.byref(record()), C.byref(out)) == cl.E_INVALID and out.value is None
    assert call(g, None) == cl.E_INVALID
    assert L.cl_graph_restore_cut(g._h, C.byref(record()), None) == cl.E_INVALID
    empty = clg.GraphSim()                   # no nodes: an empty cut has the right lengths and still cannot be used
    assert call(empty, record(tokens=None, channel=None, count=None, msgs=None)) == cl.E_STATE
    assert call(empty, record()) == cl.E_STATE


# ---- SnapshotCut -------------------------------------------------------------------------------
def hand_cut(**kw):
    """5 nodes, 6 channels; entries on channels 1 (2 messages), 2 (1) and 5 (3)."""
    a = dict(tokens=[4, 0, 9, 1, 7], channel=[1, 2, 5], count=[2, 1, 3], msg_tokens=[3, 1, 4, 1, 5, 9], n_channels=6,
             topology_key=123456789012345678)
    a.update(kw)
    return clg.SnapshotCut(11, **a)


TOPO = dict(src=[0, 0, 1, 2, 3, 4], dst=[1, 2, 2, 3, 4, 0], ids=np.array([b"a", b"bb", b"c", b"d", b"e"]))


def test_cut_derived_values():
    c = hand_cut()
    assert (c.source_sid, c.msgs, c.channels, c.payload_tokens) == (11, 6, 3, 23)
    assert c.info() == {"source_sid": 11, "channels": 3, "msgs": 6, "tokens": 23, "max_ch_msgs": 3, "unit_payloads": 0,
                        "node_tokens": 21}
    tok, off, msg = c.dense()
    assert tok.dtype == off.dtype == msg.dtype == np.int64
    assert tok.tolist() == [4, 0, 9, 1, 7] and off.tolist() == [0, 0, 2, 3, 3, 3, 6] and msg.tolist() == [3, 1, 4, 1, 5, 9]
    u = hand_cut(msg_tokens=None)
    assert (u.msgs, u.payload_tokens, u.info()["unit_payloads"], u.info()["tokens"]) == (6, 6, 1, 6)
    assert u.dense()[2].tolist() == [1] * 6
    assert hand_cut(msg_tokens=[1] * 6).info()["unit_payloads"] == 1
    e = clg.SnapshotCut(0, [1, 2], [], [], n_channels=2)
    assert (e.msgs, e.channels, e.info()["max_ch_msgs"]) == (0, 0, 0) and e.dense()[1].tolist() == [0, 0, 0]
    assert c == hand_cut() and c != u and c != hand_cut(tokens=[4, 0, 9, 1, 8]) and c != hand_cut(topology_key=1)
    assert c != hand_cut(**TOPO) and hand_cut(**TOPO) == hand_cut(**TOPO)
    assert (c == 5) is False


@pytest.mark.parametrize("kw", [
    dict(count=[2, 1]),                                  # channel and count differ
    dict(msg_tokens=[3, 1, 4, 1, 5]),                    # one payload short
    dict(msg_tokens=[3, 1, 4, 1, 5, 9, 2]),              # one too many
    dict(n_channels=2),                                  # more entries than channels
    dict(src=TOPO["src"]),                               # the topology comes whole
    dict(src=TOPO["src"], dst=TOPO["dst"]),
    dict(TOPO, dst=TOPO["dst"][:5]),
    dict(TOPO, n_channels=7),
    dict(TOPO, ids=np.array([b"a", b"b"])),
])
def test_cut_constructor_refuses_inconsistent_lengths(kw):
    with pytest.raises(ValueError):
        hand_cut(**kw)


@pytest.mark.parametrize("kw", [dict(), dict(TOPO), dict(msg_tokens=None), dict(TOPO, msg_tokens=None),
                                dict(n_channels=None, topology_key=None), dict(topology_key=2**64 - 1)])
def test_cut_file_round_trip(kw, tmp_path):
    c = hand_cut(**kw)
    path = str(tmp_path / "cut.npz")
    c.save(path)
    with np.load(path, allow_pickle=False) as z:          # plain arrays only
        assert all(z[f].dtype.kind in "iuS" for f in z.files)
    d = clg.SnapshotCut.load(path)
    assert d == c and (d.source_sid, d.n_channels, d.topology_key) == (c.source_sid, c.n_channels, c.topology_key)
    for f in ("tokens", "channel", "count", "msg_tokens", "src", "dst", "ids"):
        a, b = getattr(c, f), getattr(d, f)
        assert (a is None) == (b is None), f
        if a is not None:
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f
    assert d.has_topology == ("src" in kw)


# ---- SparseSnapshots.cut -----------------------------------------------------------------------
class FakeSim:
    """What SparseSnapshots.cut asks of a sim."""
    num_nodes, num_channels = 3, 4

    def topology_key(self):
        return 99

    def channels(self):
        return i32(0, 0, 1, 2), i32(1, 2, 2, 0)

    def node_ids(self):
        return ["x", "y", "zz"]


def sparse(**kw):
    """Snapshots 5..7 of 3 nodes: 5 complete with entries on channels 0 and 3, 6 incomplete, 7 complete and empty."""
    a = dict(complete=[1, 0, 1], row_offsets=[0, 2, 2, 2], channel=[0, 3], count=[1, 2], msg_tokens=[7, 1, 2],
             tokens=[[3, 4, 5], [-1, -1, -1], [6, 6, 0]], node_lo=0, node_hi=3)
    a.update(kw)
    return clg.SparseSnapshots(5, **a)


def test_sparse_snapshots_cut():
    sim = FakeSim()
    c = sparse().cut(5, sim=sim)
    assert c == clg.SnapshotCut(5, [3, 4, 5], [0, 3], [1, 2], [7, 1, 2], n_channels=4, topology_key=99)
    assert sparse().cut(7, sim=sim) == clg.SnapshotCut(7, [6, 6, 0], [], [], [], n_channels=4, topology_key=99)
    t = sparse().cut(5, sim=sim, topology=True)
    assert t.has_topology and t.src.tolist() == [0, 0, 1, 2] and t.dst.tolist() == [1, 2, 2, 0]
    assert t.ids.tolist() == [b"x", b"y", b"zz"]
    bare = sparse().cut(5)
    assert (bare.n_channels, bare.topology_key) == (None, None) and bare.tokens.tolist() == [3, 4, 5]
    with pytest.raises(cl.ClSnapError) as e:
        sparse().cut(6, sim=sim)
    assert e.value.code == cl.E_NOT_COMPLETE
    with pytest.raises(IndexError):
        sparse().cut(8, sim=sim)
    for bad in (sparse(tokens=None), sparse(msg_tokens=None),
                sparse(tokens=[[4, 5], [-1, -1], [6, 0]], node_lo=1),             # a part: not all nodes
                sparse(tokens=[[3, 4], [-1, -1], [6, 6]], node_hi=2)):
        with pytest.raises(ValueError):
            bad.cut(5, sim=sim)
    with pytest.raises(ValueError):
        sparse().cut(5, topology=True)                    # no sim to take it from


# ---- topology_key ------------------------------------------------------------------------------
def test_topology_key():
    src, dst = [0, 0, 1, 2], [1, 2, 2, 0]
    key = clg.topology_key(3, src, dst)
    raw = struct.pack("<qq", 3, 4) + struct.pack("<4i", *src) + struct.pack("<4i", *dst)
    assert key == int.from_bytes(hashlib.blake2b(raw, digest_size=8).digest(), "little")
    assert clg.topology_key(2, [0, 1], [1, 0]) == 6219321262831889755          # known answer
    assert clg.topology_key(3, np.array(src, dtype=np.int64), np.array(dst, dtype=np.int16)) == key   # any int dtype
    assert clg.topology_key(3, [0, 0, 1, 2], [1, 2, 0, 0]) != key               # one edge changed
    assert clg.topology_key(3, dst, src) != key                                 # src and dst swapped
    assert clg.topology_key(4, src, dst) != key
    with pytest.raises(ValueError):
        clg.topology_key(3, src, dst[:3])
    g = template()
    s, d = g.channels()
    assert (s.tolist(), d.tolist()) == ([0, 1], [1, 0])
    assert g.topology_key() == clg.topology_key(2, s, d) == 6219321262831889755


def test_restore_cut_refuses_another_topology_before_the_native_call():
    g = template()
    calls = []

    class Spy:
        """The library with cl_graph_restore_cut recorded instead of called."""
        def __init__(self, L):
            self._L = L

        def __getattr__(self, name):
            if name == "cl_graph_restore_cut":
                return lambda *a: calls.append(a) or cl.E_DEVICE
            return getattr(self._L, name)

    g._L = Spy(g._L)
    ok = dict(n_channels=2, topology_key=g.topology_key())
    for kw in (dict(ok, topology_key=g.topology_key() ^ 1), dict(ok, n_channels=3), dict(ok, topology_key=None),
               dict(ok, n_channels=None)):
        with pytest.raises(ValueError):
            g.restore_cut(clg.SnapshotCut(0, [1, 0], [0], [2], [1, 1], **kw))
    with pytest.raises(TypeError):
        g.restore_cut(([1, 0], [0], [2]))
    assert calls == []
    with pytest.raises(cl.ClSnapError):                   # the matching cut is the one that goes through
        g.restore_cut(clg.SnapshotCut(0, [1, 0], [0], [2], [1, 1], **ok))
    assert len(calls) == 1
    with pytest.raises(ValueError):
        clg.GraphSim.from_cut(clg.SnapshotCut(0, [1, 0], [0], [2], [1, 1], **ok))    # saved without its topology


def test_from_cut_builds_the_template_on_the_host():
    """The template of from_cut is host work: the bulk rule for the ids, the saved order.  The
    native restore that follows needs a device."""
    assert clg._bulk_id_width(np.array([b"N00", b"N01", b"N02"])) == 2
    assert clg._bulk_id_width(np.array([b"N0", b"N1"])) == 1
    for ids in ([b"N1", b"N10", b"N2"], [b"N1", b"N0"], [b"M0", b"N1"], [b"N0", b"N2"], [b"a", b"b"], [b"N0", b"Nx"]):
        assert clg._bulk_id_width(np.array(ids)) == 0, ids
    src, dst = [0, 1, 2], [1, 2, 0]
    key = clg.topology_key(3, src, dst)
    cut = lambda ids: clg.SnapshotCut(0, [1, 2, 3], [0], [1], [1], n_channels=3, topology_key=key, src=src, dst=dst,  # noqa: E731
                                      ids=np.array(ids))
    with pytest.raises(ValueError, match="rank order"):
        clg.GraphSim.from_cut(cut([b"b", b"a", b"c"]))                # ids that sort differently
    for ids in ([b"N00", b"N01", b"N02"], [b"a", b"b", b"c"]):        # bulk and node by node: both reach the native call
        try:
            r = clg.GraphSim.from_cut(cut(ids))
        except cl.ClSnapError as e:
            assert e.code == cl.E_DEVICE
        else:
            assert r.node_ids() == [i.decode() for i in ids]


def test_a_forked_child_does_not_destroy_its_parents_graphs():
    """A graph belongs to the process that made it: a forked child (a multiprocessing manager, a
    pool worker) holds copies of the parent's GraphSim objects, and when its garbage collector
    finalises one, no native call may follow -- the native graph's device state is the parent's.
    Host only: the graphs here never reach a device."""
    destroyed = []

    class Spy:
        """The library with cl_graph_destroy recorded before it is called."""
        def __init__(self, L):
            self._L = L

        def __getattr__(self, name):
            f = getattr(self._L, name)
            if name != "cl_graph_destroy":
                return f
            return lambda h: destroyed.append(os.getpid()) or f(h)

    g, other = template(), template()
    g._L = other._L = Spy(g._L)
    assert g._pid == other._pid == os.getpid()
    r, w = os.pipe()
    pid = os.fork()
    if pid == 0:                              # the child: finalise its copy, report, leave without cleanup
        code = 1
        try:
            g.__del__()
            code = 0 if not destroyed and g._h is None else 2
        finally:
            os.write(w, bytes([code]))
            os._exit(0)
    os.close(w)
    assert os.read(r, 1) == b"\x00"
    os.close(r)
    os.waitpid(pid, 0)
    assert destroyed == [] and g._h                           # the parent's graph is untouched
    g.__del__()
    assert destroyed == [os.getpid()] and g._h is None        # and the parent destroys it, once
    g.__del__()
    del other
    assert destroyed == [os.getpid()] * 2
    made = clg.GraphSim._of_handle(clg.glib(), None, 0)       # what restore and restore_cut wrap their result in
    assert made._pid == os.getpid()
