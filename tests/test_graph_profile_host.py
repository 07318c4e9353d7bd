"""CPU-only tests of the graph engine's node and channel profile over a snapshot range: the
exported symbols, the head words, the spec and the entry layout against include/clgraph.h, the
argument checks and the empty range (answered without a device), the loud failure without a GPU,
the host functions of SnapshotProfile (merge, hottest, the means, by_receiver) on hand-made
objects, and the self-consistency of the expected values (profilecheck) on the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import graphcheck as GC
import profilecheck as PC
import tablecheck as T
from snapcheck import ROOT, TEST_DATA

cl, clg = GC.cl, GC.clg
HEAD = len(clg.PROFILE_HEAD)
PF = PC.PF
I64_MAX, I64_MIN = PC.I64_MAX, PC.I64_MIN


def header():
    return open(os.path.join(ROOT, "include", "clgraph.h")).read()


def test_symbols_and_signatures():
    L = clg.glib()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert L.cl_graph_snapshot_profile.argtypes == [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64]
    assert L.cl_graph_profile_time.argtypes == [vp, vp]
    assert L.cl_graph_set_profile_slices.argtypes == [vp, i32]
    assert L.cl_graph_snapshot_profile.restype == L.cl_graph_profile_time.restype \
        == L.cl_graph_set_profile_slices.restype == C.c_int
    for name in ("snapshot_profile", "profile_time", "set_profile_slices"):
        assert hasattr(clg.GraphSim, name), name
    assert hasattr(clg.PartitionedGraphSim, "snapshot_profile")
    for name in ("word", "mean_tokens", "var_tokens", "mean_latency", "hottest", "by_receiver", "merge"):
        assert hasattr(clg.SnapshotProfile, name), name


def test_head_words_spec_and_entry_mirror_the_header():
    text = header()
    words = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"^#define CL_PF_(\w+) (\d+)", text, re.M)}
    assert words.pop("head") == HEAD == 16
    assert words.pop("node_words") == len(clg.PROFILE_NODE_FIELDS) == 8
    assert words == {f: i for i, f in enumerate(clg.PROFILE_HEAD) if not f.startswith("reserved")}
    assert [i for i, f in enumerate(clg.PROFILE_HEAD) if f.startswith("reserved")] == [13, 14, 15]
    assert int(re.search(r"^#define CL_GRAPH_PROFILE_MAX_BINS (\d+)", text, re.M).group(1)) \
        == clg.PROFILE_MAX_BINS == 1024
    # the node words, in the order of the header's comment
    names = re.search(r"#define CL_PF_NODE_WORDS 8\s*/\*([^*]*)\*/", text).group(1)
    assert [f.strip() for f in names.split(",")] == list(clg.PROFILE_NODE_FIELDS)
    assert clg.PROFILE_NODE_DTYPE.itemsize == 64
    body = re.search(r"typedef struct \{([^}]*)\} cl_graph_profile_spec;", text).group(1)
    fields = [f.strip() for decl in re.findall(r"int32_t\s+([\w, ]+);", body) for f in decl.split(",")]
    assert fields == list(clg.PROFILE_SPEC_DTYPE.names)
    assert clg.PROFILE_SPEC_DTYPE.itemsize == 16
    assert [clg.PROFILE_SPEC_DTYPE.fields[f][1] for f in fields] == [0, 4, 8, 12]
    # the 32-byte entry: four int32, then two int64
    body = re.search(r"typedef struct cl_graph_profile_entry \{(.*?)\} cl_graph_profile_entry;", text, re.S).group(1)
    decl = re.findall(r"^\s*(int32_t|int64_t)\s+(\w+);", body, re.M)
    assert [f for _, f in decl] == list(clg.PROFILE_ENTRY_DTYPE.names)
    dt = clg.PROFILE_ENTRY_DTYPE
    assert dt.itemsize == 32
    offset = 0
    for ctype, f in decl:
        size = 4 if ctype == "int32_t" else 8
        assert dt.fields[f][0].itemsize == size and dt.fields[f][1] == offset, f
        offset += size
    assert offset == 32


def small_graph():
    g = clg.GraphSim()
    g.read_topology_file(os.path.join(TEST_DATA, "2nodes.top"))
    g.StartSnapshot("N1")
    g.Tick(1)
    return g


def spec_of(msg_bins=4, msg_width=1, min_msgs=1, reserved=0):
    s = np.zeros(1, dtype=clg.PROFILE_SPEC_DTYPE)
    s["msg_bins"], s["msg_width"], s["min_msgs"], s["reserved"] = msg_bins, msg_width, min_msgs, reserved
    return s


class Outputs:
    """The outputs of one call at a fill value."""

    def __init__(self, bins=4, ns=1, nodes=2, cap=4):
        self.head = np.full(HEAD + bins, 77, dtype=np.int64)
        self.used = np.full(ns + 1, 77, dtype=np.int32)
        self.rows = np.full(nodes, 77, dtype=clg.PROFILE_NODE_DTYPE)
        self.entries = np.zeros(cap, dtype=clg.PROFILE_ENTRY_DTYPE)
        self.entries.view(np.int64)[:] = 77

    def untouched(self):
        return (self.head == 77).all() and (self.used == 77).all() and (self.rows.view(np.int64) == 77).all() \
            and (self.entries.view(np.int64) == 77).all()


def test_invalid_arguments_are_answered_without_a_device():
    g = small_graph()                        # one snapshot, nothing flushed
    L, h = g._L, g._h
    o = Outputs()
    ok = spec_of()
    p = lambda a: None if a is None else cl._p(a)  # noqa: E731

    def call(hnd=h, lo=0, hi=1, spec=ok, head=o.head, entries=o.entries, cap=4):
        return L.cl_graph_snapshot_profile(hnd, lo, hi, p(spec), None, None, p(head), p(o.used), p(o.rows),
                                           p(entries), cap)

    assert call(hnd=None) == cl.E_INVALID
    assert call(spec=None) == cl.E_INVALID
    assert call(head=None) == cl.E_INVALID
    for bad in (dict(msg_bins=0), dict(msg_bins=-3), dict(msg_bins=clg.PROFILE_MAX_BINS + 1), dict(msg_width=0),
                dict(msg_width=-1), dict(min_msgs=0), dict(min_msgs=-2), dict(reserved=1)):
        assert call(spec=spec_of(**bad)) == cl.E_INVALID, bad
    for lo, hi in ((-1, 1), (1, 0), (0, 2), (2, 2)):
        assert call(lo=lo, hi=hi) == cl.E_INVALID, (lo, hi)
    assert call(cap=-1) == cl.E_INVALID
    assert call(entries=None, cap=1) == cl.E_INVALID
    assert o.untouched()
    assert L.cl_graph_set_profile_slices(None, 1) == cl.E_INVALID
    assert L.cl_graph_set_profile_slices(h, -1) == cl.E_INVALID
    assert L.cl_graph_set_profile_slices(h, 5) == L.cl_graph_set_profile_slices(h, 0) == 0
    t = C.c_double(0)
    assert L.cl_graph_profile_time(h, C.byref(t)) == cl.E_STATE             # nothing has run
    assert L.cl_graph_profile_time(h, None) == cl.E_INVALID
    assert L.cl_graph_profile_time(None, C.byref(t)) == cl.E_INVALID
    # the wrapper checks its own arrays
    with pytest.raises(ValueError):
        g.snapshot_profile(0, 1, use=[1, 0])
    with pytest.raises(ValueError):
        g.snapshot_profile(0, 1, origins=[1, 2, 3])
    with pytest.raises(cl.ClSnapError) as e:
        g.snapshot_profile(0, 1, msg_bins=0)
    assert e.value.code == cl.E_INVALID


def test_empty_range_needs_no_device():
    g = small_graph()
    L, h, p = g._L, g._h, cl._p
    for lo in (0, 1):
        o = Outputs()
        assert L.cl_graph_snapshot_profile(h, lo, lo, p(spec_of()), None, None, p(o.head), p(o.used), p(o.rows),
                                           p(o.entries), 4) == 0
        want = np.zeros(HEAD + 4, dtype=np.int64)
        want[PF["node_hi"]] = o.head[PF["node_hi"]]
        np.testing.assert_array_equal(o.head, want)                          # zeroed but for the node range
        assert 0 == o.head[PF["node_lo"]] <= o.head[PF["node_hi"]] <= 2
        assert (o.used == 77).all() and (o.rows.view(np.int64) == 77).all() and (o.entries.view(np.int64) == 77).all()
        # the sizing form, too
        assert L.cl_graph_snapshot_profile(h, lo, lo, p(spec_of()), None, None, p(o.head), None, None, None, 0) == 0
    pr = g.snapshot_profile(1, 1, msg_bins=8, msg_width=2, min_msgs=3)
    assert len(pr) == 0 and pr.n_used == 0 and pr.spec == (8, 2, 3) and pr.entries.size == 0
    assert pr.hist.tolist() == [0] * 8 and pr.origins is None
    assert all(tuple(r) == PC.NODE_IDENTITY for r in pr.node.tolist())
    assert g.snapshot_profile(1, 1, nodes=False).node is None
    with pytest.raises(cl.ClSnapError) as e:
        g.profile_time()
    assert e.value.code == cl.E_STATE


def test_no_gpu_fails_loudly():
    """Like every other result query: no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    g = small_graph()
    with pytest.raises(cl.ClSnapError) as e:
        g.snapshot_profile()
    assert e.value.code == cl.E_DEVICE


# ---- SnapshotProfile on hand-made objects ----------------------------------------------------
def entries_of(*rows):
    e = np.zeros(len(rows), dtype=clg.PROFILE_ENTRY_DTYPE)
    for i, r in enumerate(rows):
        e[i] = r
    return e


def head_of(**kw):
    h = np.zeros(HEAD, dtype=np.int64)
    for k, v in kw.items():
        h[PF[k]] = v
    return h


def part_a(**kw):
    d = dict(sid_lo=2, used=[1, 0, 1],
             head=head_of(n_sids=3, n_used=2, node_lo=0, node_hi=2, channels=3, active=2, entries=2, msgs=7, tokens=9,
                          max_msgs=5, max_peak=4, max_snaps=2, unit_payloads=0),
             hist=[1, 0, 1, 1],
             # (channel, snaps, peak, peak_sid, msgs, tokens)
             entries=entries_of((0, 1, 2, 4, 2, 3), (5, 2, 4, 2, 5, 6)),
             node=np.array([(20, 202, 9, 11, 6, 4, 2, 3), (8, 32, 4, 4, -2, 0, 5, 6)], dtype=clg.PROFILE_NODE_DTYPE),
             origins=[1, 2, 3], msg_width=2, min_msgs=1)
    d.update(kw)
    return clg.SnapshotProfile(**d)


def part_b(**kw):
    d = dict(sid_lo=2, used=[1, 0, 1],
             head=head_of(n_sids=3, n_used=2, node_lo=2, node_hi=3, channels=2, active=1, entries=1, msgs=5, tokens=5,
                          max_msgs=5, max_peak=5, max_snaps=1, unit_payloads=0),
             hist=[1, 0, 1, 0],
             entries=entries_of((3, 1, 5, 2, 5, 5)),
             node=np.array([(3, 5, 1, 2, 10, 7, 5, 5)], dtype=clg.PROFILE_NODE_DTYPE),
             origins=[1, 2, 3], msg_width=2, min_msgs=1)
    d.update(kw)
    return clg.SnapshotProfile(**d)


def test_profile_accessors():
    a = part_a()
    assert len(a) == 3 and a.n_used == 2 and (a.node_lo, a.node_hi) == (0, 2) and a.spec == (4, 2, 1)
    assert a.word("msgs") == 7 and a.word("max_peak") == 4 and a.used.dtype == np.int32
    assert a.mean_tokens().tolist() == [10.0, 4.0]
    assert a.var_tokens().tolist() == [1.0, 0.0]
    assert a.mean_latency().tolist() == [3.0, -1.0]
    none = part_a(used=[0, 0, 0], head=head_of(n_sids=3, node_hi=2))
    assert np.isnan(none.mean_tokens()).all() and np.isnan(none.var_tokens()).all() \
        and np.isnan(none.mean_latency()).all()
    with pytest.raises(ValueError):
        part_a(node=None).mean_latency()
    assert a == part_a() and a != part_b() and a != part_a(node=None) and a != part_a(origins=None)
    assert a != part_a(msg_width=1) and a != part_a(hist=[1, 0, 2, 0]) and a != "x"
    with pytest.raises(ValueError):
        clg.SnapshotProfile(0, [1], np.zeros(HEAD - 1), [0], entries_of())
    # by receiver: channels 0 and 5 go to nodes 1 and 0
    dst = np.array([1, 0, 0, 2, 2, 0])
    got = a.by_receiver(dst)
    assert got["node"].tolist() == [0, 1] and got["channels"].tolist() == [1, 1]
    assert got["msgs"].tolist() == [5, 2] and got["tokens"].tolist() == [6, 3]


def test_profile_hottest():
    e = entries_of((1, 1, 1, 0, 4, 4), (2, 1, 1, 0, 9, 9), (6, 1, 1, 0, 4, 5), (7, 1, 1, 0, 1, 1), (9, 2, 3, 1, 9, 9))
    pr = part_a(entries=e)
    assert pr.hottest(3)["channel"].tolist() == [2, 9, 1]                  # ties by the lower channel
    assert pr.hottest(4)["channel"].tolist() == [2, 9, 1, 6]
    assert pr.hottest(99)["channel"].tolist() == [2, 9, 1, 6, 7] and pr.hottest(0).size == 0
    assert pr.hottest(1).dtype == clg.PROFILE_ENTRY_DTYPE and pr.hottest(1)["msgs"].tolist() == [9]


def test_profile_merge():
    a, b = part_a(), part_b()
    m = clg.SnapshotProfile.merge([a, b])
    want = clg.SnapshotProfile(
        2, [1, 0, 1],
        head_of(n_sids=3, n_used=2, node_lo=0, node_hi=3, channels=5, active=3, entries=3, msgs=12, tokens=14,
                max_msgs=5, max_peak=5, max_snaps=2, unit_payloads=0),
        [2, 0, 2, 1], entries_of((0, 1, 2, 4, 2, 3), (3, 1, 5, 2, 5, 5), (5, 2, 4, 2, 5, 6)),
        np.concatenate([a.node, b.node]), [1, 2, 3], 2, 1)
    assert m == want
    np.testing.assert_array_equal(m.head, want.head)
    assert clg.SnapshotProfile.merge([a]) == a
    # without node rows on one part there are none
    assert clg.SnapshotProfile.merge([a, part_b(node=None)]).node is None


def test_profile_merge_refuses_what_does_not_belong_together():
    a = part_a()
    merge = clg.SnapshotProfile.merge
    with pytest.raises(ValueError):
        merge([])
    with pytest.raises(ValueError):
        merge([a, part_b(sid_lo=3)])                                          # other range
    with pytest.raises(ValueError):
        merge([a, part_b(used=[1, 0, 1, 1], origins=[1, 2, 3, 4])])           # other length
    with pytest.raises(ValueError):
        merge([a, part_b(msg_width=1)])                                       # other spec
    with pytest.raises(ValueError):
        merge([a, part_b(min_msgs=2)])
    with pytest.raises(ValueError):
        merge([a, part_b(hist=[1, 0, 1])])                                    # other bins
    with pytest.raises(ValueError):
        merge([a, part_b(used=[1, 1, 1])])                                    # other used rows
    with pytest.raises(ValueError):
        merge([a, part_b(origins=[1, 2, 4])])                                 # other origins
    with pytest.raises(ValueError):
        merge([a, part_b(origins=None)])
    with pytest.raises(ValueError):
        merge([part_b(), a])                                                  # not in rank order
    with pytest.raises(ValueError):
        merge([a, part_b(head=head_of(n_sids=3, n_used=2, node_lo=3, node_hi=4))])    # a gap between the node ranges


# ---- the expected values on the oracle alone -------------------------------------------------
def test_expected_values_are_self_consistent():
    p, o, table = T.powerlaw_drained()
    ns, n = o.num_snapshots, p.n
    assert ns == 12 and np.array_equal(np.lexsort((p.dst, p.src)), np.arange(p.src.size))     # channel order
    for use in (None, np.arange(ns) % 2 == 0):
        rows = np.ones(ns, dtype=bool) if use is None else use
        x = PC.expected_profile(o, 0, ns, use=use, dst=p.dst)
        assert x.n_used == rows.sum() and x.word("channels") == p.src.size == x.hist.sum()
        assert x.entries["msgs"].sum() == x.word("msgs") == table["rec_msgs"][rows].sum()
        assert x.node["in_msgs"].sum() == x.word("msgs") and x.node["in_tokens"].sum() == x.word("tokens")
        assert x.node["tok_sum"].sum() == table["node_tokens"][rows].sum()
        assert x.word("active") == x.word("entries") == x.entries.size
        assert x.word("max_peak") == table["max_ch_msgs"][rows].max()
        assert (x.entries["peak_sid"] >= 0).all() and rows[x.entries["peak_sid"]].all()
        np.testing.assert_array_equal(x.by_receiver(p.dst)["msgs"], x.node["in_msgs"])
        # a two-way node split merges to the whole
        cut = 1024
        parts = [PC.expected_profile(o, 0, ns, use=use, dst=p.dst, node_lo=lo, node_hi=hi)
                 for lo, hi in ((0, cut), (cut, n))]
        assert parts[0].entries.size > 0 and parts[1].entries.size > 0
        PC.assert_profile_equal(clg.SnapshotProfile.merge(parts), x)
    # min_msgs bounds the entries by the histogram's tail
    for m in (2, 3):
        y = PC.expected_profile(o, 0, ns, min_msgs=m, dst=p.dst)
        assert y.entries.size == y.word("entries") == y.hist[m:].sum() and (y.entries["msgs"] >= m).all()
