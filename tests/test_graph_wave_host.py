"""CPU-only tests of the graph engine's marker-wave profile and marker tree: the exported
symbols, the head words and the spec against include/clgraph.h, the argument checks and the
empty range (answered without a device), the loud failure without a GPU, and the host functions
of SnapshotWave (merge, coverage, means) and MarkerTree (depth, path) on hand-made objects."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import graphcheck as GC
import wavecheck as WC
from snapcheck import ROOT, TEST_DATA

cl, clg = GC.cl, GC.clg
HEAD = len(clg.WAVE_HEAD)
I64_MAX, I64_MIN = WC.I64_MAX, WC.I64_MIN


def header():
    return open(os.path.join(ROOT, "include", "clgraph.h")).read()


def test_symbols_and_signatures():
    L = clg.glib()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert L.cl_graph_snapshot_wave.argtypes == [vp, i32, i32, vp, vp, vp, i64]
    assert L.cl_graph_wave_time.argtypes == [vp, vp, vp]
    assert L.cl_graph_snapshot_tree.argtypes == [vp, i32, i32, vp, vp]
    assert L.cl_graph_snapshot_wave.restype == L.cl_graph_wave_time.restype == L.cl_graph_snapshot_tree.restype \
        == C.c_int
    for name in ("snapshot_wave", "snapshot_tree", "wave_time"):
        assert hasattr(clg.GraphSim, name), name
    for name in ("snapshot_wave", "snapshot_tree"):
        assert hasattr(clg.PartitionedGraphSim, name), name


def test_head_words_and_spec_mirror_the_header():
    text = header()
    words = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"^#define CL_WV_(\w+) (\d+)", text, re.M)}
    assert words.pop("head") == HEAD == 12
    assert words == {f: i for i, f in enumerate(clg.WAVE_HEAD) if f != "reserved"}
    assert clg.WAVE_HEAD.index("reserved") == HEAD - 1
    assert int(re.search(r"^#define CL_GRAPH_WAVE_MAX_BINS (\d+)", text, re.M).group(1)) == clg.WAVE_MAX_BINS == 1024
    body = re.search(r"typedef struct \{([^}]*)\} cl_graph_wave_spec;", text).group(1)
    fields = [f.strip() for decl in re.findall(r"int32_t\s+([\w, ]+);", body) for f in decl.split(",")]
    assert fields == list(clg.WAVE_SPEC_DTYPE.names)
    assert clg.WAVE_SPEC_DTYPE.itemsize == 16
    assert [clg.WAVE_SPEC_DTYPE.fields[f][1] for f in fields] == [0, 4, 8, 12]


def small_graph():
    g = clg.GraphSim()
    g.read_topology_file(os.path.join(TEST_DATA, "2nodes.top"))
    g.StartSnapshot("N1")
    g.Tick(1)
    return g


def spec_of(lat_bins=4, lat_width=1, depth_bins=2, reserved=0):
    s = np.zeros(1, dtype=clg.WAVE_SPEC_DTYPE)
    s["lat_bins"], s["lat_width"], s["depth_bins"], s["reserved"] = lat_bins, lat_width, depth_bins, reserved
    return s


def test_invalid_arguments_are_answered_without_a_device():
    g = small_graph()                        # one snapshot, nothing flushed
    L, h, p = g._L, g._h, cl._p
    out = np.full(64, 77, dtype=np.int64)
    ok = spec_of()
    wave = lambda hnd, lo, hi, spec, o, words: L.cl_graph_snapshot_wave(  # noqa: E731
        hnd, lo, hi, None if spec is None else p(spec), None, None if o is None else p(o), words)
    assert wave(None, 0, 1, ok, out, 64) == cl.E_INVALID
    assert wave(h, 0, 1, None, out, 64) == cl.E_INVALID
    assert wave(h, 0, 1, ok, None, 64) == cl.E_INVALID
    for bad in (dict(lat_bins=0), dict(lat_bins=-3), dict(lat_bins=clg.WAVE_MAX_BINS + 1), dict(lat_width=0),
                dict(lat_width=-1), dict(depth_bins=-1), dict(depth_bins=clg.WAVE_MAX_BINS + 1), dict(reserved=1)):
        assert wave(h, 0, 1, spec_of(**bad), out, 1 << 20) == cl.E_INVALID, bad
    for lo, hi in ((-1, 1), (1, 0), (0, 2), (2, 2)):
        assert wave(h, lo, hi, ok, out, 64) == cl.E_INVALID, (lo, hi)
    # one row of 12 + 4 + 2 words
    assert wave(h, 0, 1, ok, out, HEAD + 5) == cl.E_LIMIT
    assert wave(h, 0, 1, ok, out, 0) == cl.E_LIMIT
    assert wave(h, 0, 1, spec_of(clg.WAVE_MAX_BINS, 1, clg.WAVE_MAX_BINS), out, HEAD + 2 * clg.WAVE_MAX_BINS - 1) \
        == cl.E_LIMIT
    # the tree call's checks
    a = np.full(4, 77, dtype=np.int32)
    assert L.cl_graph_snapshot_tree(None, 0, 1, p(a), None) == cl.E_INVALID
    assert L.cl_graph_snapshot_tree(h, 0, 1, None, p(a)) == cl.E_INVALID
    for lo, hi in ((-1, 1), (1, 0), (0, 2), (2, 2)):
        assert L.cl_graph_snapshot_tree(h, lo, hi, p(a), None) == cl.E_INVALID, (lo, hi)
    assert (out == 77).all() and (a == 77).all()           # nothing was written
    t, r = C.c_double(0), C.c_int32(0)
    assert L.cl_graph_wave_time(h, C.byref(t), C.byref(r)) == cl.E_STATE     # nothing has run
    assert L.cl_graph_wave_time(h, C.byref(t), None) == cl.E_STATE
    assert L.cl_graph_wave_time(h, None, None) == cl.E_INVALID
    assert L.cl_graph_wave_time(None, C.byref(t), None) == cl.E_INVALID


def test_empty_range_needs_no_device():
    g = small_graph()
    L, h, p = g._L, g._h, cl._p
    out = np.full(8, 77, dtype=np.int64)
    for lo in (0, 1):
        assert L.cl_graph_snapshot_wave(h, lo, lo, p(spec_of()), None, p(out), 0) == 0
        assert L.cl_graph_snapshot_tree(h, lo, lo, p(out), None) == 0
    assert (out == 77).all()
    w = g.snapshot_wave(1, 1, lat_bins=8, lat_width=2, depth_bins=4)
    assert len(w) == 0 and w.rows.shape == (0, HEAD + 12) and w.spec == (8, 2, 4)
    assert g.snapshot_tree(1, 1) == []
    with pytest.raises(cl.ClSnapError) as e:
        g.wave_time()
    assert e.value.code == cl.E_STATE


def test_no_gpu_fails_loudly():
    """Like every other result query: no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    g = small_graph()
    for call in (g.snapshot_wave, g.snapshot_tree):
        with pytest.raises(cl.ClSnapError) as e:
            call()
        assert e.value.code == cl.E_DEVICE


# ---- SnapshotWave on hand-made rows ----------------------------------------------------------
def wave(*rows, spec=(4, 2, 3)):
    out = np.zeros((len(rows), HEAD + spec[0] + spec[2]), dtype=np.int64)
    for r, d in zip(out, rows):
        for k, v in d.items():
            if k == "lat_hist":
                r[HEAD:HEAD + spec[0]] = v
            elif k == "depth_hist":
                r[HEAD + spec[0]:] = v
            else:
                r[WC.W[k]] = v
    return clg.SnapshotWave(out, *spec)


A = dict(sid=3, origin=5, created=4, lat_sum=10, lat_sumsq=40, lat_min=0, lat_max=6, depth_sum=5, depth_sumsq=9,
         depth_max=2, broken=0, lat_hist=[2, 1, 0, 1], depth_hist=[1, 1, 2])
B = dict(sid=3, origin=5, created=2, lat_sum=9, lat_sumsq=41, lat_min=4, lat_max=5, depth_sum=7, depth_sumsq=25,
         depth_max=4, broken=1, lat_hist=[0, 0, 2, 0], depth_hist=[0, 0, 1])
EMPTY = dict(sid=3, origin=5, lat_min=I64_MAX, lat_max=I64_MIN, depth_max=-1)


def test_wave_accessors():
    w = wave(A, dict(EMPTY, sid=4))
    assert len(w) == 2 and w.row_words == HEAD + 7
    assert w.sid.tolist() == [3, 4] and w.origin.tolist() == [5, 5] and w.created.tolist() == [4, 0]
    assert w.lat_hist.tolist() == [[2, 1, 0, 1], [0, 0, 0, 0]] and w.depth_hist.tolist() == [[1, 1, 2], [0, 0, 0]]
    assert w.mean_latency[0] == 2.5 and np.isnan(w.mean_latency[1])
    assert w.mean_depth[0] == 1.25 and np.isnan(w.mean_depth[1])
    assert w.coverage().tolist() == [[0.5, 0.75, 0.75, 1.0], [0.0, 0.0, 0.0, 0.0]]
    assert w.word("lat_max").tolist() == [6, I64_MIN]


def test_wave_merge():
    a, b = wave(A), wave(B)
    want = wave(dict(sid=3, origin=5, created=6, lat_sum=19, lat_sumsq=81, lat_min=0, lat_max=6, depth_sum=12,
                     depth_sumsq=34, depth_max=4, broken=1, lat_hist=[2, 1, 2, 1], depth_hist=[1, 1, 3]))
    assert a.merge(b) == b.merge(a) == want
    np.testing.assert_array_equal(a.merge(b).rows, want.rows)
    assert a.merge(b) != a
    # a part that created no node leaves the extremes to the other
    assert wave(EMPTY).merge(b) == b and b.merge(wave(EMPTY)) == b
    # the squares add modulo 2^64
    big = wave(dict(A, lat_sumsq=I64_MAX)).merge(wave(dict(B, lat_sumsq=1)))
    assert big.word("lat_sumsq")[0] == I64_MIN


def test_wave_merge_refuses_what_does_not_belong_together():
    a = wave(A, dict(A, sid=4))
    with pytest.raises(ValueError):
        a.merge(wave(dict(B, sid=4), B))                      # other order
    with pytest.raises(ValueError):
        a.merge(wave(B))                                      # other range
    with pytest.raises(ValueError):
        wave(A).merge(wave(dict(B, origin=6)))                # other origin
    with pytest.raises(ValueError):
        wave(A).merge(clg.SnapshotWave(wave(B).rows, 2, 2, 5))    # other spec, the same row width
    with pytest.raises(ValueError):
        wave(A).merge(wave(B, spec=(4, 1, 3)))                # other bin width


# ---- MarkerTree on hand-made trees -----------------------------------------------------------
def test_tree_depth_and_path_on_a_chain():
    n = 1000                                 # 3 <- 4 <- ... <- 999 <- 0 <- 1 <- 2: one chain from rank 3
    parent = (np.arange(n) - 1) % n
    parent[3] = -1
    t = clg.MarkerTree(parent, (np.arange(n) - 3) % n + 7)
    d = t.depth()
    assert d.dtype == np.int64 and d.tolist() == ((np.arange(n) - 3) % n).tolist()
    assert t.path(3) == [3] and t.path(5) == [5, 4, 3]
    assert t.path(2) == [2, 1, 0] + list(range(999, 2, -1))
    assert t.created.all() and len(t) == n


def test_tree_with_holes_and_branches():
    #        0
    #      /   \
    #     2     5        1, 6: no local snapshot; 7 hangs below 6 (never in a run: its chain
    #    / \    |        does not reach the initiator)
    #   3   4   8
    parent = np.array([-1, -2, 0, 2, 2, 0, -2, 6, 5])
    t = clg.MarkerTree(parent)
    assert t.depth().tolist() == [0, -1, 1, 2, 2, 1, -1, -1, 2]
    assert t.created.tolist() == [True, False, True, True, True, True, False, True, True]
    assert t.path(8) == [8, 5, 0] and t.path(0) == [0]
    for v in (1, 7):
        with pytest.raises(ValueError):
            t.path(v)
    with pytest.raises(IndexError):
        t.path(9)
    assert t.tick is None and t == clg.MarkerTree(parent) and t != clg.MarkerTree(parent, np.zeros(9))


def test_tree_refuses_cycles_parts_and_foreign_parents():
    with pytest.raises(ValueError):
        clg.MarkerTree([1, 2, 0, -1]).depth()
    with pytest.raises(ValueError):
        clg.MarkerTree([1, 2, 0, -1]).path(0)
    with pytest.raises(ValueError):
        clg.MarkerTree([-1, 0, 4]).depth()                    # a parent outside the nodes
    with pytest.raises(ValueError):
        clg.MarkerTree([-1, 0], node_lo=256).depth()          # a part of a partitioned run
    with pytest.raises(ValueError):
        clg.MarkerTree([-1, 0], [1, 2, 3])


def test_expected_values_are_self_consistent():
    """On the oracle alone: the helper's ring is the chain the GPU test relies on, and its rows
    agree with MarkerTree.depth and the table."""
    p, o, x = WC.ring_drained()
    assert o.status == 0 and o.time == 1840 and x.origin.tolist() == [1]
    assert x.depth[0].max() == 599 and sorted(x.depth[0].tolist()) == list(range(600))
    assert (x.tick[0] - x.origin[0]).max() == 1829
    tree = x.trees()[0]
    np.testing.assert_array_equal(tree.depth(), x.depth[0])
    assert tree.path(199) == [(199 - i) % 600 for i in range(600)]
    rows = x.rows(64, 32, 1024)
    w = clg.SnapshotWave(rows, 64, 32, 1024)
    assert w.created.tolist() == [600] and w.depth_hist[0, :600].tolist() == [1] * 600
    assert w.lat_hist.sum() == 600 and w.coverage()[0, -1] == 1.0
