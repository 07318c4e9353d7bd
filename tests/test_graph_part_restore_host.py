"""CPU-only tests of the partitioned run that begins in a restored cut
(cl_graph_part_begin_seeded, cl_graph_part_seed_share, PartitionedGraphSim.from_cut): the exported
symbols against include/clgraph.h, the errors answered before any device work, the numpy
statement of a rank's share (partrestorecheck) against a walk over the entries on small random
cuts, and from_cut's own argument check.  Everything that seeds is in the GPU file."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import graphcheck as GC
import graphgen as G
import partrestorecheck as PR
from snapcheck import ROOT, TEST_DATA

cl, clg = GC.cl, GC.clg


def template():
    """The 2-node topology, never run: an ordinary graph, not a restored one."""
    g = clg.GraphSim()
    g.read_topology_file(os.path.join(TEST_DATA, "2nodes.top"))
    return g


def test_symbols_and_signatures():
    L = clg.glib()
    assert L.cl_graph_part_begin_seeded.argtypes == [C.c_void_p, C.c_int32, C.c_int32]
    assert L.cl_graph_part_seed_share.argtypes == [C.c_void_p, C.c_void_p]
    assert L.cl_graph_part_begin_seeded.restype == L.cl_graph_part_seed_share.restype == C.c_int
    text = open(os.path.join(ROOT, "include", "clgraph.h")).read()
    assert re.search(r"^int cl_graph_part_begin_seeded\(cl_graph\* r, int32_t node_lo, int32_t node_hi\);", text, re.M)
    assert re.search(r"^int cl_graph_part_seed_share\(cl_graph\* r, int64_t out\[4\]\);", text, re.M)
    for name in ("cut", "from_cut", "restore"):
        assert hasattr(clg.PartitionedGraphSim, name)


def test_null_handles():
    L = clg.glib()
    out = np.zeros(4, dtype=np.int64)
    assert L.cl_graph_part_begin_seeded(None, 0, 0) == cl.E_INVALID
    assert L.cl_graph_part_seed_share(None, out.ctypes.data) == cl.E_INVALID
    assert L.cl_graph_part_seed_share(template()._h, None) == cl.E_INVALID


def test_an_ordinary_graph_is_refused_without_a_device():
    g = template()
    L = g._L
    out = np.full(4, -7, dtype=np.int64)
    assert L.cl_graph_part_begin_seeded(g._h, 0, g.num_nodes) == cl.E_STATE
    assert b"restored" in L.cl_last_error()
    assert L.cl_graph_part_begin_seeded(g._h, 1, 1) == cl.E_STATE          # (the state comes before the range)
    assert L.cl_graph_part_seed_share(g._h, out.ctypes.data) == cl.E_STATE
    assert (out == -7).all()
    assert g.device_bytes == 0                                               # nothing reached a device
    empty = clg.GraphSim()
    assert L.cl_graph_part_begin_seeded(empty._h, 0, 0) == cl.E_STATE


@pytest.mark.parametrize("seed", range(6))
def test_the_share_statement_against_a_walk(seed):
    """Random cuts on a random regular graph of 5 x 256 nodes, every split into 1..5 ranks, and the
    ranges that are no rank's: empty ones, the whole graph, single blocks."""
    rng = np.random.default_rng(seed)
    n = 1280
    src, dst = G.regular_graph(n, 3, 40 + seed)
    order = np.lexsort((dst, src))
    src = np.asarray(src)[order]
    e = src.size
    off = PR.out_offsets(n, src)
    assert off[-1] == e and (np.diff(src) >= 0).all()
    density = (0.0, 0.002, 0.05, 0.5, 0.9, 1.0)[seed]
    channel = np.nonzero(rng.random(e) < density)[0]
    if seed == 2:                                       # entries right at the bounds of the middle block
        channel = np.union1d(channel, [off[512] - 1, off[512], off[768] - 1, off[768], 0, e - 1])
    count = rng.integers(1, 9, size=channel.size)
    ranges = [(0, 0), (n, n), (0, n), (256, 256), (256, 512), (512, 768), (1024, n)]
    for world in range(1, 6):
        sp = PR.spans(n, world)
        ranges += sp
        PR.assert_shares_tile([PR.share(channel, count, off, lo, hi) for lo, hi in sp if lo < hi], channel.size,
                              int(count.sum()))
    for lo, hi in ranges:
        assert PR.share(channel, count, off, lo, hi) == PR.brute_share(channel.tolist(), count.tolist(), src, lo, hi)


def test_spans_are_the_partition_s():
    assert PR.spans(2000, 3) == [(0, 768), (768, 1536), (1536, 2000)]
    assert PR.spans(2000, 2) == [(0, 1024), (1024, 2000)]
    assert PR.spans(4096, 2) == [(0, 2048), (2048, 4096)]


def test_from_cut_needs_a_template_or_a_topology():
    cut = clg.SnapshotCut(0, [1, 0], [0], [2], [1, 1], n_channels=2, topology_key=1)
    assert not cut.has_topology
    with pytest.raises(ValueError):
        clg.PartitionedGraphSim.from_cut(cut, 0, 2)
    with pytest.raises(ValueError):
        clg.PartitionedGraphSim.from_cut(cut, 0, 2, template=None, fifo_slots=64)
