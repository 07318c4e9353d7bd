"""CPU-only tests of the graph engine's restore (cl_graph_restore, GraphSim.restore): the exported
symbols and the seed info record against include/clgraph.h, and the argument checks that are
answered without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import graphcheck as GC
from snapcheck import ROOT, TEST_DATA

cl, clg = GC.cl, GC.clg


def test_symbols_signatures_and_info_layout():
    L = clg.glib()
    vp, i32 = C.c_void_p, C.c_int32
    assert L.cl_graph_restore.argtypes == [vp, i32, C.POINTER(C.c_void_p)]
    assert L.cl_graph_seed_info_of.argtypes == [vp, vp]
    assert L.cl_graph_restore_time.argtypes == [vp, vp, vp]
    assert L.cl_graph_restore.restype == L.cl_graph_seed_info_of.restype == L.cl_graph_restore_time.restype == C.c_int
    assert clg.SEED_INFO_DTYPE.itemsize == 64            # sizeof(cl_graph_seed_info)
    text = open(os.path.join(ROOT, "include", "clgraph.h")).read()
    body = re.search(r"typedef struct cl_graph_seed_info \{(.*?)\} cl_graph_seed_info;", text, re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"^\s*int64_t\s+([\w, ]+);", body, re.M) for f in decl.split(",")]
    assert fields == list(clg.SEED_INFO_DTYPE.names) == list(clg.SEED_INFO_FIELDS)
    assert [clg.SEED_INFO_DTYPE.fields[f][1] for f in fields] == [8 * i for i in range(8)]
    for name in ("restore", "seed_info", "restore_time"):
        assert hasattr(clg.GraphSim, name)


def small_graph():
    g = clg.GraphSim()
    g.read_topology_file(os.path.join(TEST_DATA, "2nodes.top"))
    g.StartSnapshot("N1")
    g.Tick(1)
    return g


def test_invalid_arguments_are_answered_without_a_device():
    g = small_graph()                        # one snapshot in a program that never ran
    L, h = g._L, g._h
    out = C.c_void_p(0xdead)
    assert L.cl_graph_restore(None, 0, C.byref(out)) == cl.E_INVALID and out.value is None
    assert L.cl_graph_restore(h, 0, None) == cl.E_INVALID
    for sid in (-1, 1, 2**31 - 1):
        out = C.c_void_p(0xdead)
        assert L.cl_graph_restore(h, sid, C.byref(out)) == cl.E_INVALID, sid
        assert out.value is None
    with pytest.raises(cl.ClSnapError) as e:
        g.restore(1)
    assert e.value.code == cl.E_INVALID
    empty = clg.GraphSim()                   # no snapshot at all
    out = C.c_void_p(0xdead)
    assert L.cl_graph_restore(empty._h, 0, C.byref(out)) == cl.E_INVALID and out.value is None


def test_an_ordinary_graph_has_no_seed():
    g = small_graph()
    L, h = g._L, g._h
    info = np.zeros(1, dtype=clg.SEED_INFO_DTYPE)
    a, b = C.c_double(-1), C.c_double(-1)
    assert L.cl_graph_seed_info_of(h, cl._p(info)) == cl.E_STATE
    assert L.cl_graph_restore_time(h, C.byref(a), C.byref(b)) == cl.E_STATE
    assert L.cl_graph_seed_info_of(None, cl._p(info)) == cl.E_INVALID
    assert L.cl_graph_seed_info_of(h, None) == cl.E_INVALID
    assert L.cl_graph_restore_time(h, None, C.byref(b)) == cl.E_INVALID
    assert L.cl_graph_restore_time(None, C.byref(a), C.byref(b)) == cl.E_INVALID
