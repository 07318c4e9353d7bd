"""Host side of the instance sets (cl_iset, InstanceSet) and of the conditional calls: the entry
points and their signatures, and every argument check that is made before any device work.  No GPU:
each check here must hold on a machine without a device."""
import ctypes as C
import importlib

import numpy as np
import pytest

from snapcheck import read_text

PKG = "chandy-lamport-distributed-snapshot-algorithm_amd"
cl = importlib.import_module(PKG)

VP, I64, I32, PP = C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)
SIGNATURES = {
    "cl_iset_from_clauses": [VP, I32, I64, I64, VP, I32, PP, VP],
    "cl_iset_from_list": [VP, VP, I64, PP],
    "cl_iset_combine": [VP, VP, VP, I32],
    "cl_iset_count": [VP, I64, I64, VP],
    "cl_iset_read": [VP, I64, I64, VP, I64, VP],
    "cl_iset_destroy": [VP],
    "cl_iset_time": [VP, VP],
    "cl_snapshot_stats_in": [VP, I32, I64, I64, VP, VP, VP, I64],
    "cl_snapshot_census_in": [VP, I32, I64, I64, VP, VP, VP, VP, VP],
    "cl_select_instances_in": [VP, I32, I64, I64, VP, VP, I32, VP, VP, I64, VP],
}
TICK = 0


def _sim(n=8, top="3nodes.top"):
    sim = cl.ChandyLamportSim(n)
    sim.read_topology_text(read_text(top))
    return sim


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _from_list(sim, insts, n=None):
    """(return code, handle) of cl_iset_from_list."""
    arr = None if insts is None else np.asarray(insts, dtype=np.int64)
    h = C.c_void_p()
    rc = cl.lib().cl_iset_from_list(sim._h, _p(arr), (0 if arr is None else arr.size) if n is None else n, C.byref(h))
    return rc, h


def _from_clauses(sim, sid, lo, hi, clauses, n_clauses, info, out=True):
    arr = None if clauses is None else np.array(clauses, dtype=cl.SELECT_CLAUSE_DTYPE)
    h = C.c_void_p()
    rc = cl.lib().cl_iset_from_clauses(sim._h, sid, lo, hi, _p(arr), n_clauses, C.byref(h) if out else None, _p(info))
    return rc, h


def test_entry_points_and_signatures():
    L = cl.lib()
    for name, args in SIGNATURES.items():
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == args, name
    assert "InstanceSet" in cl.__all__
    assert (cl.ISET_AND, cl.ISET_OR, cl.ISET_ANDNOT) == (0, 1, 2)
    for name in ("instance_set", "instance_set_from", "snapshot_stats_in", "snapshot_census_in",
                 "select_instances_in", "iset_time"):
        assert callable(getattr(cl.ChandyLamportSim, name)), name
    for name in ("count", "insts", "close", "__and__", "__or__", "__sub__", "__len__", "__enter__", "__exit__"):
        assert callable(getattr(cl.InstanceSet, name)), name


def test_argument_errors_need_no_device():
    L = cl.lib()
    sim, other = _sim(8), _sim(8)
    good = [(TICK, 0, 0, 0, 0, 100)]
    info = np.full(5, 7, dtype=np.int64)
    # nothing has run: no event was ever issued
    assert _from_clauses(sim, 0, 0, 8, good, 1, info)[0] == cl.E_STATE
    assert _from_clauses(sim, 0, 0, 8, None, 0, info)[0] == cl.E_STATE
    with pytest.raises(cl.ClSnapError) as e:
        sim.instance_set(0)
    assert e.value.code == cl.E_STATE
    with pytest.raises(cl.ClSnapError) as e:
        sim.iset_time()
    assert e.value.code == cl.E_STATE

    # ---- lists: checked before any device work; a set made before anything ran keeps its list
    for insts in ([8], [-1], [0, 1, 2, 8], [3, -5, 3], [2**40]):
        rc, h = _from_list(sim, insts)
        assert rc == cl.E_INVALID and not h.value, insts
    assert _from_list(sim, None, n=3)[0] == cl.E_INVALID            # NULL list with n > 0
    assert _from_list(sim, [1, 2], n=-1)[0] == cl.E_INVALID         # n < 0
    assert L.cl_iset_from_list(sim._h, None, 0, None) == cl.E_INVALID   # NULL output
    rc, a = _from_list(sim, [0, 3, 3, 7])                            # duplicates are allowed
    assert rc == 0 and a.value
    rc, empty = _from_list(sim, None)                                # n == 0: the empty set
    assert rc == 0 and empty.value
    rc, b = _from_list(other, [1])
    assert rc == 0 and b.value

    # ---- combine: NULL sets, an unknown op, sets of two sims
    for dst, x, y in ((None, a, a), (a, None, a), (a, a, None)):
        assert L.cl_iset_combine(dst, x, y, cl.ISET_AND) == cl.E_INVALID
    for op in (-1, 3, 100):
        assert L.cl_iset_combine(empty, a, a, op) == cl.E_INVALID, op
    for dst, x, y in ((empty, a, b), (empty, b, a), (b, a, empty), (b, a, a)):
        assert L.cl_iset_combine(dst, x, y, cl.ISET_OR) == cl.E_INVALID

    # ---- count and read: NULL set, NULL output, the range, cap
    n, out = C.c_int64(7), np.full(8, 7, dtype=np.int64)
    assert L.cl_iset_count(None, 0, 8, C.byref(n)) == cl.E_INVALID
    assert L.cl_iset_count(a, 0, 8, None) == cl.E_INVALID
    assert L.cl_iset_read(None, 0, 8, _p(out), 8, C.byref(n)) == cl.E_INVALID
    assert L.cl_iset_read(a, 0, 8, _p(out), 8, None) == cl.E_INVALID
    assert L.cl_iset_read(a, 0, 8, _p(out), -1, C.byref(n)) == cl.E_INVALID
    assert L.cl_iset_read(a, 0, 8, None, 8, C.byref(n)) == cl.E_INVALID
    for lo, hi in ((-1, 8), (0, 9), (5, 4)):
        assert L.cl_iset_count(a, lo, hi, C.byref(n)) == cl.E_INVALID
        assert L.cl_iset_read(a, lo, hi, _p(out), 8, C.byref(n)) == cl.E_INVALID
    assert n.value == 7 and (out == 7).all()

    # ---- the conditional calls: a NULL set and a set of another sim, before and after events
    spec = np.array([0, 16, 4], dtype=np.int32)
    raw = np.full(sim.stats_layout(0, 16, 4)["total_words"], 7, dtype=np.int64)
    cspec = cl._CensusSpec(4, 0)
    classes = np.zeros(4, dtype=cl.CENSUS_CLASS_DTYPE)
    cinfo = np.full(5, 7, dtype=np.int64)
    insts = np.full(8, 7, dtype=np.int64)

    def conditional(iset):
        return (L.cl_snapshot_stats_in(sim._h, 0, 0, 8, iset, _p(spec), _p(raw), raw.size),
                L.cl_snapshot_census_in(sim._h, 0, 0, 8, iset, C.byref(cspec), _p(classes), None, _p(cinfo)),
                L.cl_select_instances_in(sim._h, 0, 0, 8, iset, None, 0, _p(insts), None, 8, _p(info)))

    assert conditional(None) == (cl.E_INVALID,) * 3
    assert conditional(b) == (cl.E_INVALID,) * 3
    assert conditional(a) == (cl.E_STATE,) * 3                       # this sim's set: the state check is next
    sim.ProcessEvent(cl.PassTokenEvent("N1", "N2", 1))
    assert sim.StartSnapshot("N1") == 0
    sim.Tick(2)
    assert conditional(None) == (cl.E_INVALID,) * 3
    assert conditional(b) == (cl.E_INVALID,) * 3
    # the other checks are those of the unconditional calls
    assert L.cl_snapshot_stats_in(sim._h, 1, 0, 8, a, _p(spec), _p(raw), raw.size) == cl.E_INVALID
    assert L.cl_snapshot_stats_in(sim._h, 0, 0, 9, a, _p(spec), _p(raw), raw.size) == cl.E_INVALID
    assert L.cl_snapshot_stats_in(sim._h, 0, 0, 8, a, _p(spec), _p(raw), 3) == cl.E_LIMIT
    assert L.cl_snapshot_stats_in(sim._h, 0, 0, 8, a, None, _p(raw), raw.size) == cl.E_INVALID
    assert L.cl_snapshot_census_in(sim._h, 0, 5, 4, a, C.byref(cspec), _p(classes), None, _p(cinfo)) == cl.E_INVALID
    assert L.cl_snapshot_census_in(sim._h, 0, 0, 8, a, C.byref(cspec), None, None, _p(cinfo)) == cl.E_INVALID
    assert L.cl_select_instances_in(sim._h, 0, 0, 8, a, None, 1, _p(insts), None, 8, _p(info)) == cl.E_INVALID
    assert L.cl_select_instances_in(sim._h, 0, 0, 8, a, None, 0, None, None, 8, _p(info)) == cl.E_INVALID
    assert L.cl_select_instances_in(sim._h, 0, 0, 8, a, None, 0, _p(insts), None, 8, None) == cl.E_INVALID
    # from_clauses makes the checks of cl_select_instances
    assert _from_clauses(sim, 0, 0, 8, good, 1, None)[0] == cl.E_INVALID          # NULL info
    assert _from_clauses(sim, 0, 0, 8, good, 1, info, out=False)[0] == cl.E_INVALID  # NULL output
    assert _from_clauses(sim, 0, 0, 8, None, 1, info)[0] == cl.E_INVALID
    assert _from_clauses(sim, 0, 0, 8, good * 9, 9, info)[0] == cl.E_INVALID
    assert _from_clauses(sim, 0, 0, 8, [(7, 0, 0, 0, 0, 1)], 1, info)[0] == cl.E_INVALID
    assert _from_clauses(sim, 0, 0, 8, [(3, 99, 0, 0, 0, 1)], 1, info)[0] == cl.E_INVALID
    assert _from_clauses(sim, 1, 0, 8, good, 1, info)[0] == cl.E_INVALID
    assert _from_clauses(sim, 0, 0, 9, good, 1, info)[0] == cl.E_INVALID
    # nothing was written
    assert (raw == 7).all() and (cinfo == 7).all() and (insts == 7).all() and (info == 7).all()

    # ---- destroy: NULL is a no-op; a set goes once, the sims free the rest
    assert L.cl_iset_destroy(None) == 0
    assert L.cl_iset_destroy(empty) == 0
    assert L.cl_iset_destroy(b) == 0


def test_python_layer_without_a_device():
    sim = _sim(8)
    for insts in ([8], [-1], [0, 99]):
        with pytest.raises(cl.ClSnapError) as e:
            sim.instance_set_from(insts)
        assert e.value.code == cl.E_INVALID
    a = sim.instance_set_from(np.array([5, 1, 1], dtype=np.int32))     # any integer dtype
    assert isinstance(a, cl.InstanceSet) and a.info is None
    with pytest.raises(TypeError):
        a & 3
    with pytest.raises(cl.ClSnapError) as e:
        sim.snapshot_stats_in(0, a)                                    # no event was ever issued
    assert e.value.code == cl.E_STATE
    a.close()
    a.close()                                                          # closing twice is harmless
    for use in (lambda: a.count(), lambda: a.insts(), lambda: sim.snapshot_stats_in(0, a), lambda: a | a):
        with pytest.raises(ValueError):
            use()
    with sim.instance_set_from([2]) as b:
        assert b._h
    assert b._h is None
    # a sim destroyed with sets alive frees them; closing such a set afterwards touches nothing
    c, d = sim.instance_set_from([0, 7]), sim.instance_set_from(())
    sim.__del__()
    assert sim._h is None
    c.close()
    with pytest.raises(ValueError):
        d.count()
    del d
