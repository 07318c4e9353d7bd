"""Host side of the snapshot crosstab: the header's words and axis struct, argument checks, axis
normalisation, SnapshotCrosstab arithmetic and the multi-rank reduce.  No GPU: every check here
must hold on a machine without a device."""
import ctypes as C
import importlib
import os
import re
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from snapcheck import ROOT, read_text

PKG = "chandy-lamport-distributed-snapshot-algorithm_amd"
cl = importlib.import_module(PKG)

TICK, MSGS, INFLIGHT, NODE, CH_MSGS, CH_TOK, KEY = range(7)
I64 = np.iinfo(np.int64)


class Axis(C.Structure):
    _fields_ = [("sid", C.c_int32), ("field", C.c_int32), ("index", C.c_int32), ("bins", C.c_int32),
                ("lo", C.c_int64), ("width", C.c_int64)]


def _sim(top, n=8):
    sim = cl.ChandyLamportSim(n)
    sim.read_topology_text(read_text(top))
    return sim


def _axis(sid=0, field=TICK, index=0, bins=4, lo=0, width=1):
    return np.array([(sid, field, index, bins, lo, width)], dtype=cl.CROSSTAB_AXIS_DTYPE)


def _call(sim, lo, hi, a, b, out, out_words=None):
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    words = (0 if out is None else out.size) if out_words is None else out_words
    return cl.lib().cl_snapshot_crosstab(sim._h, lo, hi, p(a), p(b), p(out), words)


def test_header_words_and_axis_struct():
    d = cl.CROSSTAB_AXIS_DTYPE
    assert d.itemsize == 32 == C.sizeof(Axis)
    assert d.names == ("sid", "field", "index", "bins", "lo", "width")
    assert [d.fields[k][1] for k in d.names] == [0, 4, 8, 12, 16, 24]
    assert [getattr(Axis, k).offset for k in d.names] == [0, 4, 8, 12, 16, 24]
    header = open(os.path.join(ROOT, "include", "clsnap.h")).read()
    words = dict(re.findall(r"#define (CL_XT_[A-Z_]+)\s+(\d+)", header))
    names = ("INSTANCES", "OK", "SAMPLE", "SUM_A", "SUM_B", "SUM_AA", "SUM_AB", "SUM_BB", "MIN_A", "MIN_B", "MAX_A",
             "MAX_B", "CELLS")
    assert {k: int(v) for k, v in words.items()} == {"CL_XT_" + k: i for i, k in enumerate(names)}
    assert [getattr(cl, "XT_" + k) for k in names] == list(range(13))
    limits = dict(re.findall(r"#define (CL_CROSSTAB_MAX_[A-Z]+)\s+(\d+)", header))
    assert limits == {"CL_CROSSTAB_MAX_BINS": "4096", "CL_CROSSTAB_MAX_CELLS": "4096"}
    assert cl.CROSSTAB_MAX_BINS == cl.CROSSTAB_MAX_CELLS == 4096
    assert re.search(r"typedef struct \{ int32_t sid, field, index, bins; int64_t lo, width; \} cl_crosstab_axis;", header)
    assert cl.CROSSTAB_FIELDS == ("tick", "msgs", "inflight", "node", "ch_msgs", "ch_tok")
    assert "SnapshotCrosstab" in cl.__all__ and "CROSSTAB_AXIS_DTYPE" in cl.__all__


def test_argument_errors_need_no_device():
    sim = _sim("3nodes.top", n=8)
    n_nodes, n_ch = sim.num_nodes, sim.num_channels
    out = np.full(12 + 16, 7, dtype=np.int64)
    good = _axis()
    # nothing has run: no event was ever issued
    assert _call(sim, 0, 8, good, good, out) == cl.E_STATE
    with pytest.raises(cl.ClSnapError) as e:
        sim.crosstab_time()
    assert e.value.code == cl.E_STATE
    with pytest.raises(cl.ClSnapError) as e:
        sim.snapshot_crosstab((0, "tick", None, 0, 1, 4), (0, "tick", None, 0, 1, 4))
    assert e.value.code == cl.E_STATE
    sim.ProcessEvent(cl.PassTokenEvent("N1", "N2", 1))
    assert sim.StartSnapshot("N1") == 0
    sim.Tick(2)

    def bad(*a, **kw):
        assert _call(sim, *a, **kw) == cl.E_INVALID, a

    bad(0, 8, None, good, out)                                        # NULL axes
    bad(0, 8, good, None, out)
    bad(0, 8, good, good, None, out_words=28)                         # NULL out
    for field in (KEY, -1, 6, 7, 100):                                # the key is not binnable; unknown fields
        bad(0, 8, _axis(field=field), good, out)
        bad(0, 8, good, _axis(field=field), out)
    for field, index in ((NODE, -1), (NODE, n_nodes), (CH_MSGS, -1), (CH_MSGS, n_ch), (CH_TOK, n_ch), (CH_TOK, -1),
                         (TICK, 1), (TICK, -1), (MSGS, 1), (INFLIGHT, 2)):
        bad(0, 8, _axis(field=field, index=index), good, out)
        bad(0, 8, good, _axis(field=field, index=index), out)
    for bins in (0, -1, 4097):
        bad(0, 8, _axis(bins=bins), _axis(bins=1), out)
        bad(0, 8, _axis(bins=1), _axis(bins=bins), out)
    big = np.full(12 + 128 * 64, 7, dtype=np.int64)
    bad(0, 8, _axis(bins=128), _axis(bins=64), big)                   # 8192 cells
    bad(0, 8, _axis(bins=4096), _axis(bins=2), big)
    for width in (0, -1, I64.min):
        bad(0, 8, _axis(width=width), good, out)
        bad(0, 8, good, _axis(width=width), out)
    for sid in (-1, 1):                                               # either sid
        bad(0, 8, _axis(sid=sid), good, out)
        bad(0, 8, good, _axis(sid=sid), out)
    for lo, hi in ((-1, 8), (0, 9), (5, 4)):
        bad(lo, hi, good, good, out)
    # the conditional form: a NULL set
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert cl.lib().cl_snapshot_crosstab_in(sim._h, 0, 8, None, p(good), p(good), p(out), out.size) == cl.E_INVALID
    # out too short for 12 + bins_a * bins_b words: after every other check
    assert _call(sim, 0, 8, good, good, out, out_words=27) == cl.E_LIMIT
    assert _call(sim, 0, 8, good, good, out, out_words=0) == cl.E_LIMIT
    assert _call(sim, 0, 8, _axis(bins=64), _axis(bins=64), big, out_words=12 + 4095) == cl.E_LIMIT
    assert _call(sim, 0, 8, _axis(sid=1), good, out, out_words=0) == cl.E_INVALID
    # nothing was written
    assert (out == 7).all() and (big == 7).all()
    assert cl.lib().cl_crosstab_time(sim._h, None) == cl.E_INVALID
    # the Python layer passes the C errors on
    with pytest.raises(cl.ClSnapError) as e:
        sim.snapshot_crosstab((1, "tick", None, 0, 1, 4), (0, "tick", None, 0, 1, 4))
    assert e.value.code == cl.E_INVALID
    with pytest.raises(cl.ClSnapError) as e:
        sim.snapshot_crosstab((0, "node", n_nodes, 0, 1, 4), (0, "tick", None, 0, 1, 4))
    assert e.value.code == cl.E_INVALID


def test_axis_normalisation():
    sim = _sim("8nodes.top")
    ids, chans = sim.node_ids(), sim.channels()
    src, dest = chans[5]
    cases = [
        ((0, "tick", None, 0, 1, 64), (0, TICK, 0, 64, 0, 1)),
        ((4, "tick", None, 26, 3, 4), (4, TICK, 0, 4, 26, 3)),
        ((1, "msgs", None, -5, 2, 9), (1, MSGS, 0, 9, -5, 2)),
        ((2, "inflight", None, I64.min, I64.max, 1), (2, INFLIGHT, 0, 1, I64.min, I64.max)),
        ((0, "node", ids[3], 1, 1, 16), (0, NODE, 3, 16, 1, 1)),
        ((0, "node", 6, I64.max, 1, 4096), (0, NODE, 6, 4096, I64.max, 1)),
        ((3, "ch_msgs", 7, 0, 1, 8), (3, CH_MSGS, 7, 8, 0, 1)),
        ((0, "ch_tok", (ids[src], ids[dest]), 0, 1, 16), (0, CH_TOK, 5, 16, 0, 1)),
        ((0, "ch_msgs", (src, dest), 0, np.int64(2), np.int32(3)), (0, CH_MSGS, 5, 3, 0, 2)),
    ]
    for axis, want in cases:
        got = sim.crosstab_axis(axis)
        assert got.dtype == cl.CROSSTAB_AXIS_DTYPE and got.shape == (1,) and got[0].tolist() == want, axis
    tick = (0, "tick", None, 0, 1, 4)
    for axis in ((0, "key", None, 0, 1, 4), (0, "ticks", None, 0, 1, 4), (0, "tick", None, 0, 1), tick + (1,),
                 (0, "tick", "N1", 0, 1, 4), (0, "node", None, 0, 1, 4), (0, "node", "N99", 0, 1, 4),
                 (0, "ch_tok", None, 0, 1, 4), (0, "ch_msgs", ("N1", "N7"), 0, 1, 4), (0, "tick", None, 0, 0, 4),
                 (0, "tick", None, 0, -1, 4), (0, "tick", None, 0, 1, 0), (0, "tick", None, 0, 1, 4097),
                 (-1, "tick", None, 0, 1, 4), (0, "tick", None, 2**63, 1, 4), (0, "tick", None, 0.5, 1, 4),
                 (0, "tick", None, None, 1, 4), (0, "tick", None, 0, 1, None), "tick", None):
        with pytest.raises(ValueError):
            sim.crosstab_axis(axis)
        # ... before the C call: nothing has run on this sim, which the C call would report first
        with pytest.raises(ValueError):
            sim.snapshot_crosstab(axis, tick)
        with pytest.raises(ValueError):
            sim.snapshot_crosstab(tick, axis)
    with pytest.raises(ValueError):
        sim.snapshot_crosstab((0, "tick", None, 0, 1, 128), (0, "tick", None, 0, 1, 64))


A4 = (0, TICK, 0, 4, 10, 1)
B3 = (1, NODE, 2, 3, -1, 1)


def _xt(pairs, a=A4, b=B3, instances=None, ok=None):
    """The crosstab of hand-made (a, b) value pairs, built word by word."""
    va = np.array([x for x, _ in pairs], dtype=np.int64)
    vb = np.array([y for _, y in pairs], dtype=np.int64)
    raw = np.zeros(12 + a[3] * b[3], dtype=np.int64)
    raw[0] = len(pairs) + 2 if instances is None else instances
    raw[1] = len(pairs) + 1 if ok is None else ok
    raw[2] = len(pairs)
    ua, ub = va.astype(np.uint64), vb.astype(np.uint64)
    raw[3], raw[4] = va.sum(), vb.sum()
    raw[5:8] = [(x * y).sum(dtype=np.uint64).view(np.int64) for x, y in ((ua, ua), (ua, ub), (ub, ub))]
    raw[8:10] = [va.min(), vb.min()] if len(pairs) else I64.max
    raw[10:12] = [va.max(), vb.max()] if len(pairs) else I64.min
    for x, y in pairs:
        ia = 0 if x < a[4] else min((x - a[4]) // a[5], a[3] - 1)
        ib = 0 if y < b[4] else min((y - b[4]) // b[5], b[3] - 1)
        raw[12 + ia * b[3] + ib] += 1
    return cl.SnapshotCrosstab((np.array([a], dtype=cl.CROSSTAB_AXIS_DTYPE), np.array([b], dtype=cl.CROSSTAB_AXIS_DTYPE)),
                               raw)


PAIRS_A = [(10, -1), (11, 0), (11, 0), (13, 1), (12, -1), (10, 1)]
PAIRS_B = [(12, 0), (13, 1), (13, 1), (11, -1)]


def test_snapshot_crosstab_views():
    x = _xt(PAIRS_A)
    assert (x.instances, x.ok, x.sample) == (8, 7, 6) and x.shape == (4, 3)
    assert x.table.shape == (4, 3) and x.table.dtype == np.int64 and int(x.table.sum()) == 6
    assert x.table.tolist() == [[1, 0, 1], [0, 2, 0], [1, 0, 0], [0, 0, 1]]
    assert x.marginal(0).tolist() == [2, 2, 1, 1] and x.marginal(1).tolist() == [2, 2, 2]
    assert x.min == (10, -1) and x.max == (13, 1)
    assert x.raw.shape == (24,) and x.raw.dtype == np.int64
    for axis in (2, -1, None):
        with pytest.raises(ValueError):
            x.marginal(axis)
    with pytest.raises(ValueError):
        cl.SnapshotCrosstab(x.axes, x.raw[:-1])
    empty = _xt([])
    assert empty.sample == 0 and empty.min == (I64.max, I64.max) and empty.max == (I64.min, I64.min)
    assert not empty.table.any()
    assert all(np.isnan(v) for v in (empty.mean(0), empty.variance(1), empty.covariance(), empty.correlation()))


def test_covariance_and_correlation_against_numpy():
    # width-1 bins that hold every value: the table alone determines the moments
    rng = np.random.default_rng(7)
    va = rng.integers(0, 16, 500)
    vb = np.clip(va // 2 + rng.integers(-2, 3, 500), -3, 12)
    a, b = (0, TICK, 0, 16, 0, 1), (1, NODE, 0, 16, -3, 1)
    x = _xt(list(zip(va.tolist(), vb.tolist())), a, b)
    assert int(x.table.sum()) == 500 and x.table[3, 4] == int(((va == 3) & (vb == 1)).sum())
    assert np.array_equal(x.marginal(0), np.bincount(va, minlength=16))
    assert np.array_equal(x.marginal(1), np.bincount(vb + 3, minlength=16))
    assert np.isclose(x.mean(0), va.mean(), rtol=1e-12, atol=0) and np.isclose(x.mean(1), vb.mean(), rtol=1e-12, atol=0)
    assert np.isclose(x.variance(0), va.var(), rtol=1e-12, atol=0)
    assert np.isclose(x.variance(1), vb.var(), rtol=1e-12, atol=0)
    cov = np.cov(va, vb, bias=True)[0, 1]
    assert np.isclose(x.covariance(), cov, rtol=1e-11, atol=0)
    assert np.isclose(x.correlation(), np.corrcoef(va, vb)[0, 1], rtol=1e-11, atol=0)
    # ... and the same from the table's cells, as a user of the table would compute them
    ia, ib = np.nonzero(x.table)
    w = x.table[ia, ib]
    ma, mb = (w * ia).sum() / 500, (w * (ib - 3)).sum() / 500
    assert np.isclose(x.covariance(), (w * (ia - ma) * (ib - 3 - mb)).sum() / 500, rtol=1e-11, atol=0)
    # a negative sum of products reads through the int64 view of the wrapped word
    y = _xt([(3, -4), (5, -1), (9, 2)], a, (1, NODE, 0, 16, -8, 1))
    assert y.raw[cl.XT_SUM_AB] == -12 - 5 + 18
    assert np.isclose(y.covariance(), np.cov([3, 5, 9], [-4, -1, 2], bias=True)[0, 1], rtol=1e-12, atol=0)
    # a constant axis has no correlation
    assert np.isnan(_xt([(3, 1), (3, 2)]).correlation())


def test_snapshot_crosstab_merge():
    a, b = _xt(PAIRS_A), _xt(PAIRS_B)
    m = a.merge(b)
    assert m == _xt(PAIRS_A + PAIRS_B, instances=a.instances + b.instances, ok=a.ok + b.ok)   # the cell-wise sum
    assert np.array_equal(m.table, a.table + b.table) and m == b.merge(a)
    assert m.min == (10, -1) and m.max == (13, 1) and m.sample == 10
    lo = _xt([(12, 0)])
    assert a.merge(lo).min == a.min and lo.merge(_xt([(13, 1)])).min == (12, 0) and lo.merge(_xt([(13, 1)])).max == (13, 1)
    # an empty side leaves the other's extrema
    empty = _xt([], instances=5, ok=0)
    assert empty.merge(a) == _xt(PAIRS_A, instances=a.instances + 5, ok=a.ok) == a.merge(empty)
    assert empty.merge(empty).min == (I64.max, I64.max) and empty.merge(empty).max == (I64.min, I64.min)
    # the moments wrap modulo 2**64
    wide = (0, TICK, 0, 2, 0, 1)
    big = _xt([(2**61 + 1, -(2**61)), (2**61 + 1, 3)], wide, wide)
    assert big.raw[cl.XT_SUM_A] == 2**62 + 2 and big.raw[cl.XT_SUM_AA] == 2**63 + 2 - 2**64
    twice = big.merge(big)
    assert twice.raw[cl.XT_SUM_A] == I64.min + 4                     # 2**63 + 4 wraps
    assert twice.raw[cl.XT_SUM_AA] == 4                              # 2 * (2**63 + 2) modulo 2**64
    for word in (cl.XT_SUM_AB, cl.XT_SUM_BB, cl.XT_SUM_B):
        want = (2 * (int(big.raw[word]) & (2**64 - 1))) & (2**64 - 1)
        assert int(twice.raw[word]) & (2**64 - 1) == want
    assert twice.table.tolist() == [[0, 0], [2, 2]]
    # mismatched axes are refused
    for other in (_xt(PAIRS_A, a=(0, TICK, 0, 4, 10, 2)), _xt(PAIRS_A, b=(0, NODE, 2, 3, -1, 1)),
                  _xt(PAIRS_A, a=B3, b=(0, TICK, 0, 4, 10, 1)), _xt(PAIRS_A, b=(1, NODE, 2, 6, -1, 1)), None, a.raw):
        with pytest.raises(ValueError):
            a.merge(other)
    assert a != _xt(PAIRS_A, a=(0, TICK, 0, 4, 10, 2)) and a == _xt(PAIRS_A) and a != b


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _parts():
    return _xt(PAIRS_A), _xt(PAIRS_B)


def _worker(rank, world, port, out):
    import sys
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    d = importlib.import_module(PKG + ".dist")
    g = d.reduce_crosstab(_parts()[rank], "cpu")
    out[rank] = (g.axes[0].tobytes(), g.axes[1].tobytes(), g.raw.tobytes())
    dist.destroy_process_group()


def test_reduce_crosstab_two_ranks_gloo_equals_merge():
    a, b = _parts()
    want = a.merge(b)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    for r in range(2):
        assert out[r] == (want.axes[0].tobytes(), want.axes[1].tobytes(), want.raw.tobytes())
    # without a process group the call returns a copy
    d = importlib.import_module(PKG + ".dist")
    alone = d.reduce_crosstab(a, "cpu")
    assert alone == a and alone.raw is not a.raw and alone.axes[0] is not a.axes[0]
