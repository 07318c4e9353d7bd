"""Expected values of ChandyLamportSim.select_instances, computed in numpy from the oracle.

The per-instance quantities come from the oracle rows the statistics and census checks use
(statscheck.Rows: sample flags, ticks, tokenMap rows, per-channel message counts and token sums;
censuscheck.CensusRows: the content keys).  Clauses are evaluated here, independently of the
engine; a scenario's oracle runs are made once and shared.
"""
import functools

import numpy as np

import oracle as O
from censuscheck import CensusRows
from censuscheck import scenario_rows as census_rows
from statscheck import Rows

FIELDS = ("tick", "msgs", "inflight", "node", "ch_msgs", "ch_tok", "key")
I64 = np.iinfo(np.int64)


@functools.lru_cache(maxsize=None)
def scenario(top, events, n):
    """(rows, keys) of n instances of a scenario: one oracle run per instance (the census checks'
    cached runs), viewed as statscheck.Rows and censuscheck.CensusRows."""
    keys = census_rows(top, events, n)
    return Rows(keys.refs), keys


def from_refs(refs):
    return Rows(refs), CensusRows(refs)


def values(rows, keys, sid, field, index):
    """The per-instance value of a clause's field, as Python-int-safe numpy (uint64 for the key)."""
    if field == "tick":
        return rows.tick[sid]
    if field == "msgs":
        return rows.ch_msgs[sid].sum(axis=1)
    if field == "inflight":
        return rows.ch_tok[sid].sum(axis=1)
    if field == "node":
        return rows.node[sid][:, index]
    if field == "ch_msgs":
        return rows.ch_msgs[sid][:, index]
    if field == "ch_tok":
        return rows.ch_tok[sid][:, index]
    assert field == "key"
    return keys.key[sid]


def expected(rows, keys, sid, lo, hi, clauses):
    """(info, insts, ticks) cl_select_instances must return for instances [lo, hi): info =
    (instances, ok, sample, n_match), insts int64 ascending (absolute), ticks int32.  A clause is
    (field, index, lo, hi) or (field, index, lo, hi, "not") with index None or an int (node rank,
    channel number) and None for an open end."""
    ok = int((rows.status[lo:hi] == O.OK).sum())
    if sid >= rows.n_sids or hi <= lo:
        return (hi - lo, ok, 0, 0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
    match = rows.done[sid].copy()
    assert np.array_equal(match, keys.done[sid])
    for clause in clauses:
        field, index, a, b = clause[:4]
        v = values(rows, keys, sid, field, 0 if index is None else index)
        if field == "key":
            a, b = np.uint64(0 if a is None else a), np.uint64(2**64 - 1 if b is None else b)
        else:
            a, b = np.int64(I64.min if a is None else a), np.int64(I64.max if b is None else b)
        inside = (v >= a) & (v <= b)
        match &= ~inside if len(clause) == 5 else inside
    sample = int(rows.done[sid][lo:hi].sum())
    insts = np.flatnonzero(match[lo:hi]).astype(np.int64) + lo
    return (hi - lo, ok, sample, insts.size), insts, rows.tick[sid][insts].astype(np.int32)


def assert_selection_equal(got, want, what="", max_out=None):
    """The info, the indices and (when returned) the ticks, exactly."""
    info, insts, ticks = want
    assert (got.instances, got.ok, got.sample, got.n_match) == info, \
        f"{what}: info {(got.instances, got.ok, got.sample, got.n_match)}, expected {info}"
    k = insts.size if max_out is None else min(insts.size, max_out)
    assert got.n_returned == k and got.truncated == (k < insts.size), f"{what}: n_returned {got.n_returned}"
    assert got.insts.dtype == np.int64 and np.array_equal(got.insts, insts[:k]), f"{what}: instances differ"
    if got.ticks is not None:
        assert got.ticks.dtype == np.int32 and np.array_equal(got.ticks, ticks[:k]), f"{what}: ticks differ"
