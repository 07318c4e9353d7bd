"""Expected values of the conditional analytics (snapshot_stats_in, snapshot_census_in,
select_instances_in) and of InstanceSet itself, computed in numpy from the oracle.

A set is a boolean mask over the instances.  `rows_in` / `keys_in` give a view of the oracle rows
(statscheck.Rows, censuscheck.CensusRows) in which done[sid] &= mask for every sid: the status is
untouched, so `instances` and `ok` stay those of the range, and the existing expected() functions
of statscheck, censuscheck and selectcheck then produce the conditional result.  Clause masks are
evaluated here with selectcheck.values, independently of the engine.
"""
import copy

import numpy as np

from selectcheck import I64, values


def clause_mask(rows, keys, sid, clauses, lo=0, hi=None):
    """The members of sim.instance_set(sid, clauses, lo, hi): the instances of [lo, hi) in the sample
    of `sid` (status OK, completed) that satisfy every clause, as bool[rows.n]."""
    hi = rows.n if hi is None else hi
    mask = np.zeros(rows.n, dtype=bool)
    if sid >= rows.n_sids or hi <= lo:
        return mask
    mask[lo:hi] = rows.done[sid][lo:hi]
    for clause in clauses:
        field, index, a, b = clause[:4]
        v = values(rows, keys, sid, field, 0 if index is None else index)
        if field == "key":
            a, b = np.uint64(0 if a is None else a), np.uint64(2**64 - 1 if b is None else b)
        else:
            a, b = np.int64(I64.min if a is None else a), np.int64(I64.max if b is None else b)
        inside = (v >= a) & (v <= b)
        mask &= ~inside if len(clause) == 5 else inside
    return mask


def list_mask(n, insts):
    """The members of sim.instance_set_from(insts) as bool[n]."""
    mask = np.zeros(n, dtype=bool)
    mask[np.asarray(insts, dtype=np.int64)] = True
    return mask


def _view(rows, mask):
    mask = np.asarray(mask, dtype=bool)
    assert mask.shape == (rows.n,)
    view = copy.copy(rows)
    view.done = [d & mask for d in rows.done]
    return view


def rows_in(rows, mask):
    """statscheck.Rows restricted to the set: done[sid] &= mask, everything else shared."""
    return _view(rows, mask)


def keys_in(keys, mask):
    """censuscheck.CensusRows restricted to the set."""
    return _view(keys, mask)


def members(mask, lo=0, hi=None):
    """What InstanceSet.insts(lo, hi) must return: ascending int64 absolute indices."""
    hi = mask.size if hi is None else hi
    return np.flatnonzero(mask[lo:hi]).astype(np.int64) + lo
