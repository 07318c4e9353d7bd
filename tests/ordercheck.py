"""Expected values of ChandyLamportSim.snapshot_topk / snapshot_quantiles / snapshot_values, computed
in numpy from the oracle.

The per-instance quantities are selectcheck.values over the oracle rows the statistics, census and
select checks use.  The sample, the order -- np.lexsort((instance, +-value)) -- and the nearest-rank
rule in Python integers are rebuilt here, independently of the engine; everything compares exactly.
A term is (sid, field, index) with index None or an int (node rank, channel number).
"""
import numpy as np

import oracle as O
from selectcheck import values


def term_values(rows, keys, term):
    """int64[rows.n]: the term's value of every instance (a key as its int64 bit pattern)."""
    sid, field, index = term
    v = np.asarray(values(rows, keys, sid, field, 0 if index is None else index))
    return v.view(np.int64) if v.dtype == np.uint64 else v.astype(np.int64)


def sample_of(rows, term, lo, hi, mask=None):
    """The sample's absolute instance indices, ascending: OK, the term's snapshot completed, in
    [lo, hi) and in `mask`."""
    sid = term[0]
    if sid >= rows.n_sids or hi <= lo:
        return np.zeros(0, dtype=np.int64)
    pick = rows.done[sid].copy() if mask is None else rows.done[sid] & np.asarray(mask, dtype=bool)
    pick[:lo] = False
    pick[hi:] = False
    return np.flatnonzero(pick).astype(np.int64)


def info_of(rows, term, lo, hi, mask=None):
    """(instances, ok, sample)."""
    return max(hi - lo, 0), int((rows.status[lo:hi] == O.OK).sum()), int(sample_of(rows, term, lo, hi, mask).size)


def ordered(insts, vals, descending):
    """(insts, vals) in the order of the calls: value ascending (descending), instance ascending."""
    order = np.lexsort((insts, -vals if descending else vals))
    return insts[order], vals[order]


def expected_topk(rows, keys, term, k, descending, lo, hi, mask=None):
    """(info, insts, values): info = (instances, ok, sample), the first min(k, sample) of the order."""
    members = sample_of(rows, term, lo, hi, mask)
    insts, vals = ordered(members, term_values(rows, keys, term)[members], descending)
    return info_of(rows, term, lo, hi, mask), insts[:k], vals[:k]


def rank_of(num, den, sample):
    """The nearest-rank position, in Python integers."""
    return 0 if num == 0 else -((-num * sample) // den) - 1


def expected_quantiles(rows, keys, term, qs, lo, hi, mask=None):
    """(info, ranks, values) for qs = [(num, den)]; on an empty sample ranks -1 and values None."""
    members = sample_of(rows, term, lo, hi, mask)
    info = info_of(rows, term, lo, hi, mask)
    if members.size == 0:
        return info, np.full(len(qs), -1, dtype=np.int64), None
    vals = np.sort(term_values(rows, keys, term)[members])
    ranks = np.array([rank_of(num, den, members.size) for num, den in qs], dtype=np.int64)
    assert ((ranks >= 0) & (ranks < members.size)).all()
    return info, ranks, vals[ranks]


def expected_values(rows, keys, term, lo, hi, mask=None):
    """(values int64[hi - lo], in_sample bool[hi - lo]): 0 outside the sample."""
    members = sample_of(rows, term, lo, hi, mask)
    out = np.zeros(max(hi - lo, 0), dtype=np.int64)
    member = np.zeros(max(hi - lo, 0), dtype=bool)
    out[members - lo] = term_values(rows, keys, term)[members]
    member[members - lo] = True
    return out, member


def assert_topk_equal(got, want, k, descending, what=""):
    info, insts, vals = want
    assert (got.instances, got.ok, got.sample) == info, f"{what}: info {(got.instances, got.ok, got.sample)} != {info}"
    assert got.k == k and got.descending == descending and got.n_returned == min(k, info[2]) == insts.size, \
        f"{what}: n_returned {got.n_returned}"
    assert got.insts.dtype == np.int64 and got.values.dtype == np.int64
    if not np.array_equal(got.insts, insts):
        bad = int(np.flatnonzero(got.insts != insts)[0])
        raise AssertionError(f"{what}: row {bad}: instance {got.insts[bad]} (value {got.values[bad]}), "
                             f"expected {insts[bad]} (value {vals[bad]})")
    assert np.array_equal(got.values, vals), f"{what}: values differ"


def assert_quantiles_equal(got, want, what=""):
    info, ranks, vals = want
    assert (got.instances, got.ok, got.sample) == info, f"{what}: info"
    assert np.array_equal(got.ranks, ranks), f"{what}: ranks {got.ranks.tolist()} != {ranks.tolist()}"
    if vals is not None:
        assert np.array_equal(got.values, vals), f"{what}: values {got.values.tolist()} != {vals.tolist()}"


def plane_expected(vals, member, k, descending, qs=None):
    """What order_plane_device must return for a plane: (insts, vals, q_values, q_ranks)."""
    vals = np.asarray(vals, dtype=np.int64)
    members = np.arange(vals.size, dtype=np.int64) if member is None else np.flatnonzero(member).astype(np.int64)
    # (-INT64_MIN overflows: order by the complement instead, which reverses int64 exactly)
    key = ~vals[members] if descending else vals[members]
    order = np.lexsort((members, key))[:k]
    qv = qr = None
    if qs is not None:
        qr = np.array([rank_of(num, den, members.size) if members.size else -1 for num, den in qs], dtype=np.int64)
        qv = np.sort(vals[members])[qr] if members.size else None
    return members[order], vals[members][order], qv, qr
