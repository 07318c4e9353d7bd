"""Expected values of ChandyLamportSim.snapshot_crosstab, computed in numpy from the oracle.

The per-instance values of an axis are selectcheck.values over the oracle rows the statistics,
census and select checks use (selectcheck.scenario); the joint sample is done[sid_a] & done[sid_b],
cut to the range and, for the conditional call, to the set's mask.  Every word of the flat result
is rebuilt here, independently of the engine, and compared exactly.

An axis is (sid, field, index, lo, width, bins) with index None or an int (node rank, channel number).
"""
import numpy as np

import oracle as O
from selectcheck import values

I64 = np.iinfo(np.int64)
(XT_INSTANCES, XT_OK, XT_SAMPLE, XT_SUM_A, XT_SUM_B, XT_SUM_AA, XT_SUM_AB, XT_SUM_BB, XT_MIN_A, XT_MIN_B, XT_MAX_A,
 XT_MAX_B, XT_CELLS) = range(13)
WORDS = ("instances", "ok", "sample", "sum_a", "sum_b", "sum_aa", "sum_ab", "sum_bb", "min_a", "min_b", "max_a",
         "max_b")


def bins_of(v, lo, width, bins):
    """bin(v) = v < lo ? 0 : min((uint64)(v - lo) / width, bins - 1), in Python integers."""
    return np.array([0 if x < lo else min((x - lo) // width, bins - 1) for x in (int(x) for x in v)], dtype=np.int64)


def joint_sample(rows, a, b, lo, hi, mask=None):
    """The absolute indices of the joint sample of axes a and b over [lo, hi)."""
    if a[0] >= rows.n_sids or b[0] >= rows.n_sids or hi <= lo:
        return np.zeros(0, dtype=np.int64)
    both = rows.done[a[0]] & rows.done[b[0]]
    if mask is not None:
        both = both & mask
    return np.flatnonzero(both[lo:hi]).astype(np.int64) + lo


def expected(rows, keys, a, b, lo, hi, mask=None):
    """The flat int64 array cl_snapshot_crosstab must return for instances [lo, hi)."""
    raw = np.zeros(XT_CELLS + a[5] * b[5], dtype=np.int64)
    raw[XT_MIN_A] = raw[XT_MIN_B] = I64.max
    raw[XT_MAX_A] = raw[XT_MAX_B] = I64.min
    raw[XT_INSTANCES] = max(hi - lo, 0)
    raw[XT_OK] = int((rows.status[lo:hi] == O.OK).sum())
    pick = joint_sample(rows, a, b, lo, hi, mask)
    raw[XT_SAMPLE] = pick.size
    if pick.size == 0:
        return raw
    va, vb = (values(rows, keys, z[0], z[1], 0 if z[2] is None else z[2])[pick].astype(np.int64) for z in (a, b))
    ua, ub = va.astype(np.uint64), vb.astype(np.uint64)
    raw[XT_SUM_A], raw[XT_SUM_B] = int(va.sum()), int(vb.sum())
    for word, prod in ((XT_SUM_AA, ua * ua), (XT_SUM_AB, ua * ub), (XT_SUM_BB, ub * ub)):   # modulo 2**64
        raw[word] = prod.sum(dtype=np.uint64).view(np.int64)
    raw[XT_MIN_A], raw[XT_MIN_B], raw[XT_MAX_A], raw[XT_MAX_B] = va.min(), vb.min(), va.max(), vb.max()
    cells = np.zeros((a[5], b[5]), dtype=np.int64)
    np.add.at(cells, (bins_of(va, *a[3:]), bins_of(vb, *b[3:])), 1)
    raw[XT_CELLS:] = cells.ravel()
    return raw


def assert_crosstab_equal(got, want, what=""):
    """Every word exactly; names the first word that differs."""
    got = np.asarray(got)
    assert got.dtype == np.int64 and got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    if np.array_equal(got, want):
        return
    bad = int(np.flatnonzero(got != want)[0])
    name = WORDS[bad] if bad < XT_CELLS else f"cell {bad - XT_CELLS}"
    raise AssertionError(f"{what}: {int((got != want).sum())} words differ; first at {name}: got {got[bad]}, "
                         f"expected {want[bad]}")
