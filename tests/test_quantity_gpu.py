"""A quantity of a snapshot -- (sid, field, index) -- has one value per instance, whichever call reads
it: the group-by term, the crosstab axis and the select clause (cl_quantity.h) against the oracle.

For a quantity, v = selectcheck.values over one OracleSim per instance (selectcheck.scenario's cached
runs) and H = the histogram of v over the sample of [lo, hi).  Then, exactly:
  snapshot_groups([q]) returns the pairs (value, count) of H;
  snapshot_crosstab with axis a = q binned one value per bin from min v to max v, and axis b the
    completion tick of the same snapshot in one bin, has marginal H (not for the key: a hash is not
    binnable);
  select_instances(sid, [(field, index, x, x)]) returns the instances with v == x, for the up to
    three most frequent x (a key through its unsigned bounds).
One case per scenario reads the quantity of a snapshot other than the walk's: as the second term of
a group-by behind the completion tick of the walk's snapshot, and as axis b of a crosstab whose axis
a is that tick -- over the instances in which both snapshots completed.

Scenarios, ranges and layouts are those of the census and group-by tests: the 3-node scenario
(records staged in LDS), the ring with 2-word node records (staged with scalar loads) and the hub
with 33 record words (not staged); instance-major records after flush(), block-major by slot after
rerun() of a mapped plan.  What keeps a case from passing vacuously is asserted on the oracle rows
before any device call (conditions()).
"""
import collections

import numpy as np
import pytest

from selectcheck import FIELDS, scenario, values
from statscheck import RING_EVENTS, RING_TOP
from test_census_gpu import AUTO, EVENTS3, HUB_EVENTS, HUB_TOP, TOP3, both_layouts, make_sim

pytestmark = pytest.mark.gpu

N = 4096                        # the smallest batch that gets a mapped block-major replay
RANGES = [(0, N), (37, 3001)]
MAX_BINS = 4096                 # per crosstab axis

# per scenario: the quantities (sid, field, index) read by all three calls, and (walk's sid,
# quantity of another snapshot); the indices are ones whose values vary in the oracle's runs
SCENARIOS = {
    "top3": (TOP3, EVENTS3,
             [(0, "tick", None), (1, "msgs", None), (0, "inflight", None), (0, "node", 1), (1, "node", 2),
              (0, "ch_msgs", 0), (0, "ch_tok", 0), (1, "key", None)],
             [(0, (1, "ch_tok", 1)), (1, (0, "key", None))]),
    "ring": (RING_TOP, RING_EVENTS,
             [(0, "tick", None), (1, "msgs", None), (0, "inflight", None), (0, "node", 2), (1, "ch_msgs", 4),
              (0, "ch_tok", 1), (1, "key", None)],
             [(0, (1, "node", 0))]),
    "hub": (HUB_TOP, HUB_EVENTS,
            [(0, "tick", None), (2, "msgs", None), (1, "inflight", None), (1, "node", 4), (3, "ch_msgs", 13),
             (0, "ch_tok", 0), (3, "key", None)],
            [(1, (3, "node", 4)), (2, (0, "inflight", None))]),
}


def quantity(rows, keys, q, sids, lo, hi):
    """(v, m): the quantity's per-instance values and the sample of [lo, hi) over the snapshots `sids`."""
    sid, field, index = q
    m = np.zeros(rows.status.size, dtype=bool)
    m[lo:hi] = True
    for s in sids:
        m &= rows.done[s]
    return values(rows, keys, sid, field, 0 if index is None else index), m


def histogram(*columns):
    """{value or tuple of values: count} of the columns' rows, as Python ints."""
    cols = [c.tolist() for c in columns]
    return dict(collections.Counter(cols[0] if len(cols) == 1 else zip(*cols)))


def typed(column, field):
    """A column of snapshot_groups' int64 values as the oracle's type (a key: uint64)."""
    return column.view(np.uint64) if field == "key" else column


def bins_of(v):
    return int(v.max()) - int(v.min()) + 1


def conditions(rows, keys, cases, others):
    """What the cases must exercise, on the oracle rows alone."""
    assert {q[1] for q in cases} == set(FIELDS)                      # every field; all but the key binned
    assert {q[1] for q in cases if q[1] != "key"} == set(FIELDS) - {"key"}
    assert others and all(q[0] != sid0 for sid0, q in others)         # the view of another snapshot
    for lo, hi in RANGES:
        for q, sids in [(q, [q[0]]) for q in cases] + [(q, [sid0, q[0]]) for sid0, q in others]:
            v, m = quantity(rows, keys, q, sids, lo, hi)
            assert m.any() and np.unique(v[m]).size >= 2, f"{q} [{lo}, {hi})"
            assert q[1] == "key" or bins_of(v[m]) <= MAX_BINS, f"{q} [{lo}, {hi})"


def check_one_snapshot(sim, rows, keys, q, lo, hi, what):
    sid, field, index = q
    v, m = quantity(rows, keys, q, [sid], lo, hi)
    H = histogram(v[m])
    g = sim.snapshot_groups([q], lo, hi)
    assert g.sample == int(m.sum()) and g.n_returned == g.n_groups == len(H), what
    assert histogram(typed(g.values[:, 0], field)) == dict.fromkeys(H, 1), what
    assert dict(zip(typed(g.values[:, 0], field).tolist(), g.groups["count"].tolist())) == H, what
    if field != "key":
        v0, bins = int(v[m].min()), bins_of(v[m])
        xt = sim.snapshot_crosstab((sid, field, index, v0, 1, bins), (sid, "tick", None, 0, 1, 1), lo, hi)
        assert xt.sample == int(m.sum()), what
        assert xt.marginal(0).tolist() == [H.get(v0 + k, 0) for k in range(bins)], what
    for x in sorted(H, key=lambda x: (-H[x], x))[:3]:
        got = sim.select_instances(sid, [(field, index, x, x)], lo, hi)
        assert got.insts.tolist() == np.flatnonzero(m & (v == x)).tolist(), f"{what} == {x}"


def check_other_snapshot(sim, rows, keys, sid0, q, lo, hi, what):
    sid, field, index = q
    v, m = quantity(rows, keys, q, [sid0, sid], lo, hi)
    g = sim.snapshot_groups([(sid0, "tick", None), q], lo, hi)
    assert g.sample == int(m.sum()) and g.n_returned == g.n_groups, what
    pairs = list(zip(g.values[:, 0].tolist(), typed(g.values[:, 1], field).tolist()))
    assert len(set(pairs)) == len(pairs), what
    assert dict(zip(pairs, g.groups["count"].tolist())) == histogram(rows.tick[sid0][m], v[m]), what
    if field != "key":
        H, v0, bins = histogram(v[m]), int(v[m].min()), bins_of(v[m])
        xt = sim.snapshot_crosstab((sid0, "tick", None, 0, 1, 1), (sid, field, index, v0, 1, bins), lo, hi)
        assert xt.sample == int(m.sum()), what
        assert xt.marginal(1).tolist() == [H.get(v0 + k, 0) for k in range(bins)], what


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_one_value_whichever_call_reads_it(name):
    top, events, cases, others = SCENARIOS[name]
    rows, keys = scenario(top, events, N)
    conditions(rows, keys, cases, others)
    sim = make_sim(top, events, N, AUTO)
    # (of these only the hub's 11 x 3 record words are not staged)
    assert (sim.num_nodes, sim.num_channels) == {"top3": (3, 6), "ring": (5, 5), "hub": (11, 21)}[name]

    def body(layout):
        for lo, hi in RANGES:
            for q in cases:
                check_one_snapshot(sim, rows, keys, q, lo, hi, f"{name} {layout} {q} [{lo}, {hi})")
            for sid0, q in others:
                check_other_snapshot(sim, rows, keys, sid0, q, lo, hi, f"{name} {layout} {sid0}: {q} [{lo}, {hi})")

    both_layouts(sim, AUTO, body)
