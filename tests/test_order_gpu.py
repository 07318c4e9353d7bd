"""ChandyLamportSim.snapshot_topk / snapshot_quantiles / snapshot_values and their _in forms
(cl_snapshot_topk, cl_snapshot_quantiles, cl_snapshot_values; cl_order.hip) against the oracle, and
the kernels' test aid (order_plane_device) against numpy over the whole int64 range.

Expected values: ordercheck over one OracleSim per instance (selectcheck.scenario's cached runs); the
info, every instance, every value and every rank must be equal exactly.  Scenarios, ranges and
layouts are those of the census, select and group-by tests: the library's choice of exec kernel
(AUTO) and the instance-per-lane kernel forced, instance-major records after flush() and block-major
by slot after rerun() of a mapped plan.  What is asserted on the oracle shows that each test reaches
its regime.
"""
import functools
import importlib

import numpy as np
import pytest

import oracle as O
from blockedcheck import (LANES, N_RING17, NODES, RING17_EVENTS, RING17_TOP, SLOTS, UNDRAINED_EVENTS,
                          blocked_ragged_sim, build_sim, undrained_refs)
from isetcheck import clause_mask
from ordercheck import (assert_quantiles_equal, assert_topk_equal, expected_quantiles, expected_topk, expected_values,
                        info_of, plane_expected, sample_of, term_values)
from selectcheck import from_refs, scenario
from test_blocked_ragged_gpu import ranges_of
from test_census_gpu import AUTO, C3_EVENTS, C3_TOP, ENGINES, HUB_EVENTS, HUB_TOP, both_layouts, make_sim

cl = importlib.import_module("chandy-lamport-distributed-snapshot-algorithm_amd")
pytestmark = pytest.mark.gpu

N = 4096                        # the smallest batch that gets a mapped block-major replay
RANGES = [(0, N), (37, 3001)]
I64 = np.iinfo(np.int64)


def tick(sid):
    return (sid, "tick", None)


C3_TERMS = [tick(0), tick(4), (0, "inflight", None), (4, "msgs", None), (1, "node", 4), (3, "ch_tok", 2),
            (2, "ch_msgs", 5)]


def ks_of(sample):
    return sorted({0, 1, 16, 1000, sample, sample + 5})


def qs_of(sample):
    """0, 1/2, 99/100, 1, and the two next to the ends."""
    qs = [(0, 1), (1, 2), (99, 100), (1, 1)]
    return qs + [(1, sample), (sample - 1, sample)] if sample > 0 else qs


def check(sim, rows, keys, terms, ranges, what, iset=None, mask=None, ks=ks_of, values=True):
    """Top-k in both directions at every k, the quantiles and the values of every term over every range."""
    for term in terms:
        for lo, hi in ranges:
            tag = f"{what} {term} [{lo}, {hi})"
            sample = info_of(rows, term, lo, hi, mask)[2]
            for largest in (False, True):
                info, insts, vals = expected_topk(rows, keys, term, sample + 5, largest, lo, hi, mask)
                for k in ks(sample):
                    got = (sim.snapshot_topk(term, k, largest, lo, hi) if iset is None
                           else sim.snapshot_topk_in(iset, term, k, largest, lo, hi))
                    assert_topk_equal(got, (info, insts[:k], vals[:k]), k, largest, f"{tag} k {k} largest {largest}")
            qs = qs_of(sample)
            got = sim.snapshot_quantiles(term, qs, lo, hi) if iset is None else sim.snapshot_quantiles_in(iset, term, qs, lo, hi)
            assert_quantiles_equal(got, expected_quantiles(rows, keys, term, qs, lo, hi, mask), tag)
            if sample:
                assert [cl.quantile_rank(q, sample) for q in qs] == got.ranks.tolist()
            if values:
                check_values(sim, rows, keys, term, lo, hi, tag, iset, mask)


def check_values(sim, rows, keys, term, lo, hi, tag, iset=None, mask=None):
    v, member = sim.snapshot_values(term, lo, hi) if iset is None else sim.snapshot_values_in(iset, term, lo, hi)
    want_v, want_m = expected_values(rows, keys, term, lo, hi, mask)
    assert v.dtype == np.int64 and member.dtype == bool
    assert np.array_equal(member, want_m), f"{tag}: in_sample"
    assert np.array_equal(v, want_v), f"{tag}: values"


# ---- 1: C3, five snapshot ids, mixed statuses, ties at the boundary ----------------------------------------
@ENGINES
def test_c3_terms_directions_and_every_k(engine):
    rows, keys = scenario(C3_TOP, C3_EVENTS, N)
    assert rows.n_sids == 5
    bad = rows.status == O.FATAL_INSUFFICIENT_TOKENS
    assert int(bad.sum()) == 117                                            # the exclusion is exercised
    assert info_of(rows, tick(0), 0, N) == (N, 3979, 3979) and info_of(rows, tick(0), 37, 3001)[2] == 2880
    # at k = 16 and k = 1000 the boundary of tick(0) falls inside a tie group: the instance rule decides
    for lo, hi in RANGES:
        for largest in (False, True):
            _, insts, vals = expected_topk(rows, keys, tick(0), N, largest, lo, hi)
            for k in (16, 1000):
                assert vals[k - 1] == vals[k] and insts[k - 1] < insts[k], (lo, hi, largest, k)
            assert not bad[insts].any()                                     # no non-OK instance is listed
    sim = make_sim(C3_TOP, C3_EVENTS, N, engine)

    def body(what):
        check(sim, rows, keys, C3_TERMS, RANGES, what)
        for lo, hi in RANGES:
            check_values(sim, rows, keys, (0, "key", None), lo, hi, f"{what} key [{lo}, {hi})")
        top = sim.snapshot_topk(tick(0), 16, True)
        assert not bad[top.insts].any() and sim.order_time() > 0
        walk, select, compact = sim.order_time(stages=True)
        assert walk > 0 and select > 0 and compact > 0

    both_layouts(sim, engine, body)
    names = sim.snapshot_topk((1, "node", sim.node_ids()[4]), 16) == sim.snapshot_topk((1, "node", 4), 16)
    assert names                                                            # ids resolve as in snapshot_groups


# ---- 2: values wider than one digit ------------------------------------------------------------------------
WIDE_TOP = "3\nN1 200000\nN2 110000\nN3 300\nN1 N2\nN2 N1\nN1 N3\nN3 N1\nN2 N3\nN3 N2\n"
WIDE_EVENTS = ("send N1 N2 60000\nsend N1 N3 257\nsend N2 N3 1\ntick 1\nsend N1 N2 3000\nsend N2 N1 65535\nsnapshot N3\n"
               "send N3 N1 5\nsend N1 N2 1\ntick 2\nsnapshot N1\nsend N2 N3 40000\ntick 1\n")
WIDE_TERMS = [(0, "inflight", None), (0, "node", 1), (0, "ch_tok", 2), (1, "inflight", None), tick(1)]


def test_values_wider_than_one_digit_both_layouts():
    rows, keys = scenario(WIDE_TOP, WIDE_EVENTS, N)
    assert (rows.status == O.OK).all() and rows.n_sids == 2 and rows.done[0].all() and rows.done[1].all()
    v = term_values(rows, keys, WIDE_TERMS[0])
    assert int(v.max()) - int(v.min()) >= 2**17 and np.unique(v).size >= 36   # three digits of 8 bits
    v = term_values(rows, keys, WIDE_TERMS[1])
    assert int(v.max()) - int(v.min()) >= 2**16 and np.unique(v).size >= 8
    assert set(np.unique(term_values(rows, keys, WIDE_TERMS[2])).tolist()) == {0, 65535}
    sim = make_sim(WIDE_TOP, WIDE_EVENTS, N, AUTO)
    both_layouts(sim, AUTO, lambda what: check(sim, rows, keys, WIDE_TERMS, RANGES, "wide " + what))


# ---- 3: ragged batches, block-major through the slot map -----------------------------------------------------
@pytest.mark.parametrize("engine", [AUTO, LANES], ids=["auto", "lanes"])
@pytest.mark.parametrize("n", [63, 65, 257])
def test_ragged_block_major(n, engine):
    rows, keys = scenario(C3_TOP, C3_EVENTS, n)
    sim, twin = blocked_ragged_sim(C3_TOP, C3_EVENTS, n, engine, fifo_lds_slots=SLOTS,
                                   want_engine=NODES if engine == AUTO else LANES)
    assert n % 64 != 0 and sim.records_blocked()
    terms = [tick(0), (4, "inflight", None)]
    check(sim, rows, keys, terms, ranges_of(n), f"ragged n = {n}", ks=lambda s: sorted({0, 1, 16, s, s + 5}))
    for term in terms:                                                      # the instance-major twin agrees
        assert sim.snapshot_topk(term, 16, True) == twin.snapshot_topk(term, 16, True)


# ---- 4: record shapes ----------------------------------------------------------------------------------------
def test_hub_three_word_records_both_layouts():
    rows, keys = scenario(HUB_TOP, HUB_EVENTS, N)
    assert (rows.status == O.OK).all() and rows.n_sids == 4
    sim = make_sim(HUB_TOP, HUB_EVENTS, N, AUTO)
    assert sim.num_nodes * 3 == 33                                          # 3-word records, 33 words: not staged
    terms = [(1, "node", 0), (3, "ch_msgs", 11), tick(2), (2, "inflight", None)]
    both_layouts(sim, AUTO, lambda what: check(sim, rows, keys, terms, RANGES, "hub " + what,
                                               ks=lambda s: sorted({0, 16, 1000, s})))


def test_ring17_two_chunks_of_whole_nodes():
    n = N_RING17
    rows, keys = scenario(RING17_TOP, RING17_EVENTS, n)
    assert (rows.status == O.OK).all() and rows.n_sids == 2
    sim, twin = blocked_ragged_sim(RING17_TOP, RING17_EVENTS, n, AUTO, fifo_lds_slots=SLOTS, want_engine=NODES)
    assert sim.num_nodes == 17 and sim.num_channels == 17                   # 34 record words
    terms = [(0, "node", 16), tick(1), (0, "ch_msgs", 15), (1, "inflight", None)]
    assert np.unique(term_values(rows, keys, terms[0])).size > 1
    for s, what in ((sim, "ring17 block-major"), (twin, "ring17 instance-major")):
        check(s, rows, keys, terms, [(0, n), (1, n - 1), (64, n)], what, ks=lambda s: sorted({0, 1, 16, s, s + 5}))


# ---- 5: subset samples ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def undrained_rows(n):
    return from_refs(undrained_refs(C3_TOP, UNDRAINED_EVENTS, n))


def test_subset_samples_and_conditional_forms():
    n = 257
    rows, keys = undrained_rows(n)
    done = [int(d.sum()) for d in rows.done]
    assert rows.n_sids == 5 and 0 < done[4] < done[3] < done[0] < n         # the snapshots complete in proper subsets
    sim = build_sim(C3_TOP, UNDRAINED_EVENTS, n, AUTO, drain=False)
    where = [("tick", None, 19, None)]
    mask = clause_mask(rows, keys, 0, where)
    both = int((mask & rows.done[4]).sum())
    assert 0 < both < int(mask.sum()) and both < done[4]                    # set & completed(4): proper subsets
    iset = sim.instance_set(0, where)                                       # executes the pending events, adds no tick
    assert len(iset) == int(mask.sum())
    terms = [tick(4), (4, "inflight", None), (3, "node", 2)]
    ranges = [(0, n), (3, 201), (64, 128)]
    small = lambda s: sorted({0, 1, 16, s, s + 5})  # noqa: E731
    check(sim, rows, keys, terms, ranges, "undrained")
    check(sim, rows, keys, terms, ranges, "undrained in set", iset=iset, mask=mask, ks=small)
    # a set holding the whole batch: byte for byte the unconditional call
    whole = sim.instance_set_from(np.arange(n))
    for term in terms:
        for lo, hi in ranges:
            for largest in (False, True):
                assert sim.snapshot_topk_in(whole, term, 16, largest, lo, hi) == sim.snapshot_topk(term, 16, largest, lo, hi)
            assert sim.snapshot_quantiles_in(whole, term, [0, 0.5, 1], lo, hi) == sim.snapshot_quantiles(term, [0, 0.5, 1], lo, hi)
            a, b = sim.snapshot_values_in(whole, term, lo, hi), sim.snapshot_values(term, lo, hi)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # an empty set, an empty range, a snapshot that completes nowhere
    empty = sim.instance_set_from(())
    none = np.zeros(n, dtype=bool)
    check(sim, rows, keys, terms[:1], [(0, n)], "empty set", iset=empty, mask=none, ks=small)
    check(sim, rows, keys, terms[:2], [(17, 17), (0, 0), (n, n)], "empty range", ks=small)
    got = sim.snapshot_topk_in(empty, tick(4), 16)
    assert (got.instances, got.ok, got.sample, got.n_returned) == (n, int((rows.status == O.OK).sum()), 0, 0)
    q = sim.snapshot_quantiles_in(empty, tick(4), [0.5, 1])
    assert q.ranks.tolist() == [-1, -1] and q.sample == 0
    fresh = make_sim(C3_TOP, None, 64, AUTO)
    assert fresh.StartSnapshot(fresh.node_ids()[0]) == 0                                 # started, never ticked: complete nowhere
    got = fresh.snapshot_topk(tick(0), 16)
    assert (got.instances, got.ok, got.sample, got.n_returned) == (64, 64, 0, 0)
    assert fresh.snapshot_quantiles(tick(0), [0.5]).ranks.tolist() == [-1]
    v, member = fresh.snapshot_values((0, "inflight", None))
    assert not v.any() and not member.any()


# ---- 6: the kernels over the whole int64 range ---------------------------------------------------------------
Q64 = [(j, 63) for j in range(64)]


def plane_check(vals, member, what, ks=None):
    vals = np.asarray(vals, dtype=np.int64)
    sample = vals.size if member is None else int(np.count_nonzero(member))
    for largest in (False, True):
        for k in sorted({0, 1, max(sample - 1, 0), sample, sample + 1} if ks is None else ks):
            if k > cl.ORDER_MAX_K:
                continue
            got = cl.order_plane_device(vals, member, k, largest, Q64)
            want = plane_expected(vals, member, k, largest, Q64)
            tag = f"{what} k {k} largest {largest}"
            assert got[0].size == min(k, sample), tag
            assert np.array_equal(got[0], want[0]), f"{tag}: instances"
            assert np.array_equal(got[1], want[1]), f"{tag}: values"
            assert np.array_equal(got[3], want[3]), f"{tag}: ranks"
            if sample:
                assert np.array_equal(got[2], want[2]), f"{tag}: quantile values"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000, 70000])
def test_plane_aid_against_numpy(n):
    rng = np.random.default_rng(20240 + n)
    full = rng.integers(I64.min, I64.max, n, endpoint=True)
    planted = [I64.min, -1, 0, 1, I64.max]
    full[rng.permutation(n)[:min(n, 5)]] = planted[:min(n, 5)]
    plane_check(full, None, f"n {n} full range")
    if n == 70000:
        plane_check(full, None, f"n {n} max k", ks=[cl.ORDER_MAX_K])
    half = rng.integers(0, 2, n).astype(bool)
    plane_check(full, half, f"n {n} half in sample")
    plane_check(full, np.zeros(n, dtype=bool), f"n {n} none in sample", ks=[0, 1, 5])
    # all values equal: k inside the tie gives the first k instances
    same = np.full(n, -12345, dtype=np.int64)
    plane_check(same, None, f"n {n} all equal", ks=[1, n // 2, n])
    got = cl.order_plane_device(same, None, max(n // 2, 1), True)
    assert got[0].tolist() == list(range(max(n // 2, 1)))
    # values that differ only in bit 0, and only in bit 63
    bit = rng.integers(0, 2, n)
    plane_check(1000 + bit, None, f"n {n} bit 0", ks=[1, n // 3, n])
    plane_check(np.where(bit == 1, np.int64(I64.min + 77), np.int64(77)), half, f"n {n} bit 63", ks=[1, n // 3, n])
    # few distinct values of small range: many ties, one digit pass
    plane_check(rng.integers(-3, 4, n), half, f"n {n} ties", ks=[1, 16, n // 2])


# ---- 7: composition: find the worst runs, look at them, replay them ------------------------------------------
def test_composition_latest_finishers():
    rows, keys = scenario(C3_TOP, C3_EVENTS, N)
    sim = make_sim(C3_TOP, C3_EVENTS, N, AUTO)
    sim.flush()
    top = sim.snapshot_topk(tick(0), 16, largest=True)
    assert_topk_equal(top, expected_topk(rows, keys, tick(0), 16, True, 0, N), 16, True, "latest finishers")
    for got, want in zip(top.collect(sim), sim.collect_snapshot_list(0, top.insts)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert top.collect(sim)[1].all()
    s = top.instance_set(sim)
    assert len(s) == 16 and np.array_equal(s.insts(), np.sort(top.insts))
    # re-run exactly those instances as their own batch: the same completion ticks
    again = make_sim(C3_TOP, C3_EVENTS, 16, AUTO)
    again.set_delay_go_seed_list(top.seeds(cl.REFERENCE_SEED))
    assert np.array_equal(again.snapshot_ticks(0), top.values)
    # sub-ranges merge into the whole, in both directions and for a record quantity
    for term in (tick(0), (0, "inflight", None)):
        for largest in (False, True):
            parts = sim.snapshot_topk(term, 16, largest, 0, 2000).merge(sim.snapshot_topk(term, 16, largest, 2000, N), offset=0)
            assert parts == sim.snapshot_topk(term, 16, largest), (term, largest)
    before = sim.device_bytes
    sim.snapshot_topk(tick(0), 4096)
    assert sim.device_bytes >= before > 0                                   # the scratch is counted
