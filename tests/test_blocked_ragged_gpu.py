"""Block-major snapshot records at ragged batch sizes, end to end: the writers of both exec kernels
and every reader, after a poisoned replay through the slot map.

A replay through the slot map writes the records block-major by slot, [S][I/64][N][64][rw], and
every reader then goes through the slot -> instance map.  The other suites pin the readers in that
layout at 4096 instances only, a whole number of 64-slot blocks.  Here the last block is partial
(slots at or past the batch hold poison), the last word of a `where` bitmap and of the select
bitmap is partial, and the node-parallel kernel's last wave is ragged.

Small cases: C3 (8nodes.top, 8nodes-concurrent-snapshots.events) at 63, 65, 130, 200 and 257
instances with 4 LDS ring slots per channel.  A few instances spill, so the plan splits the batch
and replays through the map (cl_plan.cpp plan_order: mapped = sort || split_slot > 0); the order
is "the clean instances, then the spillers", a shift that displaces every instance after the first
spiller.  test_blocked_ragged_host.py holds the oracle's prediction; blocked_ragged_sim() asserts
the regime on the device before anything is read.  The same program without its drain (snapshots
3 and 4 incomplete in some OK instances) makes the cross-snapshot conditioning a proper subset.

Sort-order cases at 4096 + 37 instances, the library's choice of kernel: the hub (3-word records,
33 record words: not staged, the multi-chunk statistics path), the three-node many-class scenario,
and C3 itself, where the clean instances go in length order -- a shuffle, not a shift.

Expected values come from the oracle (statscheck, censuscheck, selectcheck, crosstabcheck,
groupscheck, isetcheck, enginecheck); the flush-only, instance-major twin is a second comparison.
"""
import numpy as np
import pytest

import censuscheck
import oracle as O
import selectcheck
import statscheck
import test_crosstab_gpu as xt_tests
import test_groups_gpu as groups_tests
from blockedcheck import (AUTO, C3_EVENTS, C3_TOP, LANES, N_RING17, N_SORT, NODES, RING17_EVENTS, RING17_TOP, SLOTS,
                          SMALL_SIZES, UNDRAINED_EVENTS, blocked_ragged_sim, cl, replay_poisoned, undrained_refs)
from enginecheck import batch_sums_from_oracle, compare_instance, oracle_batch
from groupscheck import assert_groups_equal
from groupscheck import expected as groups_expected
from isetcheck import clause_mask, keys_in, list_mask, members, rows_in
from selectcheck import assert_selection_equal
from statscheck import assert_stats_equal
from test_census_gpu import EVENTS3, HUB_EVENTS, HUB_TOP, TOP3
from test_iset_gpu import check_in

pytestmark = pytest.mark.gpu

CLAMPING = dict(tick_lo=20, tick_bins=4, msg_bins=8)      # test_stats_gpu case 3
C3_PAIRS = xt_tests.C3_PAIRS                              # axes of snapshot ids 0 and 4, records and totals
C3_TERMS = [groups_tests.C3_TICKS2, groups_tests.C3_MIXED, [(0, "key", None), (4, "node", 3)]]
ENGINE_IDS = {AUTO: "auto", LANES: "lanes"}


def ranges_of(n):
    out = [(0, n), (1, n - 1), (n - 1, n), (0, 0), (n, n)]
    if n >= 65:
        out.append((63, 65))
    if n > 64:
        out.append((64, n))
    return out


class Case:
    """One (n, engine): the replayed sim, its flush-only twin and the oracle's rows."""

    def __init__(self, n, engine, drain=True):
        self.n, self.engine = n, engine
        if drain:
            self.rows, self.keys = selectcheck.scenario(C3_TOP, C3_EVENTS, n)
        else:
            self.rows, self.keys = selectcheck.from_refs(undrained_refs(C3_TOP, UNDRAINED_EVENTS, n))
        # at these sizes the library's choice is the node-parallel kernel
        self.sim, self.twin = blocked_ragged_sim(C3_TOP, C3_EVENTS if drain else UNDRAINED_EVENTS, n, engine,
                                                 fifo_lds_slots=SLOTS, want_engine=NODES if engine == AUTO else LANES,
                                                 drain=drain)
        self.what = f"n = {n} {ENGINE_IDS[engine]}"


def _id(p):
    return f"{p[0]}-{ENGINE_IDS[p[1]]}"


@pytest.fixture(scope="module", params=[(n, e) for n in SMALL_SIZES for e in (AUTO, LANES)], ids=_id)
def case(request):
    return Case(*request.param)


@pytest.fixture(scope="module", params=[(n, e) for n in (65, 257) for e in (AUTO, LANES)], ids=_id)
def loose(request):
    return Case(*request.param, drain=False)


def splitting_clause(rows, keys, sid, field, negate=False):
    """A clause on `field` of snapshot sid whose bound is the oracle's middle value, at the first
    node or channel whose values differ over the sample: it matches some of the sample, not all."""
    pick = np.flatnonzero(rows.done[sid])
    width = {"node": rows.node[sid].shape[1], "ch_msgs": rows.ch_msgs[sid].shape[1],
             "ch_tok": rows.ch_tok[sid].shape[1]}.get(field)
    for index in [None] if width is None else range(width):
        u = np.unique(selectcheck.values(rows, keys, sid, field, 0 if index is None else index)[pick])
        if u.size >= 2:
            clause = (field, index, None, int(u[(u.size - 1) // 2]))
            return clause + ("not",) if negate else clause
    raise AssertionError(f"no {field} of snapshot {sid} varies over the sample")


# ---- the writers ----------------------------------------------------------------------------------
def check_writer(c, batch):
    sim, twin, n = c.sim, c.twin, c.n
    _, want_status, want_ticks, counters, want_hashes = batch
    ok = want_status == O.OK
    status, times = sim.status(), sim.time()
    assert np.array_equal(status, want_status) and np.array_equal(status, twin.status())
    assert np.array_equal(times[ok], want_ticks[ok]) and np.array_equal(times, twin.time())
    sums = dict(zip(cl.SUM_NAMES, sim.checksums().tolist()))
    for k, v in batch_sums_from_oracle(want_status, counters, want_hashes).items():
        assert sums[k] == v, f"{c.what} {k}: engine {sums[k]} vs oracle {v}"
    assert np.array_equal(sim.checksums(), twin.checksums())
    got, got_ok = sim.counters(), sim.counters(only_ok=True)
    assert got == twin.counters() and got_ok == twin.counters(only_ok=True)
    for k, name in enumerate(("push", "peek", "pop_tok", "pop_mk")):
        assert got[name] == counters[:, k].sum(), f"{c.what} {name}"
    assert got["ticks"] == want_ticks.sum()
    assert got_ok["recorded"] == counters[ok, 4].sum() and got_ok["completed"] == counters[ok, 6].sum()
    hashes = sim.instance_hashes()
    assert np.array_equal(hashes[ok], want_hashes[ok]) and np.array_equal(hashes, twin.instance_hashes())
    for sid in range(c.rows.n_sids):
        for lo, hi in ((0, n), (n - 1, n), (37, n)):
            for g, w in zip(sim.collect_snapshot_packed(sid, lo, hi), twin.collect_snapshot_packed(sid, lo, hi)):
                assert g.dtype == w.dtype and np.array_equal(g, w), f"{c.what} packed sid {sid} [{lo}, {hi})"
    for i in sorted({0, 33, 34, 35, 63, 64, n - 2, n - 1} & set(range(n))):
        compare_instance(sim, i, c.keys.refs[i], status=status, times=times)


def test_writer_after_poisoned_mapped_replays(case):
    batch = oracle_batch(C3_TOP, C3_EVENTS, case.n)
    assert (batch[1] != O.OK).any() and (batch[1] == O.OK).any()
    check_writer(case, batch)
    before = case.sim.replay_split()
    replay_poisoned(case.sim)                             # the second replay of the same plan
    assert case.sim.mapped_replays() and case.sim.records_blocked() and case.sim.replay_split() == before
    check_writer(case, batch)


# ---- statistics -----------------------------------------------------------------------------------
def check_stats(c, sids=None):
    sim, rows, n = c.sim, c.rows, c.n
    for spec in ({}, CLAMPING):
        layout = sim.stats_layout(**spec)
        for sid in range(rows.n_sids) if sids is None else sids:
            for lo, hi in ranges_of(n):
                st = sim.snapshot_stats(sid, lo, hi, **spec)
                assert st.layout == layout
                assert_stats_equal(st.raw, statscheck.expected(layout, rows, sid, lo, hi), layout,
                                   f"{c.what} sid {sid} [{lo}, {hi}) {spec}")
            whole = sim.snapshot_stats(sid, 0, n, **spec)
            assert whole == c.twin.snapshot_stats(sid, 0, n, **spec)
            for a in [1] + ([64] if n > 64 else []) + [n - 1]:
                parts = sim.snapshot_stats(sid, 0, a, **spec).merge(sim.snapshot_stats(sid, a, n, **spec))
                assert_stats_equal(parts.raw, whole.raw, layout, f"{c.what} sid {sid} merge at {a}")


def test_statistics(case):
    t0 = case.rows.tick[0][case.rows.done[0]]
    assert t0.min() < 20 and t0.max() >= 23               # both tick clamps of the clamping spec are hit
    check_stats(case)


# ---- census -----------------------------------------------------------------------------------------
def check_census(c, what=""):
    sim, keys, n = c.sim, c.keys, c.n
    for sid in range(keys.n_sids):
        for lo, hi in ranges_of(n):
            want = censuscheck.expected(keys, sid, lo, hi)
            tag = f"{c.what} {what} sid {sid} [{lo}, {hi})"
            ref = sim.snapshot_census(sid, lo, hi, class_of=True, lds_slots=0)
            censuscheck.assert_census_equal(ref, want, tag)
            for s in (16, -1):
                got = sim.snapshot_census(sid, lo, hi, class_of=True, lds_slots=s)
                assert got.classes.tobytes() == ref.classes.tobytes(), f"{tag} lds_slots {s}"
                assert got.class_of.tobytes() == ref.class_of.tobytes(), f"{tag} lds_slots {s}"
        want = censuscheck.expected(keys, sid, 0, n)
        for cut in (0, 2):
            got = sim.snapshot_census(sid, max_classes=cut, class_of=True)
            assert (got.n_returned, got.n_classes) == (min(cut, want[0][3]), want[0][3])
            censuscheck.assert_census_equal(got, want, f"{c.what} {what} sid {sid} cut {cut}", max_classes=cut)


def test_census(case):
    whole = [censuscheck.expected(case.keys, sid, 0, case.n) for sid in range(5)]
    assert any(w[0][3] > 2 for w in whole)                # class_of names classes beyond a cut of 2
    check_census(case)


# ---- select -----------------------------------------------------------------------------------------
def test_select(case):
    sim, rows, keys, n = case.sim, case.rows, case.keys, case.n
    wheres = [[]] + [[splitting_clause(rows, keys, 0, f)] for f in cl.SELECT_FIELDS]
    wheres.append([splitting_clause(rows, keys, 0, "node", negate=True)])
    wheres.append([splitting_clause(rows, keys, 0, "tick"), splitting_clause(rows, keys, 0, "key", negate=True)])
    sample = int(rows.done[0].sum())
    for where in wheres[1:-1]:
        assert 0 < selectcheck.expected(rows, keys, 0, 0, n, where)[0][3] < sample, where
    for lo, hi in ranges_of(n):
        for where in wheres:
            want = selectcheck.expected(rows, keys, 0, lo, hi, where)
            tag = f"{case.what} [{lo}, {hi}) where {where}"
            got = sim.select_instances(0, where, lo, hi, ticks=True)
            assert_selection_equal(got, want, tag)
            assert (np.diff(got.insts) > 0).all() and (got.insts.size == 0 or got.insts[-1] < n), tag
            plain = sim.select_instances(0, where, lo, hi)
            assert plain.ticks is None
            assert_selection_equal(plain, want, tag)
            for cap in (0, 1, n):
                assert_selection_equal(sim.select_instances(0, where, lo, hi, max_out=cap, ticks=True), want,
                                       f"{tag} max_out {cap}", max_out=cap)
    for sid in range(1, 5):
        where = [splitting_clause(rows, keys, sid, "tick")]
        for lo, hi in ((0, n), (37, n)):
            for w in ([], where):
                assert_selection_equal(sim.select_instances(sid, w, lo, hi, ticks=True),
                                       selectcheck.expected(rows, keys, sid, lo, hi, w), f"{case.what} sid {sid} {w}")
    want_ticks = np.where(rows.done[4], rows.tick[4], -1).astype(np.int32)
    assert np.array_equal(sim.snapshot_ticks(4), want_ticks)


# ---- instance sets and the conditional calls ------------------------------------------------------------
def check_sets(c, sids):
    sim, rows, keys, n = c.sim, c.rows, c.keys, c.n
    wa, wb = [splitting_clause(rows, keys, 0, "tick")], [splitting_clause(rows, keys, 0, "node", negate=True)]
    ma, mb = clause_mask(rows, keys, 0, wa), clause_mask(rows, keys, 0, wb)
    assert ma.any() and mb.any() and (ma != mb).any()
    assert sim.records_blocked()                          # the sets are built on the block-major records
    a, b = sim.instance_set(0, wa), sim.instance_set(0, wb)
    assert a.info == selectcheck.expected(rows, keys, 0, 0, n, wa)[0]
    part = sim.instance_set(0, wa, 37, n)                 # a set over a sub-range: matches of that range only
    mpart = clause_mask(rows, keys, 0, wa, 37, n)
    la, lb = np.arange(0, n, 3), np.array([n - 1, 0, n - 1] + list(range(n // 2, n)))
    mla, mlb = list_mask(n, la), list_mask(n, lb)
    sa, sb = sim.instance_set_from(la), sim.instance_set_from(lb)
    sample, ms = sim.instance_set(0, []), rows.done[0]
    sets = [("a", a, ma), ("b", b, mb), ("part", part, mpart), ("a & b", a & b, ma & mb), ("a | b", a | b, ma | mb),
            ("a - b", a - b, ma & ~mb), ("la", sa, mla), ("la | lb", sa | sb, mla | mlb), ("la - lb", sa - sb, mla & ~mlb),
            ("lb - la", sb - sa, mlb & ~mla), ("sample", sample, ms), ("la - sample", sa - sample, mla & ~ms),
            ("(la | lb) - (la & lb)", (sa | sb) - (sa & sb), mla ^ mlb)]
    for name, iset, mask in sets:
        got = iset.insts()
        tag = f"{c.what} {name}"
        assert len(iset) == int(mask.sum()) <= n and np.array_equal(got, members(mask)), tag
        assert got.size == 0 or got[-1] < n, tag
        for lo, hi in ranges_of(n):
            assert iset.count(lo, hi) == int(mask[lo:hi].sum()), f"{tag} count [{lo}, {hi})"
            assert np.array_equal(iset.insts(lo, hi), members(mask, lo, hi)), f"{tag} insts [{lo}, {hi})"
    assert len(sb) == n - n // 2 + 1 and sb.count(n - 1, n) == 1   # the duplicates of n - 1 count once
    whole = (sa | sb) | sim.instance_set_from(np.arange(n))
    assert len(whole) == n
    ranges = [(0, n), (37, n), (n - 1, n)]
    for name, iset, mask in (sets[0], sets[2], sets[5], sets[7], ("whole", whole, np.ones(n, dtype=bool))):
        for sid in sids:
            tag = f"{c.what} set {name}"
            check_in(sim, rows, keys, mask, iset, sid, ranges, tag,
                     wheres=[[], [("msgs", None, 1, None)]], spec=CLAMPING)
        xt_tests.check(sim, rows, keys, C3_PAIRS, ranges, f"{c.what} set {name}", iset=iset, mask=mask)
        groups_tests.check(sim, rows, keys, C3_TERMS, ranges, f"{c.what} set {name}", iset=iset, mask=mask)
    for sid in sids:                                      # the whole batch as the set: the unconditional bytes
        assert (sim.snapshot_stats_in(sid, whole, **CLAMPING).raw.tobytes()
                == sim.snapshot_stats(sid, **CLAMPING).raw.tobytes())
        assert sim.select_instances_in(sid, whole, ticks=True) == sim.select_instances(sid, ticks=True)


def test_instance_sets_and_conditional_calls(case):
    check_sets(case, (3, 4))


# ---- crosstab and group-by -------------------------------------------------------------------------------
def check_groups(c, what=""):
    sim, rows, keys, n = c.sim, c.rows, c.keys, c.n
    for terms in C3_TERMS:
        for lo, hi in ranges_of(n):
            want = groups_expected(rows, keys, terms, lo, hi)
            tag = f"{c.what} {what} {terms} [{lo}, {hi})"
            ref = sim.snapshot_groups(terms, lo, hi, group_of=True, lds_slots=0)
            assert_groups_equal(ref, want, tag)
            for s in (16, -1):
                got = sim.snapshot_groups(terms, lo, hi, group_of=True, lds_slots=s)
                assert got.groups.tobytes() == ref.groups.tobytes() and got.values.tobytes() == ref.values.tobytes(), tag
                assert got.group_of.tobytes() == ref.group_of.tobytes(), f"{tag} lds_slots {s}"
        want = groups_expected(rows, keys, terms, 0, n)
        for cut in (0, 2):
            got = sim.snapshot_groups(terms, max_groups=cut, group_of=True)
            assert (got.n_returned, got.n_groups) == (min(cut, want[0][3]), want[0][3])
            assert_groups_equal(got, want, f"{c.what} {what} {terms} cut {cut}", max_groups=cut)


def test_crosstab_and_groups(case):
    sim, rows, keys, n = case.sim, case.rows, case.keys, case.n
    xt_tests.check(sim, rows, keys, C3_PAIRS, ranges_of(n), case.what)
    assert all(groups_expected(rows, keys, t, 0, n)[0][3] > 2 for t in C3_TERMS)   # group_of beyond a cut of 2
    check_groups(case)
    for terms in C3_TERMS:
        g = sim.snapshot_groups(terms)
        for k in sorted({0, 1, g.n_returned - 1}):
            iset = g.instance_set(sim, k)
            assert len(iset) == int(g.groups["count"][k]), f"{case.what} {terms} group {k}"
            assert iset.insts()[0] == g.groups["first_inst"][k] and iset.insts()[-1] < n


def test_key_equal_to_the_empty_marker(case, monkeypatch):
    """The table's empty marker moved onto the key of the largest class (test_census_gpu,
    test_groups_gpu): that class goes through the extra entry and nothing changes."""
    want = censuscheck.expected(case.keys, 0, 0, case.n)
    monkeypatch.setenv("CLSNAP_CENSUS_EMPTY_KEY", str(int(want[1]["key"][0])))
    check_census(case, "marker on the largest class")
    want = groups_expected(case.rows, case.keys, C3_TERMS[0], 0, case.n)
    monkeypatch.setenv("CLSNAP_CENSUS_EMPTY_KEY", str(int(want[1]["key"][0])))
    check_groups(case, "marker on the largest group")


# ---- the same program without its drain: snapshots 3 and 4 incomplete in some OK instances ------------------
def test_undrained_cross_snapshot_conditioning(loose):
    c, n = loose, loose.n
    ok = int((c.rows.status == O.OK).sum())
    assert all(0 < int(c.rows.done[sid].sum()) < ok for sid in (3, 4))
    assert np.array_equal(c.sim.status(), c.rows.status) and np.array_equal(c.sim.status(), c.twin.status())
    assert np.array_equal(c.sim.instance_hashes(), c.twin.instance_hashes())
    for sid in range(5):
        for g, w in zip(c.sim.collect_snapshot_packed(sid, 0, n), c.twin.collect_snapshot_packed(sid, 0, n)):
            assert np.array_equal(g, w)
        assert np.array_equal(c.sim.snapshot_ticks(sid), np.where(c.rows.done[sid], c.rows.tick[sid], -1))
    check_stats(c, sids=(0, 3, 4))
    check_census(c)
    check_groups(c)
    check_sets(c, (3, 4))


# ---- records longer than a staging chunk, an even record size: two chunks, the last of one node ---------------
def test_ring_of_17_two_chunks_of_whole_nodes():
    """34 record words of 2-word records: the statistics stage 16 nodes and then R16 alone, whose rows
    of 2 words sit at the odd pitch 3 (the hub's single-node chunk has rows of 3 words at pitch 3,
    where a row pitch of kw goes unnoticed); census, select and group-by read the plane word by word.
    17 nodes are one more than the instance-per-lane kernel takes: the node-parallel kernel only,
    3 instances per wave."""
    n = N_RING17
    sim, twin = blocked_ragged_sim(RING17_TOP, RING17_EVENTS, n, AUTO, fifo_lds_slots=SLOTS, want_engine=NODES)
    assert sim.num_nodes == 17 and sim.num_channels == 17
    rows, keys = selectcheck.scenario(RING17_TOP, RING17_EVENTS, n)
    assert (rows.status == O.OK).all() and rows.n_sids == 2
    assert np.array_equal(sim.instance_hashes(), twin.instance_hashes())
    spec = dict(tick_lo=40, tick_bins=16, msg_bins=2)
    where = [splitting_clause(rows, keys, 0, "node", negate=True)]
    terms = [(0, "node", 16), (1, "tick", None), (0, "ch_msgs", 15)]
    for sid in range(2):
        for kw in ({}, spec):
            layout = sim.stats_layout(**kw)
            for lo, hi in ranges_of(n):
                assert_stats_equal(sim.snapshot_stats(sid, lo, hi, **kw).raw, statscheck.expected(layout, rows, sid, lo, hi),
                                   layout, f"ring of 17 sid {sid} [{lo}, {hi}) {kw}")
            parts = sim.snapshot_stats(sid, 0, 64, **kw).merge(sim.snapshot_stats(sid, 64, n, **kw))
            assert parts == sim.snapshot_stats(sid, **kw) == twin.snapshot_stats(sid, **kw)
        for lo, hi in ranges_of(n):
            tag = f"ring of 17 sid {sid} [{lo}, {hi})"
            censuscheck.assert_census_equal(sim.snapshot_census(sid, lo, hi, class_of=True),
                                            censuscheck.expected(keys, sid, lo, hi), tag)
            for w in ([], where, [("ch_tok", 15, 1, 3), ("node", 16, 8, 8)]):
                assert_selection_equal(sim.select_instances(sid, w, lo, hi, ticks=True),
                                       selectcheck.expected(rows, keys, sid, lo, hi, w), f"{tag} {w}")
            for g, w in zip(sim.collect_snapshot_packed(sid, lo, hi), twin.collect_snapshot_packed(sid, lo, hi)):
                assert np.array_equal(g, w), tag
    groups_tests.check(sim, rows, keys, [terms], ranges_of(n), "ring of 17")
    xt_tests.check(sim, rows, keys, [((0, "node", 16, 8, 1, 4), (1, "tick", None, 40, 2, 16))], ranges_of(n), "ring of 17")


# ---- 4096 + 37 instances: mapped by the length sort ---------------------------------------------------------
SORT_RANGES = [(0, N_SORT), (37, 3001), (4096, N_SORT), (N_SORT - 1, N_SORT)]


def sorted_sim(top, events):
    """4096 + 37 instances on the library's choice of kernel, mapped by the length sort (no split is asked for)."""
    return blocked_ragged_sim(top, events, N_SORT, AUTO, split=False)


def test_hub_three_word_records_sort_order():
    n = N_SORT
    sim, twin = sorted_sim(HUB_TOP, HUB_EVENTS)
    assert sim.num_nodes * 3 == 33        # 33 record words: not staged, whole-node chunks
    rows, keys = selectcheck.scenario(HUB_TOP, HUB_EVENTS, n)
    assert (rows.status == O.OK).all() and rows.n_sids == 4
    assert np.array_equal(sim.instance_hashes(), twin.instance_hashes())
    layout = sim.stats_layout()
    for sid in range(4):
        wheres = [[splitting_clause(rows, keys, sid, "node")], [splitting_clause(rows, keys, sid, "ch_tok")], []]
        for lo, hi in SORT_RANGES:
            tag = f"hub sid {sid} [{lo}, {hi})"
            assert_stats_equal(sim.snapshot_stats(sid, lo, hi).raw, statscheck.expected(layout, rows, sid, lo, hi),
                               layout, tag)
            censuscheck.assert_census_equal(sim.snapshot_census(sid, lo, hi, class_of=True),
                                            censuscheck.expected(keys, sid, lo, hi), tag)
            for where in wheres:
                assert_selection_equal(sim.select_instances(sid, where, lo, hi, ticks=True),
                                       selectcheck.expected(rows, keys, sid, lo, hi, where), f"{tag} {where}")
            for g, w in zip(sim.collect_snapshot_packed(sid, lo, hi), twin.collect_snapshot_packed(sid, lo, hi)):
                assert np.array_equal(g, w), tag
    groups_tests.check(sim, rows, keys, groups_tests.HUB_LISTS, SORT_RANGES, "hub")


def test_three_nodes_many_classes_sort_order():
    n = N_SORT
    sim, twin = sorted_sim(TOP3, EVENTS3)
    rows, keys = selectcheck.scenario(TOP3, EVENTS3, n)
    want = censuscheck.expected(keys, 0, 0, n)
    assert want[0][3] == 413                              # as at 4096 (test_blocked_ragged_host re-measures it)
    cut = [sim.snapshot_census(0, max_classes=16, class_of=True, lds_slots=s) for s in (0, 16, -1, 64)]
    for c in cut:
        assert (c.n_returned, c.n_classes) == (16, 413) and int(c.class_of.max()) > 15
        censuscheck.assert_census_equal(c, want, "cut", max_classes=16)
        assert c.classes.tobytes() == cut[0].classes.tobytes() and c.class_of.tobytes() == cut[0].class_of.tobytes()
    layout = sim.stats_layout(**CLAMPING)
    for sid in range(2):
        for lo, hi in SORT_RANGES:
            tag = f"three nodes sid {sid} [{lo}, {hi})"
            assert_stats_equal(sim.snapshot_stats(sid, lo, hi, **CLAMPING).raw,
                               statscheck.expected(layout, rows, sid, lo, hi), layout, tag)
            censuscheck.assert_census_equal(sim.snapshot_census(sid, lo, hi, class_of=True),
                                            censuscheck.expected(keys, sid, lo, hi), tag)
    groups_tests.check(sim, rows, keys, [groups_tests.TOP3_TOK_TICK], SORT_RANGES, "three nodes")
    assert np.array_equal(sim.instance_hashes(), twin.instance_hashes())


def test_c3_length_sorted_order():
    """C3 at 4096 + 37: some instances spill and the rest go in length order -- the one scenario here
    whose slot order is a shuffle (the hub's and the three-node scenario's instances all spill at the
    library's ring size, and "the spillers in index order" is the identity)."""
    n = N_SORT
    sim, twin = blocked_ragged_sim(C3_TOP, C3_EVENTS, n, AUTO)
    spilled, split = sim.replay_split()
    assert 0 < spilled < n // 4 and 0 < split < n
    rows, keys = selectcheck.scenario(C3_TOP, C3_EVENTS, n)
    clean = np.flatnonzero(rows.status == O.OK)
    ticks = np.array([keys.refs[i].time for i in clean])
    assert (np.diff(ticks) > 0).any() and (np.diff(ticks) < 0).any()   # lengths not monotone: the sort moves them
    assert np.array_equal(sim.instance_hashes(), twin.instance_hashes())
    layout = sim.stats_layout(**CLAMPING)
    where = [("tick", None, 19, 24), ("node", 4, 1, 4, "not")]
    iset, mask = sim.instance_set(0, where), clause_mask(rows, keys, 0, where)
    assert np.array_equal(iset.insts(), members(mask))
    for lo, hi in SORT_RANGES:
        for sid in (0, 4):
            tag = f"C3 sid {sid} [{lo}, {hi})"
            assert_stats_equal(sim.snapshot_stats(sid, lo, hi, **CLAMPING).raw,
                               statscheck.expected(layout, rows, sid, lo, hi), layout, tag)
            censuscheck.assert_census_equal(sim.snapshot_census(sid, lo, hi, class_of=True),
                                            censuscheck.expected(keys, sid, lo, hi), tag)
            assert_selection_equal(sim.select_instances(sid, where[:1], lo, hi, ticks=True),
                                   selectcheck.expected(rows, keys, sid, lo, hi, where[:1]), tag)
            assert_stats_equal(sim.snapshot_stats_in(sid, iset, lo, hi, **CLAMPING).raw,
                               statscheck.expected(layout, rows_in(rows, mask), sid, lo, hi), layout, tag + " in the set")
            censuscheck.assert_census_equal(sim.snapshot_census_in(sid, iset, lo, hi, class_of=True),
                                            censuscheck.expected(keys_in(keys, mask), sid, lo, hi), tag + " in the set")
        for g, w in zip(sim.collect_snapshot_packed(4, lo, hi), twin.collect_snapshot_packed(4, lo, hi)):
            assert np.array_equal(g, w)
    xt_tests.check(sim, rows, keys, C3_PAIRS[:1] + C3_PAIRS[3:], SORT_RANGES, "C3")
    groups_tests.check(sim, rows, keys, C3_TERMS, SORT_RANGES, "C3")


# ---- what never gets block-major records ---------------------------------------------------------------------
def _never_mapped(top, events):
    sim = cl.ChandyLamportSim(N_SORT)
    sim.read_topology_text(top)
    sim.read_events_text(events)
    sim.flush()
    replay_poisoned(sim)
    return sim


def test_long_records_and_the_multi_pass_statistics_stay_instance_major():
    """Two arms of the readers that no batch reaches in block-major layout (asserted, so that a planner
    that starts mapping them fails here and the arms get their cases): records of more than 32 words
    (the piece-chunk arm of stage_rows<true, E>) need 33 nodes and more, one instance per wave, where the
    length sort gains nothing and the layout is not specialized; so with the 24-node complete digraph of
    the multi-pass statistics."""
    leaves = 35
    ids = [f"L{k:02d}" for k in range(leaves)]
    star = (f"{leaves + 1}\nH 9\n" + "".join(f"{x} 6\n" for x in ids) + "".join(f"{x} H\n" for x in ids)
            + "".join(f"H {x}\n" for x in ids))
    star_events = ("".join(f"send {x} H {1 + k % 3}\n" for k, x in enumerate(ids)) + "send H L00 2\nsnapshot L01\n"
                   + "".join(f"send {x} H 1\n" for x in ids[::2]) + "tick 1\nsnapshot H\n"
                   + "".join(f"send {x} H 2\n" for x in ids[1::2]) + "send H L02 1\ntick 2\n")
    sim = _never_mapped(star, star_events)
    assert not sim.mapped_replays() and not sim.records_blocked()
    ids = [f"N{v:02d}" for v in range(24)]
    top = "24\n" + "".join(f"{x} 100\n" for x in ids) + "".join(f"{a} {b}\n" for a in ids for b in ids if a != b)
    events = ("send N00 N01 3\nsend N05 N02 1\nsnapshot N03\nsend N01 N00 2\ntick 1\n"
              "send N10 N11 4\nsnapshot N20\nsend N02 N05 1\ntick 2\n")
    sim = _never_mapped(top, events)
    assert sim.num_channels == 552 and not sim.mapped_replays() and not sim.records_blocked()
