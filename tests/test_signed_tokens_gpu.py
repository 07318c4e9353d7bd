"""The batch engine and its analytics at the ends of the int32 token range, against the oracle.

signedcheck's scenarios hold node words at INT32_MIN, within 2^18 of INT32_MAX and at INT32_MAX,
with mixed statuses; over a batch the true sum of squares of a node passes 2^64 and the sum of
products of two nodes passes 2^63 in magnitude.  Device code that zero-extended a node word or
accumulated it at 32 bits would differ from the oracle in every test here: the exec kernels'
signed balance check and record writers, the checksums' snapshot key and residuals, the trace's
token column, the statistics' moments, the census key, select and instance-set clauses, the
crosstab's bins and sum of products, the group key, and the order key's sign flip.

Everything compares exactly, over every instance of every range; the expected values are those of
statscheck, censuscheck, selectcheck, isetcheck, crosstabcheck, groupscheck, ordercheck and
enginecheck over one OracleSim per instance.  signedcheck.signed(), maxed(), debt() assert on the oracle
rows that the regime is reached before anything runs.

Engines: the library's choice (AUTO) runs SIGNED and MAXED on the node-parallel kernel -- with
payloads of 65,535 nothing else can.  The instance-per-lane kernel admits payloads below 128 only,
so where ENGINE_LANES is forced the programs are SIGNED_LANES and MAXED_LANES, the same events with
payloads below 128 that reach the same ends of int32 (signedcheck); that SIGNED itself is refused
there is asserted once.  DEBT, a send from a node whose balance is negative, runs on both kernels.
Layouts: instance-major after flush(), block-major by slot after rerun() of a mapped plan, at 4096
instances and at ragged sizes through the spill split.
"""
import importlib

import numpy as np
import pytest

import oracle as O
import selectcheck
from blockedcheck import NODES, SLOTS, blocked_ragged_sim
from crosstabcheck import XT_SUM_AA, XT_SUM_AB, assert_crosstab_equal
from crosstabcheck import expected as crosstab_expected
from enginecheck import batch_sums_from_oracle, compare_instance, oracle_batch
from groupscheck import assert_groups_equal
from groupscheck import expected as groups_expected
from isetcheck import clause_mask, members
from ordercheck import assert_topk_equal, expected_topk, term_values
from selectcheck import assert_selection_equal
from signedcheck import (DEBT_EVENTS, DEBT_TOP, I64_MIN, INT32_MAX, INT32_MIN, N1, N2, N3, debt, maxed, maxed_texts,
                         signed, signed_texts, true_sum)
from test_blocked_ragged_gpu import ranges_of
from test_census_gpu import AUTO, ENGINES, LANES, flush_on, make_sim, replay_blocked
from test_census_gpu import check as census_check
from test_iset_gpu import check_in
from test_order_gpu import check as order_check
from test_stats_gpu import check as stats_check
from test_trace_gpu import check_instances, oracle_log, traced_run

cl = importlib.import_module("chandy-lamport-distributed-snapshot-algorithm_amd")
pytestmark = pytest.mark.gpu

N = 4096                        # the smallest batch that gets a mapped block-major replay
RANGES = [(0, N), (37, 3001)]
SMALL = 257
TOP = 2**31 - 2**18             # signedcheck: N1 stays above this


def used_engine(engine):
    """The exec kernel a launch of these scenarios must have used."""
    return NODES if engine == AUTO else LANES


# ---- the exec kernels, instance by instance ------------------------------------------------------------------
def run_and_compare(top, events, rows_keys, n, engine):
    _, keys = rows_keys
    sim = make_sim(top, events, n, engine)
    sim.flush()
    assert sim.exec_engine() == used_engine(engine)
    status, times = sim.status(), sim.time()
    for i in range(n):
        compare_instance(sim, i, keys.refs[i], status=status, times=times)
    return sim


@ENGINES
def test_signed_every_instance(engine):
    lanes = engine == LANES
    run_and_compare(*signed_texts(lanes), signed(SMALL, lanes), SMALL, engine)


@ENGINES
def test_maxed_every_instance(engine):
    lanes = engine == LANES
    run_and_compare(*maxed_texts(lanes), maxed(SMALL, lanes), SMALL, engine)


@ENGINES
def test_send_from_a_node_in_debt(engine):
    """A send of 0 tokens from a balance of -3 is fatal (-3 < 0): the balance check is signed."""
    sim = run_and_compare(DEBT_TOP, DEBT_EVENTS, debt(SMALL), SMALL, engine)
    rows, _ = debt(SMALL)
    assert np.array_equal(sim.status(), rows.status)
    stats_check(sim, rows, [(0, SMALL)], "debt")


def test_forced_lanes_refuses_the_wide_payloads():
    for top, events in (signed_texts(), maxed_texts()):
        sim = make_sim(top, events, 64, LANES)
        with pytest.raises(cl.ClSnapError) as e:
            sim.flush()
        assert e.value.code == cl.E_LIMIT


# ---- the trace's token column ----------------------------------------------------------------------------------
def test_trace_token_column():
    n = 64
    top, events = signed_texts()
    balances = np.array([rec[5] for i in range(n) for rec in oracle_log(top, events, O.REFERENCE_SEED + i).log()])
    assert int(balances.min()) == INT32_MIN and int(balances.max()) > TOP     # what the column must carry
    assert ((balances < 0) & (balances > INT32_MIN)).any()
    sim = traced_run(top, events, n, n)
    check_instances(sim, top, events, n)


# ---- SIGNED at 4096 instances: one flushed sim and one replayed sim per engine ------------------------------
class Batch:
    def __init__(self, engine):
        self.engine, self.lanes = engine, engine == LANES
        self.top, self.events = signed_texts(self.lanes)
        self.rows, self.keys = signed(N, self.lanes)
        self.ok = self.rows.status == O.OK
        self.sims = []
        for what in ("instance-major", "block-major"):
            sim = make_sim(self.top, self.events, N, engine)
            flush_on(sim, engine)
            assert sim.exec_engine() == used_engine(engine) and not sim.records_blocked()
            if what == "block-major":
                replay_blocked(sim)
            self.sims.append((what, sim))
        # the least N1 of snapshot 0: the `lo` of a width-1 axis
        self.n1_min = int(self.rows.node[0][self.ok, N1].min())
        assert self.lanes or self.n1_min == 2147291207

    def each(self, body):
        for what, sim in self.sims:
            body(sim, what)


@pytest.fixture(scope="module", params=[AUTO, LANES], ids=["auto", "lanes"])
def batch(request):
    return Batch(request.param)


def test_batch_sums_and_conservation(batch):
    _, status, ticks, counters, hashes = oracle_batch(batch.top, batch.events, N)
    assert np.array_equal(status, batch.rows.status)
    want = batch_sums_from_oracle(status, counters, hashes)

    def body(sim, what):
        assert np.array_equal(sim.status(), status), what
        assert np.array_equal(sim.time()[batch.ok], ticks[batch.ok]), what
        sums = dict(zip(cl.SUM_NAMES, sim.checksums().tolist()))
        for k, v in want.items():
            assert sums[k] == v, f"{what} {k}: engine {sums[k]} vs oracle {v}"
        assert sums["cut_residual"] == 0 and sums["final_residual"] == 0, what    # the total is -1
        assert np.array_equal(sim.instance_hashes()[batch.ok], hashes[batch.ok]), what

    batch.each(body)


def test_statistics_every_word(batch):
    rows = batch.rows
    sq = [true_sum(rows.node[sid][batch.ok, N2]) for sid in range(3)]
    assert min(sq) >= 2**64                                                 # node_sumsq wraps
    batch.each(lambda sim, what: stats_check(sim, rows, RANGES, what))
    st = batch.sims[0][1].snapshot_stats(2)
    assert int(st.node_sumsq[N2]) % 2**64 == sq[2] % 2**64
    assert st.min_node[N2] == INT32_MIN and st.max_node[N1] > TOP and st.node_sum[N2] < -2**32


def test_census(batch):
    batch.each(lambda sim, what: census_check(sim, batch.keys, RANGES, what))


def signed_wheres(b):
    """Clauses on node words of snapshot 2 whose bounds straddle zero and sit at the ends of int32."""
    mid = int(np.median(b.rows.node[2][b.ok, N2]))
    return [
        [("node", N2, INT32_MIN, INT32_MIN)],
        [("node", N2, INT32_MIN + 1, None)],
        [("node", N2, None, INT32_MIN)],
        [("node", N2, INT32_MIN, INT32_MIN, "not")],
        [("node", N2, None, mid)],
        [("node", N2, -5, 5)],
        [("node", N2, -5, 5, "not")],
        [("node", N2, None, 0), ("node", N1, 0, INT32_MAX)],
        [("node", N2, None, -1), ("node", N1, 1, None), ("node", N3, -1, 1, "not")],
        [("node", N1, None, -1)],
        [("node", N1, TOP, INT32_MAX), ("node", N2, INT32_MIN + 1, -1)],
        [("node", N1, INT32_MAX, INT32_MAX, "not"), ("node", N2, 0, INT32_MAX, "not")],
    ]


def matches(b, where, sid=2):
    return selectcheck.expected(b.rows, b.keys, sid, 0, N, where)[0][3]


def test_select_on_node_words(batch):
    b = batch
    wheres = signed_wheres(b)
    sample = int(b.ok.sum())
    at_min = int((b.rows.node[2][b.ok, N2] == INT32_MIN).sum())
    assert 0 < at_min < sample
    assert [matches(b, w) for w in wheres[:4]] == [at_min, sample - at_min, at_min, sample - at_min]
    assert 0 < matches(b, wheres[4]) < sample
    assert [matches(b, w) for w in wheres[5:10]] == [0, sample, sample, sample, 0]
    assert [matches(b, w) for w in wheres[10:]] == [sample - at_min, sample]

    def body(sim, what):
        for lo, hi in RANGES:
            for where in wheres:
                got = sim.select_instances(2, where, lo, hi, ticks=True)
                assert_selection_equal(got, selectcheck.expected(b.rows, b.keys, 2, lo, hi, where),
                                       f"{what} [{lo}, {hi}) where {where}")

    b.each(body)


def test_instance_sets_from_node_clauses(batch):
    b = batch
    wheres = signed_wheres(b)
    cases = [("at INT32_MIN", wheres[0]), ("above INT32_MIN", wheres[1]), ("lower half", wheres[4])]
    inner = [[], [("node", N2, INT32_MIN, INT32_MIN, "not")], [("node", N1, None, -1)]]

    def body(sim, what):
        for name, where in cases:
            mask = clause_mask(b.rows, b.keys, 2, where)
            assert 0 < int(mask.sum()) < int(b.ok.sum())
            iset = sim.instance_set(2, where)
            assert iset.info == selectcheck.expected(b.rows, b.keys, 2, 0, N, where)[0]
            assert np.array_equal(iset.insts(), members(mask))
            for sid in (2, 0):                                  # the set's own snapshot and another one
                check_in(sim, b.rows, b.keys, mask, iset, sid, RANGES, f"{what} {name}", wheres=inner,
                         spec=dict(tick_lo=0, tick_bins=256, msg_bins=16))

    b.each(body)


def signed_pairs(b):
    """(sid, field, index, lo, width, bins) pairs: node axes of negative lo, an axis that starts at the
    least N1, the pair (N1, N2) whose sum of products wraps, and an axis whose lo is INT64_MIN."""
    n1_wide = (0, "node", N1, -2**31, 2**20, 4096)
    n2_wide = (2, "node", N2, -2**31, 2**20, 64)
    n1_fine = (0, "node", N1, b.n1_min, 1, 64)
    n2_fine = (2, "node", N2, INT32_MIN, 1, 64)
    n2_far = (2, "node", N2, I64_MIN, 2**52, 4096)
    one = (1, "tick", None, 0, 1, 1)
    return [(n1_fine, n2_wide), (n2_fine, n1_fine), (n1_wide, one), (one, n1_wide), (n2_far, one),
            ((1, "node", N1, I64_MIN, 2**52, 64), (2, "node", N2, I64_MIN, 2**57, 64))]


def test_crosstab_bins_and_wrapped_products(batch):
    b = batch
    pairs = signed_pairs(b)
    a, c = b.rows.node[0][b.ok, N1], b.rows.node[2][b.ok, N2]
    assert abs(true_sum(a, c)) >= 2**63 and true_sum(c) >= 2**64            # sum_ab and sum_bb wrap
    want = crosstab_expected(b.rows, b.keys, *pairs[0], 0, N)
    assert int(want[XT_SUM_AB]) % 2**64 == true_sum(a, c) % 2**64
    assert int(want[XT_SUM_AA]) % 2**64 == true_sum(a) % 2**64
    # where the values must fall: the top bin of 4096 from -2^31, and the two sides of bin 2048 from INT64_MIN
    assert crosstab_expected(b.rows, b.keys, *pairs[2], 0, N)[cl.XT_CELLS + 4095] == int(b.ok.sum())
    assert crosstab_expected(b.rows, b.keys, *pairs[4], 0, N)[cl.XT_CELLS + 2047] == int(b.ok.sum())

    def body(sim, what):
        for x, y in pairs:
            for lo, hi in RANGES:
                got = sim.snapshot_crosstab(x, y, lo, hi)
                assert_crosstab_equal(got.raw, crosstab_expected(b.rows, b.keys, x, y, lo, hi),
                                      f"{what} {x} x {y} [{lo}, {hi})")
                assert int(got.table.sum()) == got.sample

    b.each(body)


def test_groups_and_their_keys(batch):
    b = batch
    named = [(2, "node", "N2"), (0, "node", "N1"), (2, "key", None)]
    terms = [(2, "node", N2), (0, "node", N1), (2, "key", None)]
    assert groups_expected(b.rows, b.keys, terms, 0, N)[0][3] > 1

    def body(sim, what):
        for lo, hi in RANGES:
            got = sim.snapshot_groups(named, lo, hi, group_of=True)
            assert_groups_equal(got, groups_expected(b.rows, b.keys, terms, lo, hi), f"{what} [{lo}, {hi})")
            assert got.n_returned == got.n_groups
            for j in range(got.n_returned):
                assert cl.group_key(got.values[j]) == int(got.groups["key"][j]), f"{what} group {j}"
            assert (got.values[:, 0] < 0).all() and (got.values[:, 1] > TOP).all()

    b.each(body)


ORDER_TERMS = [(2, "node", N2), (0, "node", N1)]


def test_order_on_both_sides_of_the_sign_bit(batch):
    b = batch
    low, high = (term_values(b.rows, b.keys, t)[b.ok] for t in ORDER_TERMS)
    assert int(low.min()) == INT32_MIN and int(low.max()) < 0 < TOP < int(high.min())
    assert np.unique(low).size > 2 and np.unique(high).size > 2
    b.each(lambda sim, what: order_check(sim, b.rows, b.keys, ORDER_TERMS, RANGES, what))


def test_contents_of_the_top_sixteen(batch):
    b = batch

    def body(sim, what):
        for term, largest in ((ORDER_TERMS[0], False), (ORDER_TERMS[1], True)):
            sid = term[0]
            top = sim.snapshot_topk(term, 16, largest)
            assert_topk_equal(top, expected_topk(b.rows, b.keys, term, 16, largest, 0, N), 16, largest, what)
            tok, done, off, msg = sim.collect_snapshot_list(sid, top.insts)
            ch = sim.num_channels
            assert tok.shape == (16, 3) and done.all() and off.shape == (16 * ch + 1,) and off[-1] == msg.size
            for r, i in enumerate(top.insts):
                otok, ooff, ovals = b.keys.refs[int(i)].collect_channels(sid)
                assert np.array_equal(tok[r], otok), f"{what} row {r}: tokens"
                assert top.values[r] == otok[term[2]]
                mine = [msg[off[r * ch + c]:off[r * ch + c + 1]].tolist() for c in range(ch)]
                assert mine == [ovals[ooff[c]:ooff[c + 1]].tolist() for c in range(ch)], f"{what} row {r}: messages"

    b.each(body)


# ---- ragged batches, block-major through the slot map ---------------------------------------------------------
@ENGINES
@pytest.mark.parametrize("n", [63, SMALL])
def test_ragged_block_major(n, engine):
    lanes = engine == LANES
    top, events = signed_texts(lanes)
    rows, keys = signed(n, lanes)
    ok = rows.status == O.OK
    sim, twin = blocked_ragged_sim(top, events, n, engine, fifo_lds_slots=SLOTS, want_engine=used_engine(engine))
    assert n % 64 != 0 and sim.records_blocked() and not twin.records_blocked()
    what = f"ragged n = {n}"
    ranges = ranges_of(n)
    where = [("node", N2, INT32_MIN + 1, -1), ("node", N1, TOP, INT32_MAX)]
    assert 0 < selectcheck.expected(rows, keys, 2, 0, n, where)[0][3] < int(ok.sum())
    pair = ((0, "node", N1, int(rows.node[0][ok, N1].min()), 1, 64), (2, "node", N2, -2**31, 2**20, 64))
    for s, layout_name in ((sim, "block-major"), (twin, "instance-major")):
        tag = f"{what} {layout_name}"
        stats_check(s, rows, ranges, tag)
        census_check(s, keys, ranges, tag)
        for lo, hi in ranges:
            got = s.select_instances(2, where, lo, hi, ticks=True)
            assert_selection_equal(got, selectcheck.expected(rows, keys, 2, lo, hi, where), f"{tag} [{lo}, {hi})")
            got = s.snapshot_crosstab(*pair, lo, hi)
            assert_crosstab_equal(got.raw, crosstab_expected(rows, keys, *pair, lo, hi), f"{tag} [{lo}, {hi})")
            for largest in (False, True):
                got = s.snapshot_topk(ORDER_TERMS[0], 16, largest, lo, hi)
                assert_topk_equal(got, expected_topk(rows, keys, ORDER_TERMS[0], 16, largest, lo, hi), 16, largest,
                                  f"{tag} [{lo}, {hi})")
    for sid in range(3):                                                    # the instance-major twin agrees
        assert sim.snapshot_stats(sid) == twin.snapshot_stats(sid)
        assert sim.snapshot_topk((sid, "node", N2), 16) == twin.snapshot_topk((sid, "node", N2), 16)
    assert sim.snapshot_crosstab(*pair).raw.tobytes() == twin.snapshot_crosstab(*pair).raw.tobytes()


# ---- MAXED: a node at INT32_MAX ---------------------------------------------------------------------------------
@ENGINES
def test_maxed_analytics(engine):
    lanes = engine == LANES
    top, events = maxed_texts(lanes)
    rows, keys = maxed(SMALL, lanes)
    sim = make_sim(top, events, SMALL, engine)
    flush_on(sim, engine)
    assert sim.exec_engine() == used_engine(engine)
    ranges = [(0, SMALL), (37, 201)]
    stats_check(sim, rows, ranges, "maxed")
    census_check(sim, keys, ranges, "maxed")
    for sid in range(2):
        st = sim.snapshot_stats(sid)
        assert st.max_node[N1] == INT32_MAX and st.min_node[N3] == -7 == st.max_node[N3]
        where = [("node", N1, INT32_MAX, INT32_MAX)]
        n_match = int((rows.node[sid][:, N1] == INT32_MAX).sum())
        assert 0 < n_match < SMALL
        for lo, hi in ranges:
            got = sim.select_instances(sid, where, lo, hi, ticks=True)
            want = selectcheck.expected(rows, keys, sid, lo, hi, where)
            assert_selection_equal(got, want, f"maxed sid {sid} [{lo}, {hi})")
        assert sim.select_instances(sid, where).n_match == n_match
        below = [("node", N1, INT32_MAX, None, "not"), ("node", N3, -7, -7)]
        assert sim.select_instances(sid, below).n_match == SMALL - n_match
    term = (0, "node", N1)
    for lo, hi in ranges:
        for k in (1, 16, SMALL):
            got = sim.snapshot_topk(term, k, True, lo, hi)
            assert_topk_equal(got, expected_topk(rows, keys, term, k, True, lo, hi), k, True,
                              f"maxed k {k} [{lo}, {hi})")
    assert sim.snapshot_topk(term, 1, True).values.tolist() == [INT32_MAX]
    order_check(sim, rows, keys, [term, (1, "node", N3)], ranges, "maxed")
