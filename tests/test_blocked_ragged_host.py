"""The scenarios of test_blocked_ragged_gpu.py on the oracle alone (no GPU): that a small C3 batch is
predicted to spill -- and so to replay split, through the slot map, with block-major records -- and
that what the GPU cases then read is not vacuous.

The prediction is blockedcheck.spill_prediction: per instance, the most packets one channel held at
once, read after every event and every tick through the drain.  With 4 ring slots per channel an
instance whose peak exceeds 4 is a predicted spiller.
"""
import numpy as np
import pytest

import censuscheck
import oracle as O
import selectcheck
from blockedcheck import (C3_EVENTS, C3_TOP, N_RING17, N_SORT, RING17_EVENTS, RING17_TOP, SLOTS, SMALL_SIZES,
                          UNDRAINED_EVENTS, spill_prediction, undrained_refs)
from enginecheck import oracle_batch
from groupscheck import expected as groups_expected
from test_census_gpu import EVENTS3, HUB_EVENTS, HUB_TOP, TOP3

NOT_OK = [2, 32, 37, 52, 61, 126, 250, 251]                  # of the first 257
SPILLERS = [34, 41, 50, 73, 87, 101, 103, 109, 112, 125, 152, 192, 195, 222, 231, 248]


@pytest.fixture(scope="module")
def c3():
    return spill_prediction(C3_TOP, C3_EVENTS, 257, SLOTS)


def test_the_walk_is_the_oracles_own_run(c3):
    """Event by event with the drain restated here, the walk ends where read_events_text ends."""
    _, status, ticks, _, _ = oracle_batch(C3_TOP, C3_EVENTS, 257)
    assert np.array_equal(status, c3.status)
    ok = status == O.OK
    assert np.array_equal(ticks[ok], c3.time[ok])


@pytest.mark.parametrize("n", SMALL_SIZES + (127,))
def test_small_c3_batches_are_predicted_to_split(c3, n):
    bad = np.flatnonzero(c3.status[:n] != O.OK).tolist()
    assert bad == [i for i in NOT_OK if i < n]
    assert (c3.status[bad] == O.FATAL_INSUFFICIENT_TOKENS).all()
    spill = c3.spillers(n).tolist()
    assert spill == [i for i in SPILLERS if i < n]
    assert len(spill) == {63: 3, 65: 3, 127: 10, 130: 10, 200: 13, 257: 16}[n]
    assert int((c3.peak[:n] > SLOTS + 1).sum()) == 0          # 5 packets at the most: 8 slots hold everything
    # both OK and not-OK instances; the spillers are OK (their records are read) ...
    assert 0 < len(bad) < n and (c3.status[spill] == O.OK).all()
    # ... and one lies below n - 1, so "the clean ones, then the spillers" is not the identity
    assert spill[0] < n - 1
    # a split needs one wave of clean instances on either kernel (64 at the most)
    assert n - len(spill) >= 8 and (n - len(spill) >= 64 or n < 64 + len(spill))


def test_c3_samples_at_the_edges():
    rows, keys = selectcheck.scenario(C3_TOP, C3_EVENTS, 257)
    assert rows.n_sids == 5
    # n = 65: instance 64, alone in the instance-major last tile, is OK and in the sample of sid 0
    assert rows.status[64] == O.OK and rows.done[0][64]
    # the drain completes every snapshot of every OK instance: the five samples are the same 249
    assert [int(d.sum()) for d in rows.done] == [249] * 5 == [int((rows.status == O.OK).sum())] * 5
    # more than one class per snapshot id, within the first 63 already
    assert all(censuscheck.expected(keys, sid, 0, 63)[0][3] > 1 for sid in range(5))


def test_undrained_c3_leaves_late_snapshots_incomplete():
    """C3's events, 6 ticks and no drain (test_iset_gpu's cross-sid scenario): snapshots 3 and 4 are
    incomplete in some OK instances, at every small size, and the batch still spills."""
    rows, _ = selectcheck.from_refs(undrained_refs(C3_TOP, UNDRAINED_EVENTS, 257))
    assert np.flatnonzero(rows.status != O.OK).tolist() == NOT_OK
    assert [int(d.sum()) for d in rows.done] == [216, 219, 249, 107, 8]
    for n in SMALL_SIZES:
        ok = int((rows.status[:n] == O.OK).sum())
        for sid in (3, 4):
            assert 0 < int(rows.done[sid][:n].sum()) < ok, (n, sid)
    pred = spill_prediction(C3_TOP, UNDRAINED_EVENTS, 257, SLOTS, drain=False)
    assert pred.spillers().tolist() == SPILLERS                # the peaks come before the drain


def test_ring_of_17_is_predicted_to_split_and_its_last_record_varies():
    pred = spill_prediction(RING17_TOP, RING17_EVENTS, N_RING17, SLOTS)
    assert (pred.status == O.OK).all()
    assert pred.spillers().size == 68 and pred.spillers()[0] == 0 and int(pred.peak.max()) == 6
    rows, _ = selectcheck.scenario(RING17_TOP, RING17_EVENTS, N_RING17)
    assert rows.n_sids == 2 and rows.done[0].all() and rows.done[1].all()
    assert rows.node[0].shape[1] * 2 == 34                    # 2-word records: 34 record words, two chunks
    # R16's record, the single-node chunk: its tokens and its in-channel's messages vary in snapshot 0
    assert np.unique(rows.node[0][:, 16], return_counts=True)[1].tolist() == [80, 50]
    assert np.unique(rows.ch_msgs[0][:, 15]).tolist() == [1, 2] and np.unique(rows.ch_tok[0][:, 15]).tolist() == [1, 4]


def test_sort_order_scenarios_at_4096_plus_37():
    """What the 4096-instance tests assert about the hub and the three-node scenario, re-measured at
    the 4133 instances of the sort-order cases."""
    rows, keys = selectcheck.scenario(TOP3, EVENTS3, N_SORT)
    assert (rows.status == O.OK).all() and rows.n_sids == 2
    want = censuscheck.expected(keys, 0, 0, N_SORT)
    counts = want[1]["count"]
    assert want[0] == (N_SORT, N_SORT, N_SORT, 413)            # 413 classes, as at 4096
    assert int((counts == 1).sum()) == 142 and (np.diff(counts[counts > 1]) == 0).any()
    assert int(rows.ch_msgs[0].max()) == 12                    # the message clamp of 8 bins is hit
    assert rows.tick[0].min() < 20 and rows.tick[0].max() >= 23   # both tick clamps
    assert groups_expected(rows, keys, [(0, "ch_tok", 0), (1, "tick", None)], 0, N_SORT)[0][3] == 102
    # at 8 ring slots 63 of its first 65 instances exceed the ring: no wave of clean instances, no
    # small split -- the scenario is mapped by the length sort alone
    assert spill_prediction(TOP3, EVENTS3, 65, 8).spillers().size == 63

    rows, keys = selectcheck.scenario(HUB_TOP, HUB_EVENTS, N_SORT)
    assert (rows.status == O.OK).all() and rows.n_sids == 4
    assert [censuscheck.expected(keys, sid, 0, N_SORT)[0][3] for sid in range(4)] == [64, 51, 32, 16]

    c3 = spill_prediction(C3_TOP, C3_EVENTS, N_SORT, SLOTS)
    assert int((c3.status != O.OK).sum()) == 117
    assert c3.spillers().size == 271 and int((c3.peak > 5).sum()) == 6     # 6.6 %
