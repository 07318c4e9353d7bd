"""Block-major snapshot records with a record size that is no power of two.

A hub with 10 out-links has degree bound 16 (the run-time-loop kernel), so a node record is
1 + max in-degree = 3 words.  At 4096 instances rerun() replays through the slot map and writes the
records block-major by slot; every reader goes through cl_engine.h rec_word, whose block-major
offset must be (idx / rw) * rw * 64 + idx % rw -- what the writer stores -- not the power-of-two
mask arithmetic.  Every result read after the replay must equal a flush-only sim (instance-major
records) and the oracle.
"""
import importlib

import numpy as np
import pytest

import oracle as O
from enginecheck import canonical, oracle_batch, oracle_run

cl = importlib.import_module("chandy-lamport-distributed-snapshot-algorithm_amd")
pytestmark = pytest.mark.gpu

_LEAVES = [f"L{k}" for k in range(10)]
HUB_TOP = (f"{len(_LEAVES) + 1}\nH 40\n" + "".join(f"{x} 5\n" for x in _LEAVES)
           + "".join(f"H {x}\n" for x in _LEAVES)
           + "".join(f"{_LEAVES[k]} {_LEAVES[(k + 1) % 10]}\n" for k in range(10)) + "L0 H\n")
HUB_EVENTS = "".join(f"send H {_LEAVES[(3 * r) % 10]} 2\nsnapshot {'H' if r % 2 == 0 else _LEAVES[r]}\n"
                     f"send L{r} L{r + 1} 1\ntick 2\n" for r in range(4))
N_INST = 4096
SAMPLE = (0, 1, 63, 64, 777, 2048, 4095)


def _sim():
    sim = cl.ChandyLamportSim(N_INST)
    sim.read_topology_text(HUB_TOP)
    assert sim.read_events_text(HUB_EVENTS) == 4
    sim.flush()
    return sim


def test_readers_after_blocked_replay_with_three_word_records():
    flat, sim = _sim(), _sim()
    assert not flat.records_blocked()
    sim.poison_outputs()
    sim.rerun()
    sim.synchronize()
    assert sim.records_blocked()

    assert (sim.status() == cl.INST_OK).all()
    assert np.array_equal(sim.checksums(), flat.checksums())
    assert sim.counters() == flat.counters()
    assert sim.counters(only_ok=True) == flat.counters(only_ok=True)
    hashes = sim.instance_hashes()
    assert np.array_equal(hashes, flat.instance_hashes())
    _, status, _, _, want_hashes = oracle_batch(HUB_TOP, HUB_EVENTS, N_INST)
    assert (status == O.OK).all()
    assert np.array_equal(hashes, want_hashes)

    for sid in range(4):
        for lo, hi in ((0, N_INST), (37, 3001)):
            got, want = sim.collect_snapshot_packed(sid, lo, hi), flat.collect_snapshot_packed(sid, lo, hi)
            for g, w in zip(got, want):
                assert np.array_equal(g, w)
    for i in SAMPLE:
        ref = oracle_run(HUB_TOP, HUB_EVENTS, seed=O.REFERENCE_SEED + i)
        for sid in range(4):
            got, base, want = sim.CollectSnapshot(sid, instance=i), flat.CollectSnapshot(sid, instance=i), ref.collect(sid)
            assert got.tokenMap == base.tokenMap == want.tokens
            assert canonical(got.messages) == canonical(base.messages) == canonical(want.messages)
