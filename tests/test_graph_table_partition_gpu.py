"""The per-snapshot summary table of a graph-partitioned run: 2 ranks over gloo share the GPU
(the worker pattern of test_partition_gpu.py), each reduces the table of its own part on the
device, and PartitionedGraphSim.snapshot_table all-gathers and merges them.  The merged table
must equal the table of the oracle's unpartitioned run, exactly."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from snapcheck import ROOT

pytestmark = pytest.mark.gpu

WORLD = 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _program(kind, n, steps, seed):
    import graphcheck as GC
    if kind == "regular":
        return GC.regular_program(n, steps=steps, seed=seed, snaps=((5, None), (5, 0), (9, None), (17, None)))
    p = GC.powerlaw_program(n, steps, 12, seed=seed, fifo_slots=512)   # (hub channels queue deep)
    p.traffic_steps = 60
    return p


def _worker(rank, world, port, case, out):
    import sys
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import graphcheck as GC
        kind, n, steps, seed, drain, transport = case
        p = _program(kind, n, steps, seed)
        g = GC.clg.GraphSim(device=0, fifo_slots=p.fifo_slots, max_snapshots=len(p.snap_step))
        g.set_topology(p.tokens, p.src, p.dst, id_width=p.width())
        g.set_delay_hash(p.delay_seed)
        g.set_traffic(p.traffic_seed, p.thresh, p.traffic_steps)
        ps = GC.clg.PartitionedGraphSim(g, rank, world, transport=transport)
        ps.run_program(p.steps, p.snap_step, p.snap_rank)
        if drain:
            assert ps.drain()
        own = g.snapshot_table()                     # this rank's part
        merged = ps.snapshot_table()                 # (a collective: every rank calls it)
        out[rank] = (g.status(), ps.lo, ps.hi, own.rows.tobytes(), merged.rows.tobytes())
    except Exception as e:  # surfaced in the parent
        out[f"error{rank}"] = repr(e)
        raise
    finally:
        dist.destroy_process_group()


CASES = [("regular", 4096, 90, 3, False, "host"), ("powerlaw", 2000, 70, 9, True, "device")]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}{c[1]}{'_drain' if c[4] else ''}_{c[5]}")
def test_partitioned_table_vs_oracle(case):
    import graphcheck as GC
    import tablecheck as T
    kind, n, steps, seed, drain, _ = case
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(WORLD, _free_port(), case, out), nprocs=WORLD, join=True)
    assert all(r in out for r in range(WORLD)), dict(out)
    p = _program(kind, n, steps, seed)
    o = GC.oracle_program(p, drain=drain, log=True)
    want = T.expected_table(o)          # whatever the oracle shows: complete or not
    assert o.status == 0
    if drain:
        assert (want["complete_tick"] >= 0).all()
    parts = []
    for r in range(WORLD):
        status, lo, hi, own, merged = out[r]
        assert status == 0
        T.assert_rows_equal(np.frombuffer(merged, dtype=T.DTYPE), want)      # the same on every rank
        parts.append((lo, hi, np.frombuffer(own, dtype=T.DTYPE)))
    for lo, hi, own in parts:
        # the initiator and the start are reported by the rank that owns the node, only
        mine = (want["initiator"] >= lo) & (want["initiator"] < hi)
        np.testing.assert_array_equal(own["initiator"], np.where(mine, want["initiator"], -1))
        np.testing.assert_array_equal(own["start_tick"], np.where(mine, want["start_tick"], -1))
        assert (own["nodes_created"] <= hi - lo).all()
    assert sum(int(own["nodes_created"].sum()) for _, _, own in parts) == int(want["nodes_created"].sum())
    merged_here = GC.clg.SnapshotTable(parts[0][2]).merge(GC.clg.SnapshotTable(parts[1][2]))
    T.assert_rows_equal(merged_here.rows, want)
