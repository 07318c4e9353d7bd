"""The sparse packed collect of a graph-partitioned run: 2 ranks over gloo share the GPU (the
worker pattern and the cases of test_graph_table_partition_gpu.py), each compacts the entries
of its own part on the device, and PartitionedGraphSim.collect_sparse gathers and merges them.
Each part must equal the oracle's unpartitioned run restricted to the part's nodes and the
channels into them, and the merged result the oracle's whole run, exactly."""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from snapcheck import ROOT
from test_graph_table_partition_gpu import CASES, WORLD, _free_port, _program

pytestmark = pytest.mark.gpu

FIELDS = ("sid_lo", "complete", "row_offsets", "channel", "count", "msg_tokens", "tokens", "node_lo", "node_hi")


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
        own = g.collect_sparse(tokens=True)          # this rank's part
        merged = ps.collect_sparse(tokens=True)      # (a collective: every rank calls it)
        out[rank] = (g.status(), ps.lo, ps.hi, tuple(getattr(own, f) for f in FIELDS),
                     tuple(getattr(merged, f) for f in FIELDS))
    except Exception as e:  # surfaced in the parent
        out[f"error{rank}"] = repr(e)
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}{c[1]}{'_drain' if c[4] else ''}_{c[5]}")
def test_partitioned_sparse_vs_oracle(case):
    import graphcheck as GC
    import sparsecheck as S
    SS = GC.clg.SparseSnapshots
    kind, n, steps, seed, drain, _ = case
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(WORLD, _free_port(), case, out), nprocs=WORLD, join=True)
    assert all(r in out for r in range(WORLD)), dict(out)
    p = _program(kind, n, steps, seed)
    o = GC.oracle_program(p, drain=drain)
    assert o.status == 0
    ns = o.num_snapshots
    want = S.expected_sparse(o, 0, ns)               # whatever the oracle shows: complete or not
    if drain:
        assert want.complete.all()
    assert want.n_entries > 0
    parts = []
    for r in range(WORLD):
        status, lo, hi, own, merged = out[r]
        assert status == 0
        own, merged = SS(*own), SS(*merged)
        S.assert_sparse_equal(merged, want)          # the same on every rank
        # a part completes a snapshot when its own nodes have: no later than the whole run
        assert (own.complete >= want.complete).all()
        S.assert_sparse_equal(own, S.expected_sparse(o, 0, ns, lo, hi, dst=p.dst, complete=own.complete))
        assert (p.dst[own.channel] >= lo).all() and (p.dst[own.channel] < hi).all()
        parts.append(own)
    np.testing.assert_array_equal(parts[0].complete & parts[1].complete, want.complete)
    assert sum(x.n_entries for x in parts) >= want.n_entries
    S.assert_sparse_equal(SS.merge(parts), want)
