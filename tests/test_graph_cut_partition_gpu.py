"""A partitioned run restored from through its merged cut: 2 ranks over gloo share the GPU (the
worker pattern of test_graph_table_partition_gpu.py, its drained power-law case),
PartitionedGraphSim.collect_sparse(tokens=True) gathers and merges the whole cut on every rank, and
rank 0 takes one snapshot of it as a SnapshotCut into GraphSim.restore_cut on a fresh, unpartitioned
template of the same topology.  The cut must equal the unpartitioned oracle run's, and the restored
run's continuation the oracle equivalent (restorecheck), exactly."""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

import test_graph_table_partition_gpu as TP
from snapcheck import ROOT

pytestmark = pytest.mark.gpu

WORLD = 2
CASE = TP.CASES[1]
SID = 5
DELAY = ("hash", 41)                  # the restored run's own delay source
OPS = [("snap", 1234), ("drain",)]    # the continuation: one snapshot, then the drain
CUT_FIELDS = ("tokens", "channel", "count", "msg_tokens")


def _worker(rank, world, port, out):
    import sys
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import cutcheck as CC
        clg = CC.graph_module()
        kind, n, steps, seed, drain, transport = CASE
        p = TP._program(kind, n, steps, seed)
        g = clg.GraphSim(device=0, fifo_slots=p.fifo_slots, max_snapshots=len(p.snap_step))
        g.set_topology(p.tokens, p.src, p.dst, id_width=p.width())
        g.set_delay_hash(p.delay_seed)
        g.set_traffic(p.traffic_seed, p.thresh, p.traffic_steps)
        ps = clg.PartitionedGraphSim(g, rank, world, transport=transport)
        ps.run_program(p.steps, p.snap_step, p.snap_rank)
        assert drain and ps.drain()
        merged = ps.collect_sparse(tokens=True)          # (a collective: every rank calls it)
        if rank == 0:
            template = clg.GraphSim(device=0, fifo_slots=p.fifo_slots)       # unpartitioned, no traffic, never run
            template.set_topology(p.tokens, p.src, p.dst, id_width=p.width())
            template.set_delay_hash(DELAY[1])
            cut = merged.cut(SID, sim=template)
            r = template.restore_cut(cut)
            info = r.seed_info
            CC.run_engine(r, OPS)
            out["cut"] = {f: getattr(cut, f).tolist() for f in CUT_FIELDS}
            out["key"] = (cut.source_sid, cut.n_channels, cut.topology_key, template.topology_key())
            out["info"] = info
            out["run"] = CC.results_doc(r)
        out[rank] = g.status()
    except Exception as e:  # surfaced in the parent
        out[f"error{rank}"] = repr(e)
        raise
    finally:
        dist.destroy_process_group()


def test_partitioned_run_restored_through_its_merged_cut():
    import graphcheck as GC
    import restorecheck as R
    kind, n, steps, seed, drain, _ = CASE
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(WORLD, TP._free_port(), out), nprocs=WORLD, join=True)
    assert all(out.get(r) == 0 for r in range(WORLD)), dict(out)
    p = TP._program(kind, n, steps, seed)
    o = GC.oracle_program(p, drain=True)                  # the unpartitioned run
    assert o.status == 0 and o.complete(SID)
    shape = GC.clg.GraphSim()                             # (host only: the channel list in rank order)
    shape.set_topology(p.tokens, p.src, p.dst, id_width=p.width())
    csrc, cdst = shape.channels()
    want = R.seed_of_oracle(o, SID, csrc, cdst)
    assert (want.channels, want.msgs) == (7121, 11114)    # (the oracle's figures: several workgroups of the check)
    cut, nz = out["cut"], np.nonzero(want.counts)[0]
    assert cut["tokens"] == want.T.tolist() and cut["channel"] == nz.tolist()
    assert cut["count"] == want.counts[nz].tolist() and cut["msg_tokens"] == want.vals.tolist()
    sid, n_channels, key, tkey = out["key"]
    assert (sid, n_channels) == (SID, csrc.size) and key == tkey == GC.clg.topology_key(n, csrc, cdst)
    assert out["info"] == want.info(SID)
    oe = R.oracle_equivalent(want, DELAY, OPS)
    run = out["run"]
    assert (run["status"], run["time"]) == (oe.status, oe.time) and oe.status == 0
    nt = oe.node_tokens()
    assert run["node_tokens"] == [nt[k] for k in oe.node_ids()] and run["node_ids"] == oe.node_ids()
    oc = oe.counters()
    assert {k: run["counters"][k] for k in R.EVENT_COUNTERS} == {k: oc[k] for k in R.EVENT_COUNTERS}
    assert run["ticks"] == [oe.completion_tick(s) for s in range(oe.num_snapshots)] and len(run["ticks"]) == 1
    assert oe.complete(0)
    for got, exp in zip(run["collected"][0], oe.collect_channels(0)):
        assert got == exp.tolist()
