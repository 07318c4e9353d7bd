"""The node and channel profile of a graph-partitioned run: 2 ranks over gloo share the GPU (the
worker pattern and the cases of test_graph_table_partition_gpu.py), each profiles its own nodes
and the channels into them on the device, and PartitionedGraphSim.snapshot_profile gathers and
merges the parts.  Each part must equal the oracle restricted to its nodes, the merged profile the
oracle's whole run, exactly."""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from snapcheck import ROOT
from test_graph_table_partition_gpu import CASES, WORLD, _free_port, _program

pytestmark = pytest.mark.gpu

FIELDS = ("sid_lo", "used", "head", "hist", "entries", "node", "origins", "msg_width", "min_msgs")
EVERY_OTHER = dict(min_msgs=2, msg_bins=5, msg_width=2)


def _worker(rank, world, port, case, out):
    import sys
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import graphcheck as GC
        cl = GC.cl
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
        ns = g.num_snapshots
        pack = lambda pr: tuple(getattr(pr, f) for f in FIELDS)  # noqa: E731
        merged, parts = ps.snapshot_profile(parts=True)              # (a collective: every rank calls it)
        masked = ps.snapshot_profile(use=np.arange(ns) % 2 == 0, **EVERY_OTHER)
        try:                                                         # only the initiator's owner knows the start
            g.snapshot_profile(nodes=True, origins=None)
            code = 0
        except cl.ClSnapError as e:
            code = e.code
        bare = g.snapshot_profile(nodes=False, origins=None)         # the channel side needs no origin
        own_done = g.snapshot_table().rows["complete_tick"] >= 0
        out[rank] = (g.status(), ps.lo, ps.hi, pack(merged), [pack(x) for x in parts], pack(masked), code, cl.E_STATE,
                     pack(bare), own_done)
    except Exception as e:  # surfaced in the parent
        out[f"error{rank}"] = repr(e)
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}{c[1]}{'_drain' if c[4] else ''}_{c[5]}")
def test_partitioned_profile_vs_oracle(case):
    import graphcheck as GC
    import profilecheck as PC
    kind, n, steps, seed, drain, _ = case
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(WORLD, _free_port(), case, out), nprocs=WORLD, join=True)
    assert all(r in out for r in range(WORLD)), dict(out)
    p = _program(kind, n, steps, seed)
    o = GC.oracle_program(p, drain=drain, log=True)
    assert o.status == 0
    ns = o.num_snapshots
    done = np.array([o.complete(s) for s in range(ns)])
    assert done.any() and (done.all() or not drain)
    start = PC._epochs(o)[1]
    unit = 1                                                          # the synthetic traffic sends single tokens
    want = PC.expected_profile(o, 0, ns, origins=start, unit_payloads=unit, dst=p.dst)
    want_masked = PC.expected_profile(o, 0, ns, use=np.arange(ns) % 2 == 0, origins=start, unit_payloads=unit,
                                      dst=p.dst, **EVERY_OTHER)
    assert want.entries.size > 0 and want.n_used == done.sum()
    SP = GC.clg.SnapshotProfile
    lo_hi = []
    for r in range(WORLD):
        status, lo, hi, merged, parts, masked, code, e_state, bare, own_done = out[r]
        assert status == 0 and code == e_state
        PC.assert_profile_equal(SP(*merged), want)                    # the same on every rank
        PC.assert_profile_equal(SP(*masked), want_masked)
        np.testing.assert_array_equal(SP(*merged).used != 0, done)    # the mask the collective used
        parts = [SP(*x) for x in parts]
        PC.assert_profile_equal(SP.merge(parts), want)
        assert [(x.node_lo, x.node_hi) for x in parts][r] == (lo, hi)
        lo_hi.append((lo, hi))
        # this rank's part: the oracle restricted to its nodes and the channels into them
        mine = PC.expected_profile(o, 0, ns, use=done, origins=start, unit_payloads=unit, node_lo=lo, node_hi=hi,
                                   dst=p.dst, complete=own_done)
        PC.assert_profile_equal(parts[r], mine)
        assert (p.dst[parts[r].entries["channel"]] >= lo).all() and (p.dst[parts[r].entries["channel"]] < hi).all()
        # without node rows a part needs no origins; its used rows are its own completed snapshots
        alone = PC.expected_profile(o, 0, ns, nodes=False, unit_payloads=unit, node_lo=lo, node_hi=hi, dst=p.dst,
                                    complete=own_done)
        PC.assert_profile_equal(SP(*bare), alone, nodes=False)
    assert lo_hi[0][0] == 0 and lo_hi[0][1] == lo_hi[1][0] and lo_hi[1][1] == n
