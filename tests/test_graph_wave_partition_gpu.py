"""The marker-wave profile and the marker tree of a graph-partitioned run: 2 ranks over gloo
share the GPU (the worker pattern of test_graph_table_partition_gpu.py).  Each rank reduces the
latency profile of its own nodes against the origins of the merged table, and
PartitionedGraphSim.snapshot_wave all-gathers and merges the parts; snapshot_tree all-gathers
the parts' planes into the whole tree, whose depth() is the depth the device cannot compute
across parts.  Everything must equal the oracle's unpartitioned run, exactly."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from snapcheck import ROOT

pytestmark = pytest.mark.gpu

WORLD = 2
SPEC = (12, 3)          # lat_bins, lat_width


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
        merged = ps.snapshot_wave(0, None, *SPEC)                   # (collectives: every rank calls them)
        sub = ps.snapshot_wave(1, 3, *SPEC)
        trees = [ps.snapshot_tree(sid) for sid in range(ps.n_sids)]
        bare = ps.snapshot_tree(0, ticks=False)
        start = ps.snapshot_table().rows["start_tick"]
        own = g.snapshot_wave(0, None, *SPEC, depth_bins=0, origins=start)      # this rank's part
        codes = []
        for kw in (dict(depth_bins=4, origins=start), dict(depth_bins=0), dict(depth_bins=4)):
            try:
                g.snapshot_wave(0, None, *SPEC, **kw)
                codes.append(0)
            except cl.ClSnapError as e:
                codes.append(e.code)
        out[rank] = (g.status(), ps.lo, ps.hi, own.rows.tobytes(), merged.rows.tobytes(), sub.rows.tobytes(),
                     np.stack([t.parent for t in trees]).tobytes(), np.stack([t.tick for t in trees]).tobytes(),
                     bare.parent.tobytes(), bare.tick is None, codes)
    except Exception as e:  # surfaced in the parent
        out[f"error{rank}"] = repr(e)
        raise
    finally:
        dist.destroy_process_group()


CASES = [("regular", 4096, 90, 3, False, "host"), ("powerlaw", 2000, 70, 9, True, "device")]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}{c[1]}{'_drain' if c[4] else ''}_{c[5]}")
def test_partitioned_wave_and_tree_vs_oracle(case):
    import graphcheck as GC
    import wavecheck as WC
    cl, clg = GC.cl, GC.clg
    kind, n, steps, seed, drain, _ = case
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(WORLD, _free_port(), case, out), nprocs=WORLD, join=True)
    assert all(r in out for r in range(WORLD)), dict(out)
    p = _program(kind, n, steps, seed)
    o = GC.oracle_program(p, drain=drain, log=True)
    assert o.status == 0
    x = WC.Expected(o)
    s = o.num_snapshots
    spec = SPEC + (0,)
    want = x.rows(*spec)
    assert (want[:, WC.W["created"]] > 0).all() and (want[:, WC.W["lat_max"]] >= SPEC[0] * SPEC[1]).any()
    rw = want.shape[1]
    parts = []
    for r in range(WORLD):
        status, lo, hi, own, merged, sub, parent, tick, bare, bare_has_no_tick, codes = out[r]
        assert status == 0
        assert codes == [cl.E_STATE] * 3, codes                 # no device depth, no origins of its own
        # the same on every rank: the merged profile, a sub-range of it, the gathered trees
        WC.assert_wave(clg.SnapshotWave(np.frombuffer(merged, dtype=np.int64), *spec), want, spec)
        WC.assert_wave(clg.SnapshotWave(np.frombuffer(sub, dtype=np.int64), *spec), want[1:3], spec)
        parent = np.frombuffer(parent, dtype=np.int32).reshape(s, n)
        tick = np.frombuffer(tick, dtype=np.int32).reshape(s, n)
        np.testing.assert_array_equal(parent, x.parent)
        np.testing.assert_array_equal(tick, x.tick)
        for sid in range(s):
            np.testing.assert_array_equal(clg.MarkerTree(parent[sid], tick[sid]).depth(), x.depth[sid])
        np.testing.assert_array_equal(np.frombuffer(bare, dtype=np.int32), x.parent[0])
        assert bare_has_no_tick
        # this rank's part: its own nodes, against the whole run's origins
        own = clg.SnapshotWave(np.frombuffer(own, dtype=np.int64), *spec)
        WC.assert_wave(own, x.rows(*spec, node_lo=lo, node_hi=hi), spec)
        assert own.rows.shape == (s, rw)
        parts.append(own)
    WC.assert_wave(parts[0].merge(parts[1]), want, spec)        # merged on the host here
