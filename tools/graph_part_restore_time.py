"""Time of a partitioned run that begins in a restored cut (PartitionedGraphSim.from_cut,
cl_graph_part_begin_seeded) and of the collective that takes such a cut (PartitionedGraphSim.cut),
next to the unpartitioned restore of the same cut: one JSON line (profiles/graph_part_restore.json).

A REHEARSAL, not a multi-GPU measurement: RANKS processes share ONE GPU and exchange over gloo
through host memory, as the partition tests do.  What it can show is the cost of the new steps on
one device and that nothing in them grows with the rank count; it says nothing about xGMI or RCCL.

The program is a power-law graph of the tests' kind (tests/graphcheck.py powerlaw_program: NODES
nodes, 8 targets, traffic on every step, SNAPS snapshots, the drain).  The source runs
unpartitioned in the first process, which takes the last completed snapshot as a SnapshotCut with
its topology, saves it, and measures
  whole   restore_cut + flush of that cut on a fresh template: wall_ms, and the device times
          build_ms (check, offsets, sums) and seed_ms (k_seed over the whole cut).
Then RANKS processes load the file and each measures, fastest of REPS:
  template_ms   GraphSim.template_of_cut: the topology from the file (what from_cut(template=None) adds)
  from_cut_ms   wall time of PartitionedGraphSim.from_cut(cut, rank, RANKS, template): restore_cut of the
                whole cut on this rank, then cl_graph_part_begin_seeded (the mode's buffers, the reset,
                the share and seed kernels, one synchronise)
  build_ms, seed_ms   device times of that restore's kernels and of this rank's seed kernel
  share         (entry lo, entry hi, message lo, message hi) this rank queued
  cut_ms        wall time of the collective PartitionedGraphSim.cut(0) after the restored run took
                one snapshot and drained: each part's sparse collect, all_gather_object, the merge
Wall times are taken around calls that end on the host or with a stream synchronise; the ranks are
not lined up by a barrier before from_cut, which is no collective.  The spread between runs is not
measured.

usage: python tools/graph_part_restore_time.py [--out PATH] [--transport host|device]
"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

OUT = os.path.join(ROOT, "profiles", "graph_part_restore.json")
NODES, STEPS, SNAPS, SEED = 20000, 40, 8, 21
FIFO = 512
DELAY = 41
RANKS = 2
REPS = 3


def now():
    return time.perf_counter() * 1e3


def source(path):
    """The unpartitioned source run, its cut into `path`, and the unpartitioned restore of it."""
    import numpy as np

    import graphcheck as GC
    clg = GC.clg
    p = GC.powerlaw_program(NODES, STEPS, SNAPS, seed=SEED, fifo_slots=FIFO)
    g = GC.engine_program(p, drain=True, max_drain=1_000_000)
    assert g.status() == 0
    done = np.nonzero(g.snapshot_table().rows["complete_tick"] >= 0)[0]
    assert done.size, "the run completed no snapshot"
    sid = int(done[-1])
    cut = g.cut(sid, topology=True)
    cut.save(path)
    template = clg.GraphSim.template_of_cut(cut, fifo_slots=FIFO)
    template.set_delay_hash(DELAY)
    best = {}
    for rep in range(REPS + 1):                            # (rep 0 warms up)
        t0 = now()
        r = template.restore_cut(cut)
        r.flush()
        wall = now() - t0
        build_ms, seed_ms = r.restore_time()
        if rep:
            for k, v in (("wall_ms", wall), ("build_ms", build_ms), ("seed_ms", seed_ms)):
                best[k] = min(best.get(k, v), v)
    return {"nodes": g.num_nodes, "channels": g.num_channels, "snapshots": g.num_snapshots, "sid": sid,
            "seed_info": r.seed_info, "whole": {k: round(v, 4) for k, v in best.items()}}


def rank_main(rank, world, port, path, transport, out):
    import torch.distributed as dist

    import cutcheck as CC
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        clg = CC.graph_module()
        cut = clg.SnapshotCut.load(path)
        best = {}

        def keep(k, v):
            best[k] = min(best.get(k, v), v)

        for rep in range(REPS + 1):                        # (rep 0 warms up)
            t0 = now()
            template = clg.GraphSim.template_of_cut(cut, fifo_slots=FIFO)
            t1 = now()
            ps = clg.PartitionedGraphSim.from_cut(cut, rank, world, template=template,
                                                  configure=lambda r: r.set_delay_hash(DELAY), transport=transport)
            t2 = now()
            build_ms, seed_ms = ps.g.restore_time()
            if rep:
                for k, v in (("template_ms", t1 - t0), ("from_cut_ms", t2 - t1), ("build_ms", build_ms),
                             ("seed_ms", seed_ms)):
                    keep(k, v)
            if rep < REPS:
                del ps, template
        ps.start()
        ps.start_snapshot_rank(0)
        assert ps.drain() and ps.g.status() == 0
        for rep in range(REPS + 1):
            dist.barrier()
            t0 = now()
            c = ps.cut(0)
            if rep:
                keep("cut_ms", now() - t0)
        res = {k: round(v, 4) for k, v in best.items()}
        res.update(share=list(ps.seed_share), nodes=[ps.lo, ps.hi], cut_entries=c.channels, cut_msgs=c.msgs)
        out[rank] = res
    finally:
        dist.destroy_process_group()


def main(argv):
    import socket

    import torch.multiprocessing as mp
    out_path, transport = OUT, "host"
    while argv:
        a = argv.pop(0)
        if a == "--out":
            out_path = argv.pop(0)
        elif a == "--transport":
            transport = argv.pop(0)
        else:
            print(__doc__, file=sys.stderr)
            return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cut.npz")
        # the source runs in a process of its own, so that the ranks start on a GPU nobody else holds
        ctx = mp.get_context("spawn")
        mgr = ctx.Manager()
        doc = mgr.dict()
        src = ctx.Process(target=_source_main, args=(path, doc))
        src.start()
        src.join(300)
        if src.is_alive() or src.exitcode != 0:
            src.kill()
            print(f"the source run failed (exit status {src.exitcode})", file=sys.stderr)
            return 1
        ranks = mgr.dict()
        mp.spawn(rank_main, args=(RANKS, port, path, transport, ranks), nprocs=RANKS, join=True)
        line = dict(doc["source"])
        line.update(ranks=RANKS, transport=transport, exchange="gloo, one GPU shared", reps=REPS,
                    per_rank=[ranks[r] for r in range(RANKS)])
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    return 0


def _source_main(path, doc):
    doc["source"] = source(path)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
