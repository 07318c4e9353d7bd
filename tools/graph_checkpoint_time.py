"""Time of a checkpoint of the graph engine -- a completed snapshot taken to the host as a
SnapshotCut, saved, loaded and restored from with no source graph (GraphSim.cut / SnapshotCut.save /
load / GraphSim.from_cut, cl_graph_restore_cut) -- next to restore(sid) of the same snapshot in the
same process, one JSON line per case (the lines of profiles/graph_checkpoint.json).  The cases are
bench.py's graph configs c4 and c5 (tests/graphcheck.py bench_program); the snapshot is the last one
the run completed, as in tools/graph_restore_time.py.

  seed_info           cl_graph_seed_info of the graph restored from the file (printed, and in the line)
  ids_ms              wall time of the source graph's first node_ids(): N calls, made once per graph
                      (cut(topology=True) needs the ids; every later cut finds them kept)
  cut_ms              wall time of g.cut(sid, topology=True): the sparse collect of the one snapshot
                      with its token plane, the channel list, the kept ids
  save_ms, load_ms    wall time of SnapshotCut.save / SnapshotCut.load; file_bytes the file's size
  from_cut_wall_ms    wall time of GraphSim.from_cut(cut) + set_limits + set_delay_hash + flush(): a
                      graph that stands in the cut, from the loaded file alone
  build_ms, seed_ms   device time of that restore's kernels (check, offsets, sums) and of its seed kernel
  upload_bytes        4 x (N + 2 x entries + messages): what restore_cut sends to the device
  restore_wall_ms     wall time of g.restore(sid) + set_limits + flush() (graph_restore_time's figure)
  restore_build_ms, restore_seed_ms   its device times
Both routes are warmed up once, then alternate REPS times; the fastest of each is kept.  Wall times
are taken around calls that end on the host or with a stream synchronise.  After one snapshot and
the drain on both graphs their checksums (and counters) are checked to be equal.  Each case runs in
a process of its own under a time limit; a case that fails ends the tool.

usage: python tools/graph_checkpoint_time.py [c4|c5 ...]     (default: both, into profiles/graph_checkpoint.json)
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

OUT = os.path.join(ROOT, "profiles", "graph_checkpoint.json")
LIMIT_S = {"c4": 420, "c5": 540}
REPS = 3


def now():
    return time.perf_counter() * 1e3


def restore_route(g, sid, fifo):
    t0 = now()
    r = g.restore(sid)
    r.set_limits(fifo, 1, 1_000_000)        # (one snapshot of its own: small snapshot planes)
    r.flush()
    return r, now() - t0


def checkpoint_route(g, clg, sid, fifo, delay, path):
    t0 = now()
    cut = g.cut(sid, topology=True)
    t1 = now()
    cut.save(path)
    t2 = now()
    del cut
    loaded = clg.SnapshotCut.load(path)
    t3 = now()
    r = clg.GraphSim.from_cut(loaded, fifo_slots=fifo, max_snapshots=1, max_drain_ticks=1_000_000)
    r.set_delay_hash(delay)
    r.flush()
    t4 = now()
    return r, loaded, {"cut_ms": t1 - t0, "save_ms": t2 - t1, "load_ms": t3 - t2, "from_cut_wall_ms": t4 - t3}


def measure(name):
    import graphcheck as GC
    clg = GC.clg
    p, cfg = GC.bench_program(name)
    g = GC.engine_program(p, drain=bool(cfg.get("drain")), max_drain=1_000_000)
    assert g.status() == 0
    rows = g.snapshot_table().rows
    done = np.nonzero(rows["complete_tick"] >= 0)[0]
    assert done.size, "the run completed no snapshot"
    sid = int(done[-1])
    # both graphs run one snapshot and no traffic: a ring of the deepest seeded channel and the
    # marker is enough (as in graph_restore_time.py)
    fifo = 16
    while fifo < int(rows["max_ch_msgs"][sid]) + 2:
        fifo *= 2
    fifo, delay = min(fifo, p.fifo_slots), p.delay_seed
    t0 = now()
    g.node_ids()
    ids_ms = now() - t0
    best = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cut.npz")
        for rep in range(REPS + 1):                        # (rep 0 warms both routes up)
            c, loaded, walls = checkpoint_route(g, clg, sid, fifo, delay, path)
            walls["build_ms"], walls["seed_ms"] = c.restore_time()
            r, walls["restore_wall_ms"] = restore_route(g, sid, fifo)
            walls["restore_build_ms"], walls["restore_seed_ms"] = r.restore_time()
            if rep == 0:
                info = c.seed_info
                assert info == r.seed_info == loaded.info()
                print(f"{name}: seed_info {info}", flush=True)
                file_bytes = os.path.getsize(path)
                upload = 4 * (loaded.tokens.size + 2 * loaded.channels + (0 if loaded.msg_tokens is None else loaded.msgs))
            else:
                for k, v in walls.items():
                    best[k] = v if k not in best else min(best[k], v)
            if rep < REPS:
                del c, r, loaded
    for x in (c, r):                                       # the same continuation on both
        x.start_snapshot_rank(0)
        x.drain()
        x.flush()
    assert c.status() == r.status() == 0
    assert c.checksums() == r.checksums() and c.counters() == r.counters()
    out = {"case": name, "nodes": g.num_nodes, "channels": g.num_channels, "snapshots": g.num_snapshots, "sid": sid,
           "reps": REPS, "seed_info": info, "ids_ms": round(ids_ms, 3), "file_bytes": file_bytes, "upload_bytes": upload}
    out.update({k: round(v, 4) for k, v in best.items()})
    out["device_bytes"] = {"from_cut": c.device_bytes, "restored": r.device_bytes}
    return out


def main(argv):
    if len(argv) == 2 and argv[0] == "--case":
        print(json.dumps(measure(argv[1])), flush=True)
        return 0
    lines = []
    for name in argv or list(LIMIT_S):
        # a process and a time limit per case: the parent never opens the GPU
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], timeout=LIMIT_S[name],
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}", file=sys.stderr)
            return r.returncode or 1
        for line in r.stdout.strip().splitlines()[:-1]:
            print(line, flush=True)
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
