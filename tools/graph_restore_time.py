"""Time of the graph engine's restore (cl_graph_restore: the seed built and pushed by kernels)
next to the host route it replaces, one JSON line per case (the lines of
profiles/graph_restore.json).  The cases are bench.py's graph configs c4 and c5 (tests/graphcheck.py
bench_program); the snapshot restored is the last one the run completed.

  seed_info           cl_graph_seed_info of the restored graph (printed, and in the line)
  build_ms            device time of the restore call's kernels (scan, write, offsets, sums)
  seed_ms             device time of the seed kernel of the restored graph's run
  restore_wall_ms     wall time of restore(sid) + flush(): a graph that stands in the cut
  host_wall_ms        wall time of the host route to the same state with calls that need no
                      restore: collect_sparse(sid) with the token plane, a new GraphSim,
                      set_topology with T', M x send_tokens_rank, flush; host_parts_ms splits it
  rerun_ms            device time of rerun() of the restored graph with a continuation (a snapshot
                      at rank 0 and the drain), of the host route's graph with the same
                      continuation, and of the source run
Both routes are warmed up once, then alternate REPS times; the fastest of each is kept.  Wall
times are taken around calls that end with a stream synchronise.  The two graphs' counters and
checksums after the continuation are checked to be equal.  Each case runs in a process of its own
under a time limit; a case that fails ends the tool.

usage: python tools/graph_restore_time.py [c4|c5 ...]        (default: both, into profiles/graph_restore.json)
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

OUT = os.path.join(ROOT, "profiles", "graph_restore.json")
LIMIT_S = {"c4": 420, "c5": 540}
REPS = 3


def now():
    return time.perf_counter() * 1e3


def gpu_route(g, sid, fifo):
    t0 = now()
    r = g.restore(sid)
    r.set_limits(fifo, 1, 1_000_000)        # (one snapshot of its own: small snapshot planes)
    r.flush()
    return r, now() - t0


def host_route(g, GraphSim, sid, fifo, src, dst, width, delay):
    t0 = now()
    s = g.collect_sparse(sid, sid + 1, tokens=True)
    ch, cnt, _ = s.entries(sid)
    tok = s.tokens[0].astype(np.int64)
    per_ch = np.add.reduceat(s.msg_tokens.astype(np.int64), s.msg_offsets[:-1]) if ch.size else np.zeros(0, np.int64)
    tok += np.bincount(src[ch], weights=per_ch, minlength=tok.size).astype(np.int64)
    t1 = now()
    b = GraphSim(fifo_slots=fifo, max_snapshots=1, max_drain_ticks=1_000_000)
    b.set_topology(tok, src, dst, id_width=width)
    b.set_delay_hash(delay)
    t2 = now()
    a, d, m = np.repeat(src[ch], cnt).tolist(), np.repeat(dst[ch], cnt).tolist(), s.msg_tokens.tolist()
    send = b.send_tokens_rank
    for i in range(len(m)):
        send(a[i], d[i], m[i])
    t3 = now()
    b.flush()
    t4 = now()
    return b, t4 - t0, {"collect": t1 - t0, "topology": t2 - t1, "sends": t3 - t2, "flush": t4 - t3}


def rerun_ms(g):
    g.run_time()
    g.rerun()
    return g.run_time()[0]


def measure(name):
    import graphcheck as GC
    p, cfg = GC.bench_program(name)
    g = GC.engine_program(p, drain=bool(cfg.get("drain")), max_drain=1_000_000)
    assert g.status() == 0
    rows = g.snapshot_table().rows
    done = np.nonzero(rows["complete_tick"] >= 0)[0]
    assert done.size, "the run completed no snapshot"
    sid = int(done[-1])
    src, dst = g.channels()
    # both routes' graphs run one snapshot and no traffic: a ring of the deepest seeded channel
    # and the marker is enough (c5's 8,192 slots per channel would be 69 GB for each of them)
    fifo = 16
    while fifo < int(rows["max_ch_msgs"][sid]) + 2:
        fifo *= 2
    fifo, width, delay = min(fifo, p.fifo_slots), p.width(), p.delay_seed
    best = {}
    parts = None
    for rep in range(REPS + 1):                        # (rep 0 warms both routes up)
        r, wr = gpu_route(g, sid, fifo)
        build, seed = r.restore_time()
        b, wb, pt = host_route(g, GC.clg.GraphSim, sid, fifo, src, dst, width, delay)
        if rep == 0:
            info = r.seed_info
            print(f"{name}: seed_info {info}", flush=True)
        else:
            for k, v in (("build_ms", build), ("seed_ms", seed), ("restore_wall_ms", wr), ("host_wall_ms", wb)):
                best[k] = v if k not in best else min(best[k], v)
            if parts is None or wb == best["host_wall_ms"]:
                parts = pt
        if rep < REPS:
            del r, b
    for x in (r, b):                                   # the same continuation on both
        x.start_snapshot_rank(0)
        x.drain()
        x.flush()
    assert r.status() == b.status() == 0
    assert r.counters() == b.counters() and r.checksums() == b.checksums()
    out = {"case": name, "nodes": g.num_nodes, "channels": g.num_channels, "snapshots": g.num_snapshots, "sid": sid,
           "reps": REPS, "seed_info": info}
    out.update({k: round(v, 4) for k, v in best.items()})
    out["host_parts_ms"] = {k: round(v, 3) for k, v in parts.items()}
    out["rerun_ms"] = {"restored": round(rerun_ms(r), 4), "host_route": round(rerun_ms(b), 4),
                       "source": round(rerun_ms(g), 4)}
    out["device_bytes"] = {"restored": r.device_bytes, "host_route": b.device_bytes}
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
