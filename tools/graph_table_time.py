"""Device time of the graph engine's per-snapshot summary table (cl_graph_snapshot_table) next
to the route it replaces, one JSON line per case (the lines of profiles/graph_table.json):

  c5_shape  tests/graphcheck.py's powerlaw_program(20000, 300, 256) with the drain -- the shape
            of tests/golden/graph_runs.json c5_shape_20k_256, whose completion ticks and
            per-snapshot digests the table is checked against here;
  c4_shape  a 2^20-node random 8-out regular digraph under traffic with ONE snapshot at step 5,
            80 ticks and the drain (BASELINE config 4's shape, drained so the snapshot completes).

  table_ms        device time of the table call's kernels, the fastest of 6 (cl_graph_table_time)
  table_wall_ms   wall time of that call (flush check, launches, the n_sids x 128 B copy)
  collect_wall_ms wall time of the loop it replaces: collect_arrays over the same snapshot ids
  checksums_wall_ms  wall time of checksums() (the run-wide sums over the same planes)
  bytes_read      S (16 n + 8 e) bytes of node records and cursors, plus 4 e of the in-position
                  -> channel map per snapshot (unit payloads: no payload history); incomplete
                  snapshots read their node records only
  hbm_share       bytes_read / table_ms as a share of 8 TB/s

Each case runs in a process of its own under a time limit; a case that fails ends the tool.

usage: python tools/graph_table_time.py [case ...]            (default: both, into profiles/graph_table.json)
"""
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

OUT = os.path.join(ROOT, "profiles", "graph_table.json")
LIMIT_S = {"c5_shape": 420, "c4_shape": 300}
REPS = 6
PEAK_BYTES_PER_MS = 8e12 / 1e3


def c5_shape():
    import graphcheck as GC
    p = GC.powerlaw_program(20000, 300, 256, fifo_slots=512)
    g = GC.engine_program(p, drain=True, max_drain=100000)
    with open(os.path.join(ROOT, "tests", "golden", "graph_runs.json")) as f:
        fx = json.load(f)["runs"]["c5_shape_20k_256"]["summary"]
    return g, {"ctick": fx["ctick"], "digest": fx["digest"]}


def c4_shape():
    clg = importlib.import_module("chandy-lamport-distributed-snapshot-algorithm_amd.graph")
    n = 1 << 20
    g = clg.GraphSim(fifo_slots=16, max_snapshots=1)
    g.generate_regular(n, 8, 100, 20240)
    g.set_delay_hash(20241)
    g.set_traffic(20242, 1 << 30, 80)
    for k in range(80):
        if k == 5:
            g.start_snapshot_rank(n // 3)
        g.Tick(1)
    g.drain()
    g.flush()
    return g, None


def measure(name):
    g, fixture = {"c5_shape": c5_shape, "c4_shape": c4_shape}[name]()
    assert g.status() == 0
    n, e, s = g.num_nodes, g.num_channels, g.num_snapshots
    best, wall = None, None
    for _ in range(REPS):
        t0 = time.perf_counter()
        tab = g.snapshot_table()
        w = (time.perf_counter() - t0) * 1e3
        ms = g.table_time()
        best = ms if best is None else min(best, ms)
        wall = w if wall is None else min(wall, w)
    rows = tab.rows
    t0 = time.perf_counter()
    sums = g.checksums()
    sums_wall = (time.perf_counter() - t0) * 1e3
    assert tab.digest_sum() == sums["digest"]
    assert int(tab.cut_residual(100 * n).sum()) == sums["cut_residual"] == 0
    if fixture:
        assert rows["complete_tick"].tolist() == fixture["ctick"]
        assert rows["digest"].tolist() == fixture["digest"]
    done = rows["complete_tick"] >= 0
    t0 = time.perf_counter()
    msgs = 0
    for sid in range(s):
        if done[sid]:
            _, off, _ = g.collect_arrays(sid)
            msgs += int(off[-1])
    collect_wall = (time.perf_counter() - t0) * 1e3
    assert msgs == int(rows["rec_msgs"].sum())
    nbytes = s * 16 * n + int(done.sum()) * 12 * e
    return {"case": name, "nodes": n, "channels": e, "snapshots": s, "completed": int(done.sum()), "reps": REPS,
            "table_ms": round(best, 4), "table_wall_ms": round(wall, 3), "collect_wall_ms": round(collect_wall, 1),
            "checksums_wall_ms": round(sums_wall, 3), "bytes_read": nbytes,
            "hbm_share": round(nbytes / best / PEAK_BYTES_PER_MS, 4),
            "max_latency": int(tab.latency.max()), "max_spread": int(tab.spread.max()),
            "rec_msgs": int(rows["rec_msgs"].sum())}


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
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
