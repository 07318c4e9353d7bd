"""Device time of the graph engine's marker-wave profile (cl_graph_snapshot_wave) and marker tree
(cl_graph_snapshot_tree) next to the summary table of the same run, one JSON line per case (the
lines of profiles/graph_wave.json).  The two shapes of tools/graph_table_time.py:

  c5_shape  tests/graphcheck.py's powerlaw_program(20000, 300, 256) with the drain;
  c4_shape  a 2^20-node random 8-out regular digraph under traffic with ONE snapshot at step 5,
            80 ticks and the drain.

  wave_ms        device time of the latency-only call's kernels (depth_bins=0), the fastest of 6
                 (cl_graph_wave_time); it reads the S x 16 n bytes of node records
  table_ms       device time of the table call's kernels on the same run in the same process, the
                 fastest of 6; the table and the latency-only wave calls alternate
  table_ms_all   every table timing of that loop: their spread is the noise wave_ms - table_ms is
                 read against (the latency-only pass reads a subset of what the table reads)
  wave_depth_ms  device time of the call with the depth on (link, doubling rounds, reduction; the
                 reads of the round flag in between included), the fastest of 6, and its `rounds`
  tree_ms        wall time of snapshot_tree with ticks (pack kernel and the 8 n bytes per snapshot
                 to the host), the fastest of 6
  depth_max, lat_max, created   of the profile, checked against the tree's depth() on the host for
                 the first and the last snapshot

Each case runs in a process of its own under a time limit; a case that fails ends the tool.

usage: python tools/graph_wave_time.py [case ...]            (default: both, into profiles/graph_wave.json)
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

OUT = os.path.join(ROOT, "profiles", "graph_wave.json")
LIMIT_S = {"c5_shape": 420, "c4_shape": 300}
REPS = 6
PEAK_BYTES_PER_MS = 8e12 / 1e3
SPEC = dict(lat_bins=64, lat_width=8)
DEPTH_BINS = 64


def measure(name):
    import graph_table_time as TT
    g, _ = {"c5_shape": TT.c5_shape, "c4_shape": TT.c4_shape}[name]()
    assert g.status() == 0
    n, s = g.num_nodes, g.num_snapshots
    table_all, wave_all = [], []
    for _ in range(REPS):                              # alternating: the same clocks, the same neighbours
        tab = g.snapshot_table()
        table_all.append(g.table_time())
        lat = g.snapshot_wave(depth_bins=0, **SPEC)
        wave_all.append(g.wave_time()[0])
    depth_all, rounds = [], 0
    for _ in range(REPS):
        w = g.snapshot_wave(depth_bins=DEPTH_BINS, **SPEC)
        ms, rounds = g.wave_time()
        depth_all.append(ms)
    tree_all = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        trees = g.snapshot_tree()
        tree_all.append((time.perf_counter() - t0) * 1e3)
    rows = tab.rows
    assert (w.broken == 0).all() and (lat.broken == 0).all()
    np.testing.assert_array_equal(w.created, rows["nodes_created"])
    np.testing.assert_array_equal(w.origin + w.word("lat_max"), rows["last_create_tick"])
    np.testing.assert_array_equal(w.lat_hist, lat.lat_hist)
    for t in (trees[0], trees[-1]):                    # the device's depth against the host's, from the tree
        d = t.depth()
        assert (d[t.created] >= 0).all()
        np.testing.assert_array_equal(np.bincount(np.minimum(d[t.created], DEPTH_BINS - 1), minlength=DEPTH_BINS),
                                      w.depth_hist[t.sid])
        assert int(d.max()) == int(w.word("depth_max")[t.sid])
    nbytes = s * 16 * n
    best = min(wave_all)
    return {"case": name, "nodes": n, "snapshots": s, "reps": REPS, "wave_ms": round(best, 4),
            "table_ms": round(min(table_all), 4), "table_ms_all": [round(x, 4) for x in table_all],
            "wave_ms_all": [round(x, 4) for x in wave_all], "wave_depth_ms": round(min(depth_all), 4),
            "rounds": rounds, "tree_ms": round(min(tree_all), 3), "bytes_read": nbytes,
            "hbm_share": round(nbytes / best / PEAK_BYTES_PER_MS, 4), "device_bytes": g.device_bytes,
            "created": int(w.created.sum()), "lat_max": int(w.word("lat_max").max()),
            "depth_max": int(w.word("depth_max").max())}


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
