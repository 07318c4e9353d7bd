"""Device time of the graph engine's node and channel profile over a snapshot range
(cl_graph_snapshot_profile) next to the summary table of the same run and to the host route it
replaces, one JSON line per case (the lines of profiles/graph_profile.json).  The two shapes of
tools/graph_table_time.py:

  c5_shape  tests/graphcheck.py's powerlaw_program(20000, 300, 256) with the drain;
  c4_shape  a 2^20-node random 8-out regular digraph under traffic with ONE snapshot at step 5,
            80 ticks and the drain.

  profile_ms      device time of the profile call's kernels over all snapshots with node rows and
                  entries (cl_graph_profile_time), the fastest of 6; profile_ms_all every repetition
  table_ms        device time of the table call's kernels on the same run, the fastest of 6; the
                  table and the profile calls alternate; table_ms_all every repetition
  bytes_needed    what the algorithm has to read, from the shapes: n_used x (8 x channels + 16 x
                  nodes) bytes of cursors and node records plus 4 bytes per recorded message where
                  the run keeps a payload history; floor_ms = bytes_needed over 8 TB/s
  host_channel_wall_ms   wall time of the route the channel side replaces: collect_sparse(payloads=
                  False) over the range and np.add.at / np.bincount per channel
  host_node_wall_ms      wall time of the route the latency columns replace: snapshot_tree with ticks
                  and numpy over the [snapshots, nodes] plane
  profile_wall_ms wall time of the profile call itself (launches, the entries and node rows to the
                  host), the fastest of 6

The host route and the profile must agree exactly on every channel's msgs and snaps and on every
node's lat_sum and lat_max; the tool asserts it.  Each case runs in a process of its own under a
time limit; a case that fails ends the tool.

usage: python tools/graph_profile_time.py [case ...]         (default: both, into profiles/graph_profile.json)
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

OUT = os.path.join(ROOT, "profiles", "graph_profile.json")
LIMIT_S = {"c5_shape": 420, "c4_shape": 300}
REPS = 6
PEAK_BYTES_PER_MS = 8e12 / 1e3


def measure(name):
    import graph_table_time as TT
    g, _ = {"c5_shape": TT.c5_shape, "c4_shape": TT.c4_shape}[name]()
    assert g.status() == 0
    n, e, s = g.num_nodes, g.num_channels, g.num_snapshots
    cap = g.snapshot_profile(nodes=False).entries.size       # (the exact capacity: one call per repetition)
    table_all, prof_all, wall_all = [], [], []
    for _ in range(REPS):                                    # alternating: the same clocks, the same neighbours
        tab = g.snapshot_table()
        table_all.append(g.table_time())
        t0 = time.perf_counter()
        pr = g.snapshot_profile(max_entries=cap)
        wall_all.append((time.perf_counter() - t0) * 1e3)
        prof_all.append(g.profile_time())
    rows = tab.rows
    used = pr.used != 0
    np.testing.assert_array_equal(used, rows["complete_tick"] >= 0)
    assert pr.word("msgs") == rows["rec_msgs"][used].sum() and pr.word("tokens") == rows["rec_tokens"][used].sum()
    assert pr.entries.size == cap == pr.word("active")
    # the host route of the channel side
    t0 = time.perf_counter()
    sp = g.collect_sparse(payloads=False)
    msgs = np.zeros(e, dtype=np.int64)
    np.add.at(msgs, sp.channel, sp.count)
    snaps = np.bincount(sp.channel, minlength=e)
    host_channel = (time.perf_counter() - t0) * 1e3
    mine = np.zeros((2, e), dtype=np.int64)
    mine[0, pr.entries["channel"]], mine[1, pr.entries["channel"]] = pr.entries["msgs"], pr.entries["snaps"]
    np.testing.assert_array_equal(mine[0], msgs)
    np.testing.assert_array_equal(mine[1], snaps)
    # the host route of the latency columns
    t0 = time.perf_counter()
    trees = g.snapshot_tree(ticks=True)
    lat = np.stack([t.tick for t in trees]).astype(np.int64) - g.snapshot_table().rows["start_tick"][:, None]
    lat_sum, lat_max = lat[used].sum(axis=0), lat[used].max(axis=0)
    host_node = (time.perf_counter() - t0) * 1e3
    np.testing.assert_array_equal(pr.node["lat_sum"], lat_sum)
    np.testing.assert_array_equal(pr.node["lat_max"], lat_max)
    n_used = int(used.sum())
    history = 0 if pr.word("unit_payloads") else 4 * pr.word("msgs")
    nbytes = n_used * (8 * e + 16 * n) + history
    best = min(prof_all)
    hot = pr.hottest(1)[0]
    return {"case": name, "nodes": n, "channels": e, "snapshots": s, "used": n_used, "reps": REPS,
            "profile_ms": round(best, 4), "profile_ms_all": [round(x, 4) for x in prof_all],
            "table_ms": round(min(table_all), 4), "table_ms_all": [round(x, 4) for x in table_all],
            "profile_wall_ms": round(min(wall_all), 3), "host_channel_wall_ms": round(host_channel, 1),
            "host_node_wall_ms": round(host_node, 1), "sparse_entries": int(sp.n_entries), "bytes_needed": nbytes,
            "floor_ms": round(nbytes / PEAK_BYTES_PER_MS, 4), "hbm_share": round(nbytes / best / PEAK_BYTES_PER_MS, 4),
            "device_bytes": g.device_bytes, "entries": int(pr.entries.size), "msgs": pr.word("msgs"),
            "max_msgs": pr.word("max_msgs"), "max_peak": pr.word("max_peak"), "max_snaps": pr.word("max_snaps"),
            "hottest": {f: int(hot[f]) for f in hot.dtype.names}}


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
