"""Device and wall time of the graph engine's sparse packed collect (cl_graph_collect_sparse)
next to the route it replaces, one JSON line per case (the lines of profiles/graph_sparse.json).
The cases are those of tools/graph_table_time.py:

  c5_shape  tests/graphcheck.py's powerlaw_program(20000, 300, 256) with the drain;
  c4_shape  a 2^20-node random 8-out regular digraph under traffic with ONE snapshot at step 5,
            80 ticks and the drain.

  sparse_ms           device time of the kernels of one fetch with payloads, without the token
                      plane, the fastest of 6 (cl_graph_sparse_time: count + scan + write)
  sparse_tokens_ms    the same with the token plane (tokens=True)
  sparse_wall_ms      wall time of GraphSim.collect_sparse() over all snapshot ids (the sizing
                      call, the fetch, the copies), the fastest of 6
  sparse_tokens_wall_ms  the same with tokens=True: everything collect_arrays returns
  collect_wall_ms     wall time of the loop it replaces: collect_arrays over the same snapshot ids
  n_entries, n_msgs   what the snapshots recorded
  bytes_out           bytes the fetch copies to the host (head, entries, payloads), and
  bytes_out_tokens    with the token plane

Every snapshot's digest from the sparse contents is checked against the summary table's.
Each case runs in a process of its own under a time limit; a case that fails ends the tool.

usage: python tools/graph_sparse_time.py [case ...]          (default: both, into profiles/graph_sparse.json)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from graph_table_time import c4_shape, c5_shape  # noqa: E402  (also puts the repository on sys.path)

OUT = os.path.join(ROOT, "profiles", "graph_sparse.json")
LIMIT_S = {"c5_shape": 420, "c4_shape": 300}
REPS = 6


def timed(g, **kw):
    """(SparseSnapshots, fastest device ms, fastest wall ms) of REPS collect_sparse calls."""
    best, wall, s = None, None, None
    for _ in range(REPS):
        t0 = time.perf_counter()
        s = g.collect_sparse(**kw)
        w = (time.perf_counter() - t0) * 1e3
        ms = g.sparse_time()
        best = ms if best is None else min(best, ms)
        wall = w if wall is None else min(wall, w)
    return s, best, wall


def measure(name):
    g, _ = {"c5_shape": c5_shape, "c4_shape": c4_shape}[name]()
    assert g.status() == 0
    n, e, ns = g.num_nodes, g.num_channels, g.num_snapshots
    s, ms, wall = timed(g)
    st, ms_tok, wall_tok = timed(g, tokens=True)
    rows = g.snapshot_table().rows
    done = rows["complete_tick"] >= 0
    assert (s.complete != 0).tolist() == done.tolist()
    assert s.n_msgs == int(rows["rec_msgs"].sum()) and s.n_entries == int(rows["rec_channels"].sum())
    for sid in range(ns):
        if done[sid]:
            assert st.digest(sid, n, e) == rows["digest"][sid], sid
    t0 = time.perf_counter()
    msgs = 0
    for sid in range(ns):
        if done[sid]:
            _, off, _ = g.collect_arrays(sid)
            msgs += int(off[-1])
    collect_wall = (time.perf_counter() - t0) * 1e3
    assert msgs == s.n_msgs
    # (without a payload history every payload is 1 and none is copied)
    unit = int(g._collect_sparse(0, ns)[1]["unit_payloads"])
    nbytes = 64 + 4 * ns + 8 * (ns + 1) + 8 * s.n_entries + (0 if unit else 4 * s.n_msgs)
    return {"case": name, "nodes": n, "channels": e, "snapshots": ns, "completed": int(done.sum()), "reps": REPS,
            "sparse_ms": round(ms, 4), "sparse_tokens_ms": round(ms_tok, 4), "sparse_wall_ms": round(wall, 3),
            "sparse_tokens_wall_ms": round(wall_tok, 3), "collect_wall_ms": round(collect_wall, 1),
            "n_entries": s.n_entries, "n_msgs": s.n_msgs, "bytes_out": nbytes, "bytes_out_tokens": nbytes + 4 * ns * n,
            "unit_payloads": unit, "walk": "gather"}


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
