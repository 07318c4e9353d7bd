"""Device time of the snapshot outcome census (cl_snapshot_census) next to the statistics pass and
the route it replaces, on C3 (8nodes-concurrent) at 2^20 and 2^17 instances: flush, rerun (the
records are then block-major by slot), then for every snapshot id, in the same process.  One JSON
line per size:

  census_ms       lds_slots = 0, the engine's workgroup table: the fastest of reps + 1 calls
                  (cl_census_time: init, key pass and gather kernels, HIP events)
  census_nolds_ms lds_slots = -1, every sample instance inserts into the global table
  census_cls_ms   lds_slots = 0 with class_of (adds the rank write-back and the lookup kernel)
  census_wall_ms  wall time of the lds_slots = 0 call, host sort and copies included
  n_classes       distinct snapshots per snapshot id; largest = the largest class's count
  stats_ms        cl_snapshot_stats on the same records (it reads the same bytes)
  collect_ms      the packed collect's kernels over the whole range
  unique_wall_ms  the status-quo route: wall time of collect_snapshot_packed (copies included)
                  plus grouping the instances' contents on the host with np.unique

usage: python tools/census_time.py [reps] [log2 sizes ...]     (the lines of profiles/census_c3.json)
"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
cl = importlib.import_module("chandy-lamport-distributed-snapshot-algorithm_amd")
DATA = os.path.join(ROOT, "tests", "golden", "test_data")
TOP, EVENTS = "8nodes.top", "8nodes-concurrent-snapshots.events"


def host_unique(sim, sid, out):
    """The route without the census: pack everything, copy it, group on the host.  An instance's
    content is its tokenMap row, its per-channel message counts and its messages; instances are
    grouped by the bytes of those (a dict over row bytes after np.unique of the fixed-width part)."""
    t0 = time.perf_counter()
    tok, done, off, msg = sim.collect_snapshot_packed(sid, out=out)
    ok = (sim.status() == 0) & done
    ch = sim.num_channels
    counts = np.diff(off).reshape(-1, ch)
    start = off[:-1:ch]
    total = counts.sum(axis=1)
    width = int(total.max()) if total.size else 0
    # fixed-width rows: tokens, per-channel counts, then the instance's messages, zero padded
    rows = np.zeros((tok.shape[0], tok.shape[1] + ch + width), dtype=np.int32)
    rows[:, :tok.shape[1]] = tok
    rows[:, tok.shape[1]:tok.shape[1] + ch] = counts
    for k in range(width):
        has = total > k
        rows[has, tok.shape[1] + ch + k] = msg[start[has] + k]
    _, cnt = np.unique(rows[ok], axis=0, return_counts=True)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, int(cnt.size), (tok, np.zeros(tok.shape[0], dtype=np.int32), off,
                                 msg.base if msg.base is not None else msg)


def measure(log2n, reps):
    n = 1 << log2n
    sim = cl.ChandyLamportSim(n)
    sim.read_topology_file(os.path.join(DATA, TOP))
    n_sids = sim.read_events_file(os.path.join(DATA, EVENTS))
    sim.flush()
    sim.rerun()
    sim.synchronize()
    res = {k: [] for k in ("census_ms", "census_nolds_ms", "census_cls_ms", "census_wall_ms", "n_classes", "largest",
                           "sample", "stats_ms", "collect_ms", "unique_wall_ms")}
    out = None
    for sid in range(n_sids):
        for name, kw in (("census_ms", {}), ("census_nolds_ms", {"lds_slots": -1}),
                         ("census_cls_ms", {"class_of": True})):
            best, wall = None, None
            for _ in range(reps + 1):       # (the first call also uploads the token histories)
                t0 = time.perf_counter()
                c = sim.snapshot_census(sid, **kw)
                w = (time.perf_counter() - t0) * 1e3
                ms = sim.census_time()
                best = ms if best is None else min(best, ms)
                wall = w if wall is None else min(wall, w)
            res[name].append(best)
            if name == "census_ms":
                res["census_wall_ms"].append(wall)
                res["n_classes"].append(c.n_classes)
                res["largest"].append(int(c.classes["count"][0]) if c.n_returned else 0)
                res["sample"].append(c.sample)
        best = None
        for _ in range(reps + 1):
            st = sim.snapshot_stats(sid)
            ms = sim.stats_time()
            best = ms if best is None else min(best, ms)
        res["stats_ms"].append(best)
        assert st.sample == c.sample
        best, wall = None, None
        for _ in range(2):                  # (a host grouping of 2^20 rows takes seconds)
            w, k, out = host_unique(sim, sid, out)
            ms = sim.collect_time()
            best = ms if best is None else min(best, ms)
            wall = w if wall is None else min(wall, w)
        assert k == c.n_classes, (k, c.n_classes)
        res["collect_ms"].append(best)
        res["unique_wall_ms"].append(wall)
    line = {"config": "c3", "top": TOP, "events": EVENTS, "instances": n, "engine": sim.exec_engine(),
            "records_blocked": sim.records_blocked(), "snapshots": n_sids, "reps": reps}
    for k, v in res.items():
        line[k] = [round(x, 4) if isinstance(x, float) else x for x in v]
    return line


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    sizes = [int(x) for x in sys.argv[2:]] or [20, 17]
    for k in sizes:
        print(json.dumps(measure(k, reps)), flush=True)
