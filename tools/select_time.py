"""Device time of the instance selection (cl_select_instances) next to the statistics pass, which
reads the same planes, and the route it replaces, on C3 (8nodes-concurrent) at 2^20 instances.
One process: flush (instance-major records), measure; rerun (block-major by slot), measure again.
One JSON line per record layout, for snapshot id 0:

  selections      "tick_p99": completion tick >= the 99th percentile of snapshot_stats' tick_hist;
                  "msgs_max": recorded messages == max_msgs; "all": the empty clause list
  n_match         matches of each selection
  select_ms       device ms of one call that counts and fetches every match, the fastest of
                  reps + 1 (cl_select_time: both stages, HIP events)
  evaluate_ms, compact_ms   its two stages (cl_select_stage_times)
  select_wall_ms  wall time of select_instances(max_out=None): a count-only call, then the fetch
  stats_ms        cl_snapshot_stats on the same records
  collect_ms      the packed collect's kernels over the whole range
  filter_wall_ms  the status-quo route to "msgs_max": wall time of collect_snapshot_packed (copies
                  included) plus the numpy filter over the offsets; its result must equal the
                  selection's
  select_over_stats        select_ms / stats_ms per selection
  filter_over_select_wall  filter_wall_ms / select_wall_ms["msgs_max"]

usage: python tools/select_time.py [reps] [log2 instances] [output file]
       (default: 5 20 profiles/select_c3.json)
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
SID = 0


def best_of(reps, fn):
    best = None
    for _ in range(reps + 1):       # (the first call also uploads the token histories)
        v = fn()
        best = v if best is None else tuple(min(a, b) for a, b in zip(best, v))
    return best


def host_filter(sim, max_msgs, out):
    """The route without the selection: pack everything, copy it, filter on the host."""
    t0 = time.perf_counter()
    tok, done, off, msg = sim.collect_snapshot_packed(SID, out=out)
    ok = (sim.status() == 0) & done
    msgs = np.diff(off).reshape(-1, sim.num_channels).sum(axis=1)
    insts = np.flatnonzero(ok & (msgs == max_msgs))
    wall = (time.perf_counter() - t0) * 1e3
    return wall, insts, (tok, np.zeros(tok.shape[0], dtype=np.int32), off, msg.base if msg.base is not None else msg)


def measure(sim, n, reps):
    def stats():
        st = sim.snapshot_stats(SID, tick_lo=0, tick_bins=256)
        return st, sim.stats_time()

    st = stats()[0]
    stats_ms = best_of(reps, lambda: (stats()[1],))[0]
    cdf = np.cumsum(st.tick_hist)
    p99 = int(np.searchsorted(cdf, 0.99 * st.sample))
    wheres = {"tick_p99": [("tick", None, p99, None)], "msgs_max": [("msgs", None, st.max_msgs, st.max_msgs)],
              "all": []}
    line = {"config": "c3", "top": TOP, "events": EVENTS, "instances": n, "engine": sim.exec_engine(),
            "records_blocked": sim.records_blocked(), "snapshot": SID, "reps": reps, "sample": st.sample,
            "tick_p99": p99, "max_msgs": st.max_msgs, "selections": list(wheres), "stats_ms": round(stats_ms, 4)}
    res = {k: [] for k in ("n_match", "select_ms", "evaluate_ms", "compact_ms", "select_wall_ms")}
    sels = {}
    for name, where in wheres.items():
        def device():
            sim.select_instances(SID, where, max_out=n)
            return (sim.select_time(),) + sim.select_time(stages=True)

        def wall():
            t0 = time.perf_counter()
            sels[name] = sim.select_instances(SID, where)
            return ((time.perf_counter() - t0) * 1e3,)

        ms, ev, co = best_of(reps, device)
        w = best_of(reps, wall)[0]
        res["n_match"].append(sels[name].n_match)
        for k, v in (("select_ms", ms), ("evaluate_ms", ev), ("compact_ms", co), ("select_wall_ms", w)):
            res[k].append(round(v, 4))
    assert sels["all"].n_match == st.sample and sels["tick_p99"].n_match == int(st.tick_hist[p99:].sum())
    out, walls, collect = None, [], []
    for _ in range(2):                  # (a collect of 2^20 instances moves hundreds of MB)
        w, insts, out = host_filter(sim, st.max_msgs, out)
        walls.append(w)
        collect.append(sim.collect_time())
    assert np.array_equal(insts, sels["msgs_max"].insts)
    line.update(res)
    line["collect_ms"] = round(min(collect), 4)
    line["filter_wall_ms"] = round(min(walls), 4)
    line["select_over_stats"] = [round(x / stats_ms, 3) for x in res["select_ms"]]
    line["filter_over_select_wall"] = round(min(walls) / res["select_wall_ms"][1], 1)
    return line


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    log2n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "select_c3.json")
    n = 1 << log2n
    sim = cl.ChandyLamportSim(n)
    sim.read_topology_file(os.path.join(DATA, TOP))
    sim.read_events_file(os.path.join(DATA, EVENTS))
    sim.flush()
    lines = [measure(sim, n, reps)]
    sim.rerun()
    sim.synchronize()
    lines.append(measure(sim, n, reps))
    with open(path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
