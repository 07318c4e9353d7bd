"""Device time of the conditional analytics over instance sets (cl_iset, cl_snapshot_stats_in,
cl_snapshot_census_in) next to the unconditional calls of the same process and the host route they
replace, on C3 (8nodes-concurrent) at 2^20 and 2^17 instances, after flush + rerun (block-major
records, as in stats_time.py and census_time.py).  One JSON line per batch size, for snapshot id 0
and three sets of different density made from clauses on it:

  sets            "tail": completion tick >= the 99th percentile of snapshot_stats' tick_hist;
                  "half": completion tick <= its median; "all": the empty clause list (the whole sample)
  members         members of each set
  from_clauses_ms device ms of instance_set() (cl_select_time: evaluation into the set's bitmap and
                  the count), the fastest of reps + 1
  stats_in_ms, census_in_ms   device ms of snapshot_stats_in / snapshot_census_in over each set
  stats_ms, census_ms         the unconditional calls in the same process
  stats_in_over_stats, census_in_over_census   the ratios per set
  combine_ms, count_ms, list_ms   device ms of tail | half, len() and insts() of "half" (cl_iset_time)
  host_wall_ms    wall time of the route without sets, per set: select_instances ->
                  collect_snapshot_list -> numpy (per-node sums, minima and maxima, per-channel
                  message sums, distinct (tokens, message counts) rows); its per-node sums must equal
                  those of snapshot_stats_in
  set_wall_ms     wall time of instance_set() + snapshot_stats_in() + snapshot_census_in()
  host_over_set_wall   host_wall_ms / set_wall_ms per set

usage: python tools/iset_time.py [reps] [output file]   (default: 5 profiles/iset_c3.json)
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
    return min(fn() for _ in range(reps + 1))      # (the first call also uploads the token histories)


def host_route(sim, where):
    """Select, collect the matches' contents, reduce them in numpy."""
    t0 = time.perf_counter()
    sel = sim.select_instances(SID, where, ticks=True)
    tok, done, off, _ = sim.collect_snapshot_list(SID, sel.insts)
    msgs = np.diff(off).reshape(-1, sim.num_channels)
    node = (tok.sum(axis=0, dtype=np.int64), tok.min(axis=0), tok.max(axis=0))
    ch = msgs.sum(axis=0)
    classes = np.unique(np.hstack([tok, msgs.astype(np.int32)]), axis=0).shape[0]
    return (time.perf_counter() - t0) * 1e3, node, ch, classes


def measure(n, reps):
    sim = cl.ChandyLamportSim(n)
    sim.read_topology_file(os.path.join(DATA, TOP))
    sim.read_events_file(os.path.join(DATA, EVENTS))
    sim.flush()
    sim.rerun()
    sim.synchronize()

    def timed(call, clock):
        def once():
            call()
            return clock()
        return best_of(reps, once)

    st = sim.snapshot_stats(SID, tick_lo=0, tick_bins=256)
    cdf = np.cumsum(st.tick_hist)
    p99, p50 = (int(np.searchsorted(cdf, q * st.sample)) for q in (0.99, 0.5))
    wheres = {"tail": [("tick", None, p99, None)], "half": [("tick", None, None, p50)], "all": []}
    stats_ms = timed(lambda: sim.snapshot_stats(SID, tick_lo=0, tick_bins=256), sim.stats_time)
    census_ms = timed(lambda: sim.snapshot_census(SID), sim.census_time)
    line = {"config": "c3", "top": TOP, "events": EVENTS, "instances": n, "engine": sim.exec_engine(),
            "records_blocked": sim.records_blocked(), "snapshot": SID, "reps": reps, "sample": st.sample,
            "tick_p99": p99, "tick_p50": p50, "sets": list(wheres), "stats_ms": round(stats_ms, 4),
            "census_ms": round(census_ms, 4)}
    keys = ("members", "from_clauses_ms", "stats_in_ms", "census_in_ms", "host_wall_ms", "set_wall_ms")
    res = {k: [] for k in keys}
    sets = {}
    for name, where in wheres.items():
        made = []
        res["from_clauses_ms"].append(timed(lambda: made.append(sim.instance_set(SID, where)), sim.select_time))
        for s in made[:-1]:
            s.close()
        iset = sets[name] = made[-1]
        res["members"].append(len(iset))
        res["stats_in_ms"].append(timed(lambda: sim.snapshot_stats_in(SID, iset, tick_lo=0, tick_bins=256),
                                        sim.stats_time))
        res["census_in_ms"].append(timed(lambda: sim.snapshot_census_in(SID, iset), sim.census_time))

        def set_route():
            t0 = time.perf_counter()
            with sim.instance_set(SID, where) as s:
                got = sim.snapshot_stats_in(SID, s, tick_lo=0, tick_bins=256), sim.snapshot_census_in(SID, s)
            return (time.perf_counter() - t0) * 1e3, got

        set_wall, (cst, ccs) = min((set_route() for _ in range(reps + 1)), key=lambda r: r[0])
        host_wall, node, ch, _ = host_route(sim, where)             # (once: at 2^20 it moves hundreds of MB)
        assert cst.sample == ccs.sample == len(iset)
        assert np.array_equal(node[0], cst.node_sum) and np.array_equal(ch, cst.ch_msgs_sum)
        assert np.array_equal(node[1], cst.min_node) and np.array_equal(node[2], cst.max_node)
        res["host_wall_ms"].append(host_wall)
        res["set_wall_ms"].append(set_wall)
    assert res["members"][2] == st.sample and res["members"][0] == int(st.tick_hist[p99:].sum())
    assert sim.snapshot_stats_in(SID, sets["all"], tick_lo=0, tick_bins=256) == st
    for k in keys:
        line[k] = [round(v, 4) if isinstance(v, float) else v for v in res[k]]
    union = [None]
    line["combine_ms"] = round(timed(lambda: union.__setitem__(0, sets["tail"] | sets["half"]), sim.iset_time), 4)
    line["count_ms"] = round(timed(lambda: len(sets["half"]), sim.iset_time), 4)
    line["list_ms"] = round(timed(lambda: sets["half"].insts(max_out=n), sim.iset_time), 4)
    line["stats_in_over_stats"] = [round(x / stats_ms, 3) for x in res["stats_in_ms"]]
    line["census_in_over_census"] = [round(x / census_ms, 3) for x in res["census_in_ms"]]
    line["host_over_set_wall"] = [round(h / s, 1) for h, s in zip(res["host_wall_ms"], res["set_wall_ms"])]
    return line


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "iset_c3.json")
    lines = []
    for log2n in (20, 17):
        lines.append(measure(1 << log2n, reps))
        print(json.dumps(lines[-1]), flush=True)
    with open(path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
