"""Device time of the tuple group-by (cl_snapshot_groups) next to its yardsticks, on C3
(8nodes-concurrent) at 2^20 and 2^17 instances: flush, rerun (the records are then block-major by
slot), then in the same process, per term list, the device-ms breakdown of the fastest of 6 calls.
One JSON line per size:

  lists           ticks2  tick(0), tick(4)              ticks5  the five completion ticks
                  nodes8  the 8 node words of sid 0     keys2   key(0), key(4)
  <list>_ms       cl_groups_time of the fastest call; <list>_stages_ms its breakdown (table
                  initialisation, key pass, gather, group_of, values); <list>_wall_ms the call's wall
                  time, host sort and copies included; <list>_groups the number of groups
  census_ms       cl_snapshot_census of sid 0 on the same records: the yardstick of a one-plane record
                  group-by (the same walk and table, plus the term loop)
  crosstab_ms     cl_snapshot_crosstab of tick(0) x tick(4): with the table initialisation, the yardstick
                  of a tick-only group-by
  host_wall_ms    the route without the call, for the five ticks: five snapshot_ticks plus
                  np.unique(axis=0) on the host; its groups must equal the call's
  ratios          nodes8_ms / census_ms, ticks2_ms / crosstab_ms, ticks2 key pass / crosstab_ms,
                  host_wall_ms / ticks5_wall_ms

usage: python tools/groups_time.py [out.json] [log2 sizes ...]     (default profiles/groups_c3.json)
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
CALLS = 6

LISTS = {
    "ticks2": [(0, "tick", None), (4, "tick", None)],
    "ticks5": [(s, "tick", None) for s in range(5)],
    "nodes8": [(0, "node", v) for v in range(8)],
    "keys2": [(0, "key", None), (4, "key", None)],
}


def fastest(call, device_ms):
    """(device ms, wall ms, result, extra) of the call with the least device time among CALLS."""
    best = None
    for _ in range(CALLS):
        t0 = time.perf_counter()
        res = call()
        wall = (time.perf_counter() - t0) * 1e3
        ms, extra = device_ms()
        if best is None or ms < best[0]:
            best = (ms, wall, res, extra)
    return best


def host_route(sim, n_sids):
    """Five snapshot_ticks and np.unique(axis=0): (wall ms, tuples, counts)."""
    t0 = time.perf_counter()
    ticks = np.stack([sim.snapshot_ticks(s) for s in range(n_sids)], axis=1)
    pick = (sim.status() == 0) & (ticks >= 0).all(axis=1)
    tuples, counts = np.unique(ticks[pick], axis=0, return_counts=True)
    return (time.perf_counter() - t0) * 1e3, tuples, counts


def measure(log2n):
    n = 1 << log2n
    sim = cl.ChandyLamportSim(n)
    sim.read_topology_file(os.path.join(DATA, TOP))
    n_sids = sim.read_events_file(os.path.join(DATA, EVENTS))
    sim.flush()
    sim.rerun()
    sim.synchronize()
    line = {"config": "c3", "top": TOP, "events": EVENTS, "instances": n, "engine": sim.exec_engine(),
            "records_blocked": sim.records_blocked(), "snapshots": n_sids, "calls": CALLS}
    got = {}
    for name, terms in LISTS.items():
        ms, wall, g, stages = fastest(lambda: sim.snapshot_groups(terms, max_groups=n),
                                      lambda: (sim.groups_time(), sim.groups_time(stages=True)))
        got[name] = g
        line[name + "_ms"], line[name + "_wall_ms"] = round(ms, 4), round(wall, 4)
        line[name + "_stages_ms"] = [round(x, 4) for x in stages]
        line[name + "_groups"], line[name + "_sample"] = g.n_groups, g.sample
    census_ms, _, census, _ = fastest(lambda: sim.snapshot_census(0), lambda: (sim.census_time(), None))
    line["census_ms"], line["census_classes"] = round(census_ms, 4), census.n_classes
    a, b = (0, "tick", None, 0, 1, 64), (4, "tick", None, 0, 1, 64)
    xt_ms, _, xt, _ = fastest(lambda: sim.snapshot_crosstab(a, b), lambda: (sim.crosstab_time(), None))
    assert int((xt.table > 0).sum()) == got["ticks2"].n_groups and xt.sample == got["ticks2"].sample
    line["crosstab_ms"] = round(xt_ms, 4)
    host_ms, tuples, counts = min((host_route(sim, n_sids) for _ in range(2)), key=lambda r: r[0])
    g = got["ticks5"]
    assert g.n_returned == g.n_groups == counts.size
    order = np.lexsort(g.values.T[::-1])                            # the call's groups in np.unique's row order
    assert np.array_equal(g.values[order], tuples) and np.array_equal(g.groups["count"][order], counts)
    line["host_wall_ms"] = round(host_ms, 4)
    line["ratios"] = {
        "nodes8_over_census": round(line["nodes8_ms"] / census_ms, 3),
        "ticks2_over_crosstab": round(line["ticks2_ms"] / xt_ms, 3),
        "ticks2_keypass_over_crosstab": round(line["ticks2_stages_ms"][1] / xt_ms, 3),
        "host_over_ticks5_wall": round(host_ms / line["ticks5_wall_ms"], 1),
    }
    return line


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "groups_c3.json")
    sizes = [int(x) for x in sys.argv[2:]] or [20, 17]
    lines = []
    for k in sizes:
        lines.append(json.dumps(measure(k)))
        print(lines[-1], flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
