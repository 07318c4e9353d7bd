"""Device time of the snapshot crosstab (cl_snapshot_crosstab) next to the statistics pass, which
reads the same planes, and the two routes it replaces, on C3 (8nodes-concurrent) at 2^20 instances.
One process: flush (instance-major records), measure; rerun (block-major by slot), measure again.
One JSON line per record layout:

  tables          "tick_same_sid": tick(0) x tick(0); "tick_two_sids": tick(0) x tick(4), 64 x 64,
                  neither reads records; "ch_tok_x_node": ch_tok 0 of sid 0 x node 4 of sid 4,
                  16 x 16, which stages both planes
  sample, cells, max_cell   joint sample, non-zero cells and the fullest cell of each table
  crosstab_ms     device ms of one call per table, the fastest of reps + 1 (cl_crosstab_time, HIP events)
  crosstab_wall_ms  wall time of snapshot_crosstab per table
  stats_ms        cl_snapshot_stats of snapshot 0 on the same records, in the same run
  crosstab_over_stats   crosstab_ms / stats_ms per table
  host_route      "tick_two_sids" through two collect_snapshot_packed calls plus numpy.histogram2d:
                  collect_ms (the packing kernels of both) and wall_ms (copies and numpy included);
                  its table must equal the crosstab's
  select_route    the same table through one conditional call per bin of axis a: instance_set(0,
                  tick == bin), then snapshot_stats_in of snapshot 4 for its tick histogram;
                  device_ms (cl_select_time + cl_stats_time summed over the bins_a pairs) and wall_ms
  host_over_crosstab_wall   host_route wall_ms / crosstab_wall_ms["tick_two_sids"]

and one line for the contended table of the 3-node scenario (ch_tok 0 of sid 0 x tick of sid 1,
16 x 64) at the same size: crosstab_ms per layout.  (The committed profile ends with one more line,
"3nodes-contended-variants": the same table with plain LDS atomics and with the equal cells of a
wave counted once, measured by this tool before the slower variant was removed; DESIGN.md.)

usage: python tools/crosstab_time.py [reps] [log2 instances] [output file]
       (default: 5 20 profiles/crosstab_c3.json)
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
TABLES = {
    "tick_same_sid": ((0, "tick", None, 0, 1, 64), (0, "tick", None, 0, 1, 64)),
    "tick_two_sids": ((0, "tick", None, 0, 1, 64), (4, "tick", None, 0, 1, 64)),
    "ch_tok_x_node": ((0, "ch_tok", 0, 0, 1, 16), (4, "node", 4, 0, 1, 16)),
}
# the contended case: the scenario of the census, select and crosstab tests
TOP3 = "3\nN1 30\nN2 30\nN3 30\nN1 N2\nN2 N1\nN1 N3\nN3 N1\nN2 N3\nN3 N2\n"
_ROUND = "send N1 N2 1\nsend N1 N2 2\nsend N2 N3 1\nsend N1 N3 1\nsend N3 N1 1\nsend N1 N2 1\ntick 1\n"
EVENTS3 = (_ROUND * 3 + "snapshot N3\n" + "send N1 N2 1\nsend N2 N1 1\ntick 1\n" * 2
           + "snapshot N1\nsend N1 N2 1\ntick 2\n")
CONTENDED = ((0, "ch_tok", 0, 0, 1, 16), (1, "tick", None, 0, 1, 64))


def best_of(reps, fn):
    best = None
    for _ in range(reps + 1):       # (the first call also uploads the token histories)
        v = fn()
        best = v if best is None else tuple(min(a, b) for a, b in zip(best, v))
    return best


def timed_crosstab(sim, a, b, reps):
    """(device ms, wall ms, the table) of snapshot_crosstab(a, b)."""
    got = {}

    def once():
        t0 = time.perf_counter()
        got["xt"] = sim.snapshot_crosstab(a, b)
        wall = (time.perf_counter() - t0) * 1e3
        return sim.crosstab_time(), wall

    ms, wall = best_of(reps, once)
    return ms, wall, got["xt"]


def host_route(sim, a, b, outs):
    """Two packed collects and numpy.histogram2d: the route without the crosstab."""
    t0 = time.perf_counter()
    ok = sim.status() == 0
    ticks, collect = [], 0.0
    for k, axis in enumerate((a, b)):
        tok, done, off, msg = sim.collect_snapshot_packed(axis[0], out=outs[k])
        collect += sim.collect_time()
        ticks.append(sim.snapshot_ticks(axis[0]))
        ok &= done
        outs[k] = (tok, np.zeros(tok.shape[0], dtype=np.int32), off, msg.base if msg.base is not None else msg)
    table = np.histogram2d(ticks[0][ok], ticks[1][ok], bins=(a[5], b[5]), range=((0, a[5]), (0, b[5])))[0]
    return (time.perf_counter() - t0) * 1e3, collect, table.astype(np.int64)


def select_route(sim, a, b):
    """One conditional statistics pass of b's snapshot per bin of axis a."""
    t0 = time.perf_counter()
    device, table = 0.0, np.zeros((a[5], b[5]), dtype=np.int64)
    for ia in range(a[5]):
        with sim.instance_set(a[0], [("tick", None, ia, ia)]) as iset:
            device += sim.select_time()
            table[ia] = sim.snapshot_stats_in(b[0], iset, tick_lo=0, tick_bins=b[5]).tick_hist
            device += sim.stats_time()
    return (time.perf_counter() - t0) * 1e3, device, table


def measure(sim, n, reps):
    def stats():
        sim.snapshot_stats(0, tick_lo=0, tick_bins=256)
        return (sim.stats_time(),)

    stats_ms = best_of(reps, stats)[0]
    line = {"config": "c3", "top": TOP, "events": EVENTS, "instances": n, "engine": sim.exec_engine(),
            "records_blocked": sim.records_blocked(), "reps": reps, "tables": list(TABLES),
            "stats_ms": round(stats_ms, 4)}
    res = {k: [] for k in ("sample", "cells", "max_cell", "crosstab_ms", "crosstab_wall_ms")}
    xts = {}
    for name, (a, b) in TABLES.items():
        ms, wall, xt = timed_crosstab(sim, a, b, reps)
        xts[name] = xt
        res["sample"].append(xt.sample)
        res["cells"].append(int((xt.table > 0).sum()))
        res["max_cell"].append(int(xt.table.max()))
        res["crosstab_ms"].append(round(ms, 4))
        res["crosstab_wall_ms"].append(round(wall, 4))
    line.update(res)
    line["crosstab_over_stats"] = [round(x / stats_ms, 3) for x in res["crosstab_ms"]]
    a, b = TABLES["tick_two_sids"]
    outs, walls, collects = [None, None], [], []
    for _ in range(2):                  # (a collect of 2^20 instances moves hundreds of MB)
        wall, collect, table = host_route(sim, a, b, outs)
        walls.append(wall), collects.append(collect)
    assert np.array_equal(table, xts["tick_two_sids"].table)
    line["host_route"] = {"collect_ms": round(min(collects), 4), "wall_ms": round(min(walls), 4)}
    wall, device, table = select_route(sim, a, b)
    assert np.array_equal(table, xts["tick_two_sids"].table)
    line["select_route"] = {"calls": a[5], "device_ms": round(device, 4), "wall_ms": round(wall, 4)}
    line["host_over_crosstab_wall"] = round(min(walls) / res["crosstab_wall_ms"][1], 1)
    return line


def contended(n, reps):
    sim = cl.ChandyLamportSim(n)
    sim.read_topology_text(TOP3)
    sim.read_events_text(EVENTS3)
    sim.flush()
    line = {"config": "3nodes-contended", "instances": n, "reps": reps, "table": "ch_tok_0_sid0_x_tick_sid1",
            "layouts": ["instance-major", "block-major"], "crosstab_ms": []}
    for layout in range(2):
        if layout:
            sim.rerun()
            sim.synchronize()
        assert sim.records_blocked() == bool(layout)
        ms, _, xt = timed_crosstab(sim, *CONTENDED, reps)
        line["crosstab_ms"].append(round(ms, 4))
        line["sample"], line["cells"], line["max_cell"] = xt.sample, int((xt.table > 0).sum()), int(xt.table.max())
    return line


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    log2n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "crosstab_c3.json")
    n = 1 << log2n
    sim = cl.ChandyLamportSim(n)
    sim.read_topology_file(os.path.join(DATA, TOP))
    sim.read_events_file(os.path.join(DATA, EVENTS))
    sim.flush()
    lines = [measure(sim, n, reps)]
    sim.rerun()
    sim.synchronize()
    lines.append(measure(sim, n, reps))
    del sim
    lines.append(contended(n, reps))
    with open(path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
