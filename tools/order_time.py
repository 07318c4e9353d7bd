"""Device and wall time of the ordering calls (cl_snapshot_topk, cl_snapshot_quantiles) next to
their host routes, on C3 (8nodes-concurrent) at 2^20 instances: flush, rerun (the records are then
block-major by slot), then in the same process REPS rounds over all cases in turn -- alternated, so
that a drift of the clocks falls on every case alike.  Per case the fastest round and the spread
(slowest - fastest) are reported.  One JSON line per size:

  terms           tick0      tick(0)                      inflight0  (0, "inflight")
                  five_sids  (s, "inflight") for the five snapshot ids s in turn, summed: the worst
                             case, every plane of the batch walked with every channel's cursor word
  calls           top16 / top4096   snapshot_topk(k, largest=True)
                  q5                snapshot_quantiles at 1/100, 1/4, 1/2, 3/4, 99/100
  <term>_<call>   device_ms (cl_order_time of the fastest round), stages_ms (value walk, select
                  passes, compaction), wall_ms (the call's wall time, copies and the host sort
                  included), spread_ms (device), wall_spread_ms
  host routes     ticks_argpartition16 / 4096_wall_ms, ticks_partition_q5_wall_ms: snapshot_ticks +
                  status, then a partition at the k-th largest and a sort of the rows at or above it
                  for the 16 (4096) latest, np.partition for the 5 quantiles
                  packed_inflight_wall_ms: collect_snapshot_packed of the whole batch + the same numpy
                  on the per-instance token sums; <route>_equal: its result equals the call's
  context         stats_ms, select_ms: one cl_snapshot_stats pass and one cl_select_instances call
                  (tick >= the 99/100 quantile) of the same run

usage: python tools/order_time.py [out.json] [log2 sizes ...]     (default profiles/order_c3.json)
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
REPS = 7
QS = [(1, 100), (1, 4), (1, 2), (3, 4), (99, 100)]
TERMS = {
    "tick0": [(0, "tick", None)],
    "inflight0": [(0, "inflight", None)],
    "five_sids": [(s, "inflight", None) for s in range(5)],
}
CALLS = {
    "top16": lambda sim, t: sim.snapshot_topk(t, 16, largest=True),
    "top4096": lambda sim, t: sim.snapshot_topk(t, 4096, largest=True),
    "q5": lambda sim, t: sim.snapshot_quantiles(t, QS),
}


def wall(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def order_top(vals, insts, k):
    """The k largest by (value descending, instance ascending): np.partition finds the k-th largest
    value, the rows at or above it are sorted."""
    if k < vals.size:
        cut = np.partition(vals, vals.size - k)[vals.size - k]
        pick = np.flatnonzero(vals >= cut)
    else:
        pick = np.arange(vals.size)
    order = np.lexsort((insts[pick], -vals[pick]))[:k]
    return insts[pick][order], vals[pick][order]


def host_quantiles(vals):
    ranks = [cl.quantile_rank(q, vals.size) for q in QS]
    return np.partition(vals, ranks)[ranks]


def measure(log2n):
    n = 1 << log2n
    sim = cl.ChandyLamportSim(n)
    sim.read_topology_file(os.path.join(DATA, TOP))
    n_sids = sim.read_events_file(os.path.join(DATA, EVENTS))
    sim.flush()
    sim.rerun()
    sim.synchronize()
    line = {"config": "c3", "top": TOP, "events": EVENTS, "instances": n, "engine": sim.exec_engine(),
            "records_blocked": sim.records_blocked(), "snapshots": n_sids, "reps": REPS}
    runs = {(t, c): [] for t in TERMS for c in CALLS}
    results = {}
    context = {"stats_ms": [], "select_ms": []}
    p99 = None
    for rep in range(REPS + 1):                       # (round 0 warms the scratch up and is dropped)
        for tname, terms in TERMS.items():
            for cname, call in CALLS.items():
                ms, stages, w = 0.0, np.zeros(3), 0.0
                for term in terms:
                    dw, res = wall(lambda: call(sim, term))
                    ms, stages, w = ms + sim.order_time(), stages + np.array(sim.order_time(stages=True)), w + dw
                    results[(tname, cname)] = res
                if rep:
                    runs[(tname, cname)].append((ms, stages, w))
        sim.snapshot_stats(0)
        if p99 is None:
            p99 = results[("tick0", "q5")].at((99, 100))
        sim.select_instances(0, [("tick", None, p99, None)])
        if rep:
            context["stats_ms"].append(sim.stats_time())
            context["select_ms"].append(sim.select_time())
    for (tname, cname), rs in runs.items():
        best = min(rs, key=lambda r: r[0])
        line[f"{tname}_{cname}"] = {
            "device_ms": round(best[0], 4), "stages_ms": [round(float(x), 4) for x in best[1]],
            "wall_ms": round(min(r[2] for r in rs), 4),
            "spread_ms": round(max(r[0] for r in rs) - best[0], 4),
            "wall_spread_ms": round(max(r[2] for r in rs) - min(r[2] for r in rs), 4)}
    for name, v in context.items():
        line[name] = round(min(v), 4)
        line[name.replace("_ms", "_spread_ms")] = round(max(v) - min(v), 4)
    top16, q5 = results[("tick0", "top16")], results[("tick0", "q5")]
    line["sample"] = top16.sample

    # ---- the host routes: the ticks, then the packed collect of the whole batch
    def ticks_route(k):
        ticks, status = sim.snapshot_ticks(0), sim.status()
        insts = np.flatnonzero((status == 0) & (ticks >= 0))
        return order_top(ticks[insts].astype(np.int64), insts, k)

    def ticks_quantiles():
        ticks, status = sim.snapshot_ticks(0), sim.status()
        return host_quantiles(ticks[(status == 0) & (ticks >= 0)].astype(np.int64))

    def packed_route():
        tok, done, off, msg = sim.collect_snapshot_packed(0, 0, n)
        sums = np.concatenate([[0], np.cumsum(msg, dtype=np.int64)])
        per_inst = off[::sim.num_channels]
        inflight = sums[per_inst[1:]] - sums[per_inst[:-1]]
        insts = np.flatnonzero((sim.status() == 0) & np.asarray(done).astype(bool))
        return order_top(inflight[insts], insts, 16), host_quantiles(inflight[insts])

    for name, f, want in (("ticks_argpartition16_wall_ms", lambda: ticks_route(16), (top16.insts, top16.values)),
                          ("ticks_argpartition4096_wall_ms", lambda: ticks_route(4096),
                           (results[("tick0", "top4096")].insts, results[("tick0", "top4096")].values)),
                          ("ticks_partition_q5_wall_ms", ticks_quantiles, q5.values)):
        best = None
        for _ in range(3):
            w, got = wall(f)
            best = w if best is None else min(best, w)
        line[name] = round(best, 4)
        line[name.replace("_wall_ms", "_equal")] = all(
            np.array_equal(a, b) for a, b in zip(got if isinstance(got, tuple) else (got,),
                                                 want if isinstance(want, tuple) else (want,)))
    best = None
    for _ in range(2):
        w, (top, qv) = wall(packed_route)
        best = w if best is None else min(best, w)
    want = results[("inflight0", "top16")]
    line["packed_inflight_wall_ms"] = round(best, 4)
    line["packed_inflight_equal"] = bool(np.array_equal(top[0], want.insts) and np.array_equal(top[1], want.values)
                                         and np.array_equal(qv, results[("inflight0", "q5")].values))
    line["ratios"] = {
        "ticks_host_over_top16_wall": round(line["ticks_argpartition16_wall_ms"] / line["tick0_top16"]["wall_ms"], 2),
        "ticks_host_over_q5_wall": round(line["ticks_partition_q5_wall_ms"] / line["tick0_q5"]["wall_ms"], 2),
        "packed_host_over_inflight_top16_wall": round(best / line["inflight0_top16"]["wall_ms"], 2),
        "tick0_top16_over_stats": round(line["tick0_top16"]["device_ms"] / line["stats_ms"], 3),
        "tick0_top16_over_select": round(line["tick0_top16"]["device_ms"] / line["select_ms"], 3),
    }
    return line


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "order_c3.json")
    sizes = [int(x) for x in sys.argv[2:]] or [20]
    lines = []
    for k in sizes:
        lines.append(json.dumps(measure(k)))
        print(lines[-1], flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
