"""Cost of making a fresh batch's Go delay rows with the host generator and with the device
generator (cl_set_delay_generator), on C3 (8nodes-concurrent: 97 draws, rows of 112 bytes) at 2^20
and 2^17 instances.  A small warm-up batch first initialises the device and compiles the exec
kernel for the topology, so neither is counted.  Per size and generator, `reps` fresh sims; one
JSON line per size:

  host_gen_ms       host generator: wall time of the sequential generators (up to 16 threads) and
                    the copy of the plane to the device (cl_delay_gen_time host_ms), fastest rep
  device_gen_ms     device generator: the kernel, from HIP events around it (cl_delay_gen_time
                    device_ms), fastest rep; device_patch_ms the host time spent on rejected rows
                    in that rep, patched_rows their number
  ratio             host_gen_ms / (device_gen_ms + device_patch_ms)
  first_flush_ms    wall time of the first flush() of a fresh sim under each generator (rows, layout,
                    allocations, the probe run of the program), fastest rep
  exec_ms           the exec kernel of that flush (cl_last_kernel_ms), for scale
  plane_bytes       the rows' plane: what the host generator copies and the device generator does not

usage: python tools/delaygen_time.py [reps] [log2 sizes ...]      (the lines of profiles/delaygen_c3.json)
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


def fresh(n, generator):
    sim = cl.ChandyLamportSim(n)
    sim.set_delay_generator(generator)
    sim.read_topology_file(os.path.join(DATA, TOP))
    sim.read_events_file(os.path.join(DATA, EVENTS))
    t0 = time.perf_counter()
    sim.flush()
    wall = (time.perf_counter() - t0) * 1e3
    assert sim.delay_generator == generator
    device_ms, host_ms, patched = sim.delay_gen_time()
    return sim, dict(wall=wall, device_ms=device_ms, host_ms=host_ms, patched=patched, exec_ms=sim.last_kernel_ms())


def measure(log2n, reps):
    n = 1 << log2n
    runs = {"host": [], "device": []}
    sums = {}
    for _ in range(reps):
        for g in runs:
            sim, r = fresh(n, g)
            runs[g].append(r)
            sums[g] = sim.checksums()
            row = (sim.draws_needed + 15) // 16 * 16
            del sim
    assert np.array_equal(sums["host"], sums["device"])  # the same rows: the same batch
    host = min(runs["host"], key=lambda r: r["host_ms"])
    dev = min(runs["device"], key=lambda r: r["device_ms"] + r["host_ms"])
    return {"config": "c3", "top": TOP, "events": EVENTS, "instances": n, "row_bytes": row, "plane_bytes": n * row,
            "reps": reps, "host_gen_ms": round(host["host_ms"], 3), "device_gen_ms": round(dev["device_ms"], 4),
            "device_patch_ms": round(dev["host_ms"], 4), "patched_rows": dev["patched"],
            "ratio": round(host["host_ms"] / (dev["device_ms"] + dev["host_ms"]), 1),
            "first_flush_ms": {g: round(min(r["wall"] for r in runs[g]), 3) for g in runs},
            "exec_ms": {g: round(min(r["exec_ms"] for r in runs[g]), 4) for g in runs},
            "all_host_gen_ms": [round(r["host_ms"], 3) for r in runs["host"]],
            "all_device_gen_ms": [round(r["device_ms"], 4) for r in runs["device"]]}


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    sizes = [int(x) for x in sys.argv[2:]] or [20, 17]
    for g in ("host", "device"):
        fresh(4096, g)  # warm-up: device initialisation, the exec kernel of this topology, the tables
    for k in sizes:
        print(json.dumps(measure(k, reps)), flush=True)
