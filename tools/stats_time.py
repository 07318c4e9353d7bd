"""Device time of the per-snapshot statistics pass (cl_snapshot_stats) next to the packed collect
of the same snapshot, on C3 (8nodes-concurrent) at 2^20 and 2^17 instances: flush, rerun (the
records are then block-major by slot), then snapshot_stats and collect_snapshot_packed for every
snapshot id in the same process.  One JSON line per size:

  stats_ms      per snapshot id, the fastest of reps + 1 calls (cl_stats_time, HIP events)
  collect_ms    per snapshot id, the packed collect's kernels (cl_collect_time), the fastest of
                as many calls, same process
  bytes_min     what the statistics kernel must read per call: every instance's N * rw record
                words of the snapshot, its status word, its completion tick and its slot-map entry
  gbps, roof    bytes_min / stats_ms, and that over the 8 TB/s of the project's roofline

usage: python tools/stats_time.py [reps] [log2 sizes ...]      (the lines of profiles/stats_c3.json)
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
cl = importlib.import_module("chandy-lamport-distributed-snapshot-algorithm_amd")
DATA = os.path.join(ROOT, "tests", "golden", "test_data")
TOP, EVENTS = "8nodes.top", "8nodes-concurrent-snapshots.events"
ROOF_BYTES_PER_S = 8e12


# Words per node snapshot record of C3's 8nodes.top (degree bound 3: cl_engine.h rec_words pads
# 1 + 3 words to 4, one 16-byte record).  This tool measures C3 only.
C3_RECORD_WORDS = 4


def measure(log2n, reps):
    n = 1 << log2n
    sim = cl.ChandyLamportSim(n)
    sim.read_topology_file(os.path.join(DATA, TOP))
    n_sids = sim.read_events_file(os.path.join(DATA, EVENTS))
    sim.flush()
    sim.rerun()
    sim.synchronize()
    blocked = sim.records_blocked()
    rw = C3_RECORD_WORDS
    bytes_min = n * (sim.num_nodes * rw * 4 + 4 + 4 + (4 if blocked else 0))
    stats_ms, collect_ms, samples = [], [], []
    out = None
    for sid in range(n_sids):
        best = None
        for _ in range(reps + 1):       # (the first call also uploads the token histories)
            st = sim.snapshot_stats(sid)
            ms = sim.stats_time()
            best = ms if best is None else min(best, ms)
        stats_ms.append(best)
        samples.append(st.sample)
        best = None
        for _ in range(reps + 1):      # (as many calls as the statistics got)
            tok, done, off, msg = sim.collect_snapshot_packed(sid, out=out)
            out = (tok, np.zeros(n, dtype=np.int32), off, msg.base if msg.base is not None else msg)
            ms = sim.collect_time()
            best = ms if best is None else min(best, ms)
        collect_ms.append(best)
        assert int(done.sum()) >= st.sample    # (the collect also packs completed non-OK instances)
    gbps = [bytes_min / (ms * 1e-3) / 1e9 for ms in stats_ms]
    return {"config": "c3", "top": TOP, "events": EVENTS, "instances": n, "engine": sim.exec_engine(),
            "records_blocked": blocked, "snapshots": n_sids, "sample": samples, "reps": reps,
            "stats_ms": [round(x, 4) for x in stats_ms], "collect_ms": [round(x, 4) for x in collect_ms],
            "bytes_min": bytes_min, "gbps": [round(x, 1) for x in gbps],
            "roof": [round(x * 1e9 / ROOF_BYTES_PER_S, 4) for x in gbps]}


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    sizes = [int(x) for x in sys.argv[2:]] or [20, 17]
    for k in sizes:
        print(json.dumps(measure(k, reps)), flush=True)
