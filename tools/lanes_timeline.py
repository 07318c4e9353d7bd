"""Where a wave of the instance-per-lane kernel spends its shader-clock cycles, by segment of
program() (cl_lanes.h Timeline): row load, rest of the prologue, ops between tick loops, tick
loops, the wait for the memory operations still in flight at a tick loop's exit, epilogue.

Needs the dbg library (make dbg) and its timeline kernels:
  CLSNAP_VARIANT=dbg CLSNAP_TIMELINE=1 python tools/lanes_timeline.py [c3|c2] [replays] [instances] [out.json]
The timeline kernels carry two s_memtime reads and a full vmcnt drain around every tick loop, so
their own replay time (printed) is not the product kernel's."""
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
m = importlib.import_module("chandy-lamport-distributed-snapshot-algorithm_amd")
G = os.path.join(ROOT, "tests/golden/test_data/")
CFGS = {"c3": ("8nodes.top", "8nodes-concurrent-snapshots.events", 1 << 20),
        "c2": ("10nodes.top", "10nodes.events", 65536)}
SEGS = ("row_load", "prologue_rest", "ops_between_loops", "tick_loops", "post_loop_wait", "epilogue")
KERNELS = ("clsnap_lanes_nospill", "clsnap_lanes_spill")


def read(reset):
    out = (C.c_ulonglong * 16)()
    f = m.lib().cl_lanes_timeline_read
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int]
    if f(out, 1 if reset else 0) != 0:
        raise RuntimeError("cl_lanes_timeline_read failed")
    return [list(out[0:8]), list(out[8:16])]


def main():
    if os.environ.get("CLSNAP_VARIANT") != "dbg" or not os.environ.get("CLSNAP_TIMELINE"):
        sys.exit(__doc__)
    name = sys.argv[1] if len(sys.argv) > 1 else "c3"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    top, ev, n = CFGS[name]
    if len(sys.argv) > 3:
        n = int(sys.argv[3])
    s = m.ChandyLamportSim(n_instances=n)
    s.set_exec_engine(m.ChandyLamportSim.ENGINE_LANES)
    s.read_topology_file(G + top)
    s.read_events_file(G + ev)
    s.flush()
    s.synchronize()
    fresh = read(reset=True)
    for _ in range(3):
        s.rerun()
    s.synchronize()
    s.kernel_time()
    read(reset=True)
    for _ in range(reps):
        s.rerun()
    s.synchronize()
    tot, k = s.kernel_time()
    rep = read(reset=True)

    def table(raw, launches):
        t = {}
        for kn, row in zip(KERNELS, raw):
            # TL_* order: ROW, PRO, OPS, LOOP, WAIT, EPI, WAVES, LOOPS
            cyc = dict(zip(("row_load", "prologue_rest", "ops_between_loops", "tick_loops", "post_loop_wait",
                            "epilogue"), row[:6]))
            waves = row[6]
            if not waves:
                continue
            total = sum(cyc.values())
            t[kn] = {"waves_per_launch": waves / launches, "tick_loops_per_wave": row[7] / waves,
                     "cycles_per_wave": round(total / waves, 1),
                     "segments": {g: {"cycles_per_wave": round(cyc[g] / waves, 1), "share": round(cyc[g] / total, 4)}
                                  for g in SEGS}}
        return t

    out = {"config": name, "instances": n, "replays": reps, "timeline_build_ms_per_replay": round(tot / k, 4),
           "replay": table(rep, reps), "fresh_launch": table(fresh, 1)}
    print(json.dumps(out))
    if len(sys.argv) > 4:
        json.dump(out, open(sys.argv[4], "w"), indent=1)


if __name__ == "__main__":
    main()
