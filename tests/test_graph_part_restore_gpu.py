"""A partitioned run that begins in a restored cut (cl_graph_part_begin_seeded,
PartitionedGraphSim.restore / from_cut / cut): ranks over gloo share the GPU (the worker pattern of
test_graph_table_partition_gpu.py, its programs), every rank restores the whole cut and queues the
messages of its own nodes' out-channels with their draw indices among all of the cut's.

Every expected value is made in the parent on the CPU oracle: the cut is the oracle's own snapshot
(restorecheck.seed_of_oracle) or written by hand, the run it must equal is the host route on the
oracle (restorecheck.oracle_equivalent: node tokens T', the cut's messages re-sent in (channel,
position) order, then the continuation), and a rank's share is the numpy statement of
partrestorecheck.  Shapes: 7,121 entries / 11,114 messages over 2,000 nodes split 1024 + 976 and
768 + 768 + 464; entries on either side of, and exactly at, the boundary channel of a 2 x 2048
split, 300 messages on one channel (two workgroups of the seed kernel within one entry); empty
shares; the first and the last channel; rings filled exactly and by two too many."""
import functools
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

import graphgen as G
import partrestorecheck as PR
import test_graph_table_partition_gpu as TP
from snapcheck import ROOT

pytestmark = pytest.mark.gpu

CASE = TP.CASES[1]                     # power-law, 2,000 nodes, drained
SID = 5
DELAY = ("hash", 41)                   # the restored run's own delay source
OPS = [("snap", 1234), ("drain",)]     # the continuation: one snapshot, then the drain
FIFO_OVERFLOW, DELAY_EXHAUSTED = 3, 5  # include/clsnap.h CL_INST_*
TRAFFIC = (99, 1 << 30, 30)            # seed, threshold, steps of the traffic test; a snapshot at rank 11 at step 4
SMALL = (512, 3, 7)                    # the unseedable cases' regular graph: nodes, degree, seed


# ---- the worker side ---------------------------------------------------------------------------
def _set_delay(r, delay):
    {"hash": r.set_delay_hash, "schedule": r.set_delay_schedule}[delay[0]](delay[1])


def _continue_op(ps, op):
    """One step of a continuation, on every rank: ("snap", rank) | ("tick", k) | ("drain",)."""
    if op[0] == "snap":
        ps.start_snapshot_rank(op[1])
    elif op[0] == "tick":
        for _ in range(op[1]):
            ps.tick()
    else:
        assert op == ("drain",)
        ps.drain()


def _continue(ps, ops):
    ps.start()
    for op in ops:
        _continue_op(ps, op)


def _report(ps, **more):
    """What the parent checks of one rank; results() is gathered (a collective), kept from rank 0."""
    res = ps.results()
    g = ps.g
    rep = {"share": ps.seed_share, "span": (ps.lo, ps.hi), "status": g.status(), "frozen": ps.frozen,
           "time": g.time(), "counters": g.counters(), "info": g.seed_info, "seed_ms": g.restore_time()[1],
           "in_flight": g.checksums()["in_flight"], "results": res if ps.rank == 0 else None}
    rep.update(more)
    return rep


def _hand_cut(clg, template, c):
    return clg.SnapshotCut(c["sid"], c["tokens"], c["channel"], c["count"], c["msgs"], n_channels=template.num_channels,
                           topology_key=template.topology_key())


def _job_own(clg, rank, world, job):
    """The source runs partitioned; the run restored from its snapshot SID continues."""
    kind, n, steps, seed, drain, _ = CASE
    p = TP._program(kind, n, steps, seed)
    g = clg.GraphSim(device=0, fifo_slots=p.fifo_slots, max_snapshots=len(p.snap_step))
    g.set_topology(p.tokens, p.src, p.dst, id_width=p.width())
    g.set_delay_hash(p.delay_seed)
    g.set_traffic(p.traffic_seed, p.thresh, p.traffic_steps)
    ps = clg.PartitionedGraphSim(g, rank, world, transport=job["transport"])
    assert ps.seed_share is None
    ps.run_program(p.steps, p.snap_step, p.snap_rank)
    assert drain and ps.drain()
    template = clg.GraphSim(device=0, fifo_slots=p.fifo_slots)       # unpartitioned, no traffic, never run
    template.set_topology(p.tokens, p.src, p.dst, id_width=p.width())
    template.set_delay_hash(DELAY[1])
    pr = ps.restore(SID, template)
    assert (pr.rank, pr.world, pr.transport, pr.dev) == (ps.rank, ps.world, ps.transport, ps.dev)
    _continue(pr, OPS)
    return _report(pr, source_status=g.status())


def _job_world(clg, rank, world, job):
    """A saved cut with its topology, loaded by another number of ranks."""
    cut = clg.SnapshotCut.load(job["path"])
    ps = clg.PartitionedGraphSim.from_cut(cut, rank, world, configure=lambda r: _set_delay(r, DELAY), fifo_slots=512)
    _continue(ps, OPS)
    return _report(ps)


def _traffic_program(tick, snap, drain):
    for k in range(TRAFFIC[2]):
        if k == 4:
            snap(11)
        tick()
    drain()


def _job_traffic(clg, rank, world, job):
    """Traffic on the restored run; rank 0 also runs the yardstick: the same cut and configuration
    unpartitioned."""
    cut = clg.SnapshotCut.load(job["path"])

    def configure(r):
        _set_delay(r, DELAY)
        r.set_traffic(*TRAFFIC)

    ps = clg.PartitionedGraphSim.from_cut(cut, rank, world, configure=configure, transport=job["transport"],
                                          fifo_slots=512)
    ps.start()
    _traffic_program(ps.tick, ps.start_snapshot_rank, ps.drain)
    rep = _report(ps)
    if rank == 0:
        r = clg.GraphSim.from_cut(cut, fifo_slots=512)
        configure(r)
        _traffic_program(lambda: r.Tick(1), r.start_snapshot_rank, r.drain)
        r.flush()
        ticks = [r.snapshot_tick(s) for s in range(r.num_snapshots)]
        rep["whole"] = {"status": r.status(), "time": r.time(), "tokens": r.node_tokens_array(), "ticks": ticks,
                        "counters": r.counters(), "in_flight": r.checksums()["in_flight"],
                        "collected": [r.collect_arrays(s) for s in range(len(ticks)) if ticks[s] >= 0]}
    return rep


def _job_bounds(clg, rank, world, job):
    """Hand-made cuts on the 4,096-node regular graph, one after another on one template: the
    owned nodes' tokens after each of 12 single ticks."""
    kind, n, steps, seed, _, _ = TP.CASES[0]
    p = TP._program(kind, n, steps, seed)
    template = clg.GraphSim(device=0, fifo_slots=512)
    template.set_topology(p.tokens, p.src, p.dst, id_width=p.width())
    reps = []
    for c in job["cuts"]:
        ps = clg.PartitionedGraphSim.from_cut(_hand_cut(clg, template, c), rank, world, template=template,
                                              configure=lambda r, c=c: _set_delay(r, c["delay"]))
        ps.start()
        steps_tok = []
        for _ in range(12):
            ps.tick()
            steps_tok.append(ps.g.node_tokens_array()[ps.lo:ps.hi])
        reps.append(_report(ps, steps=np.array(steps_tok)))
    return reps


def _job_unseedable(clg, rank, world, job):
    n, deg, seed = SMALL
    src, dst = G.regular_graph(n, deg, seed)
    reps = []
    for c in job["cuts"]:
        template = clg.GraphSim(device=0, fifo_slots=c["fifo_slots"])
        template.set_topology(np.full(n, 50), src, dst, id_width=3)
        ps = clg.PartitionedGraphSim.from_cut(_hand_cut(clg, template, c), rank, world, template=template,
                                              configure=lambda r, c=c: _set_delay(r, c["delay"]),
                                              transport=job["transport"])
        assert ps.frozen == (c["status"] if job["transport"] == "device" else 0)   # (the host learns it at start())
        ps.start()
        after_start = (ps.frozen, ps.g.status(), ps.g.time())
        for op in c["ops"]:
            _continue_op(ps, op)
        reps.append(_report(ps, after_start=after_start))
    return reps


JOBS = {"own": _job_own, "world": _job_world, "traffic": _job_traffic, "bounds": _job_bounds,
        "unseedable": _job_unseedable}


def _worker(rank, world, port, job, out):
    import sys
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import cutcheck as CC
        out[rank] = JOBS[job["kind"]](CC.graph_module(), rank, world, job)
    except Exception as e:  # surfaced in the parent
        out[f"error{rank}"] = repr(e)
        raise
    finally:
        dist.destroy_process_group()


def spawn(world, **job):
    """{rank: the job's report} of `world` workers that share device 0."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, TP._free_port(), job, out), nprocs=world, join=True)
    got = dict(out)
    assert all(r in got for r in range(world)), got
    return got


# ---- the parent side: the oracle ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_cut():
    """(seed of snapshot SID of the oracle's unpartitioned run of CASE, out_off, the oracle
    equivalent of the seed under DELAY after OPS).  Computed once; nothing changes them."""
    import graphcheck as GC
    import restorecheck as R
    kind, n, steps, seed, drain, _ = CASE
    p = TP._program(kind, n, steps, seed)
    o = GC.oracle_program(p, drain=True)
    assert o.status == 0 and o.complete(SID)
    shape = GC.clg.GraphSim()                              # (host only: the channel list in rank order)
    shape.set_topology(p.tokens, p.src, p.dst, id_width=p.width())
    csrc, cdst = shape.channels()
    want = R.seed_of_oracle(o, SID, csrc, cdst)
    assert (want.channels, want.msgs) == (7121, 11114)
    oe = R.oracle_equivalent(want, DELAY, OPS)
    assert oe.status == 0 and oe.complete(0)
    return want, PR.out_offsets(n, csrc), oe


def cut_with_topology(seed, sid):
    """The SnapshotCut of a restorecheck.Seed, carrying its topology: made from the oracle alone."""
    import graphcheck as GC
    nz = np.nonzero(seed.counts)[0]
    return GC.clg.SnapshotCut(sid, seed.T, nz, seed.counts[nz], seed.vals, n_channels=seed.src.size,
                              topology_key=GC.clg.topology_key(seed.T.size, seed.src, seed.dst), src=seed.src,
                              dst=seed.dst, ids=np.array([i.encode() for i in seed.ids], dtype="S"))


def oracle_tokens(oe):
    nt = oe.node_tokens()
    return [nt[k] for k in oe.node_ids()]


def assert_results_are_oracle(reps, oe):
    """results() of a finished partitioned run (rank 0's gathered copy) against an oracle run."""
    import restorecheck as R
    status, tokens, ct, counters, snaps = reps[0]["results"]
    assert status == oe.status
    assert all(rep["status"] == oe.status and rep["time"] == oe.time for rep in reps.values())
    assert tokens.tolist() == oracle_tokens(oe)
    assert ct == [oe.completion_tick(s) for s in range(oe.num_snapshots)]
    oc = oe.counters()
    assert {k: counters[k] for k in R.EVENT_COUNTERS} == {k: oc[k] for k in R.EVENT_COUNTERS}
    assert sum(rep["counters"]["push"] for rep in reps.values()) == oc["push"]
    assert sorted(snaps) == [s for s in range(oe.num_snapshots) if oe.complete(s)]
    for sid, got in snaps.items():
        for a, b in zip(got, oe.collect_channels(sid)):
            np.testing.assert_array_equal(a, b)


def assert_shares(reps, channel, count, out_off, n):
    """Every rank's share is the numpy statement's, and together they tile the cut."""
    world = len(reps)
    sp = PR.spans(n, world)
    shares = [reps[r]["share"] for r in range(world)]
    assert [reps[r]["span"] for r in range(world)] == sp
    assert shares == [PR.share(channel, count, out_off, lo, hi) for lo, hi in sp]
    PR.assert_shares_tile(shares, len(channel), int(np.sum(count)))


# ---- 1. restored from its own run --------------------------------------------------------------
@pytest.mark.parametrize("transport", ["host", "device"])
def test_restored_from_its_own_partitioned_run(transport):
    want, out_off, oe = oracle_cut()
    reps = spawn(2, kind="own", transport=transport)
    assert all(rep["source_status"] == 0 for rep in reps.values())
    assert_results_are_oracle(reps, oe)
    assert len(reps[0]["results"][2]) == 1                      # the continuation's one snapshot, complete
    nz = np.nonzero(want.counts)[0]
    assert_shares(reps, nz, want.counts[nz], out_off, want.T.size)
    assert reps[1]["share"][1] == 7121 and reps[1]["share"][3] == 11114
    for rep in reps.values():
        assert rep["info"] == want.info(SID)                    # the whole cut, on every rank
        assert rep["seed_ms"] > 0


# ---- 2. another world --------------------------------------------------------------------------
def test_a_saved_cut_on_three_ranks_and_on_none(tmp_path):
    import graphcheck as GC
    import restorecheck as R
    want, out_off, oe = oracle_cut()
    cut = cut_with_topology(want, SID)
    path = str(tmp_path / "cut.npz")
    cut.save(path)
    reps = spawn(3, kind="world", path=path)
    assert [reps[r]["span"] for r in range(3)] == [(0, 768), (768, 1536), (1536, 2000)]
    assert_results_are_oracle(reps, oe)
    assert_shares(reps, cut.channel, cut.count, out_off, 2000)
    assert all(rep["info"] == want.info(SID) for rep in reps.values())
    # the same file unpartitioned: 1, 2 (above) and 3 ranks agree, being the oracle equivalent all
    r = GC.clg.GraphSim.from_cut(GC.clg.SnapshotCut.load(path), fifo_slots=512)
    R.set_delay(r, DELAY)
    GC.compare(R.run_engine(r, OPS), oe)


# ---- 3. slice boundaries -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def regular_topology():
    import graphcheck as GC
    kind, n, steps, seed, _, _ = TP.CASES[0]
    p = TP._program(kind, n, steps, seed)
    shape = GC.clg.GraphSim()
    shape.set_topology(p.tokens, p.src, p.dst, id_width=p.width())
    csrc, cdst = shape.channels()
    return n, csrc, cdst, shape.node_ids(), PR.out_offsets(n, csrc)


def hand_seed(tokens, entries):
    """(restorecheck.Seed, the cut's arrays) of entries {channel: payloads} on the regular graph."""
    import restorecheck as R
    n, csrc, cdst, ids, _ = regular_topology()
    counts = np.zeros(csrc.size, dtype=np.int64)
    vals = []
    for c in sorted(entries):
        counts[c] = len(entries[c])
        vals += list(entries[c])
    off = np.concatenate([[0], np.cumsum(counts)])
    return R.Seed(tokens, off, vals, csrc, cdst, ids)


def as_job_cut(seed, sid, delay, **more):
    nz = np.nonzero(seed.counts)[0]
    c = {"sid": sid, "tokens": seed.T, "channel": nz, "count": seed.counts[nz], "msgs": seed.vals, "delay": delay}
    c.update(more)
    return c


def test_slice_boundaries():
    import restorecheck as R
    n, csrc, cdst, ids, out_off = regular_topology()
    e = csrc.size
    c_mid = int(out_off[2048])
    assert n == 4096 and 0 < c_mid < e and csrc[c_mid - 1] == 2047 and csrc[c_mid] == 2048
    tokens = 100 + np.arange(n) % 7
    deep = lambda k: [2 + (3 * j + k) % 3 for j in range(300)]  # noqa: E731  (payloads 2..4)
    seeds = [
        hand_seed(tokens, {c_mid + 5: [1, 1], c_mid + 100: [3], e - 7: [2, 1, 1, 5]}),        # rank 0's share is empty
        hand_seed(tokens, {3: [4, 1], c_mid - 9: [1, 1, 1]}),                                 # rank 1's share is empty
        hand_seed(tokens, {c_mid - 1: deep(0), c_mid: deep(1)}),                              # exactly at the boundary
        hand_seed(tokens, {0: [1, 2, 3], e - 1: [5, 4, 3, 2, 1]}),                            # the first and the last channel
    ]
    sched = [(3 * i + 1) % 5 for i in range(8)]                                               # exactly the 8 draws
    delays = [("hash", 12), ("hash", 13), ("hash", 14), ("schedule", sched)]
    reps = spawn(2, kind="bounds", cuts=[as_job_cut(s, 20 + i, d) for i, (s, d) in enumerate(zip(seeds, delays))])
    empty = [(0, None), (1, None), (None, None), (None, None)]
    for i, (seed, delay) in enumerate(zip(seeds, delays)):
        both = {r: reps[r][i] for r in range(2)}
        nz = np.nonzero(seed.counts)[0]
        assert_shares(both, nz, seed.counts[nz], out_off, n)
        if empty[i][0] is not None:
            e_lo, e_hi, m_lo, m_hi = both[empty[i][0]]["share"]
            assert e_lo == e_hi and m_lo == m_hi
        if i == 2:
            assert both[0]["share"] == (0, 1, 0, 300) and both[1]["share"] == (1, 2, 300, 600)
        oe = R.oracle_equivalent(seed, delay)
        want = []
        for _ in range(12):
            assert oe.tick() == 0
            want.append(oracle_tokens(oe))
        got = np.concatenate([both[0]["steps"], both[1]["steps"]], axis=1)
        np.testing.assert_array_equal(got, np.array(want))
        assert all(rep["status"] == 0 and rep["time"] == 12 for rep in both.values())
        oc = oe.counters()
        for k in R.EVENT_COUNTERS:
            assert sum(rep["counters"][k] for rep in both.values()) == oc[k], k
        assert [rep["counters"]["push"] for rep in both.values()] == [rep["share"][3] - rep["share"][2]
                                                                     for rep in both.values()]
        assert all(rep["info"] == seed.info(20 + i) for rep in both.values())


# ---- 4. with traffic ---------------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["host", "device"])
def test_traffic_on_a_partitioned_restored_run(tmp_path, transport):
    """An engine-against-engine comparison.  With traffic the host-route equivalence does not hold
    (the step-0 traffic sees T, not T': test_graph_restore_gpu.test_traffic_on_a_restored_graph), so
    no oracle run exists to compare with.  The yardstick is the unpartitioned restored run of the
    same cut and configuration, which the restore and cut tests pin to the oracle without traffic and
    the partition tests pin with traffic from the initial state; the cut itself is the oracle's."""
    want, out_off, _ = oracle_cut()
    cut = cut_with_topology(want, SID)
    path = str(tmp_path / "cut.npz")
    cut.save(path)
    reps = spawn(2, kind="traffic", path=path, transport=transport)
    whole = reps[0]["whole"]
    status, tokens, ct, counters, snaps = reps[0]["results"]
    assert status == whole["status"] == 0
    assert all(rep["status"] == 0 and rep["time"] == whole["time"] for rep in reps.values())
    np.testing.assert_array_equal(tokens, whole["tokens"])
    assert ct == whole["ticks"] and len(ct) == 1 and ct[0] >= 0
    for k in ("push", "peek", "pop_tok", "pop_mk", "recorded", "completed"):
        assert counters[k] == whole["counters"][k], k
    assert counters["push"] > want.msgs
    for a, b in zip(snaps[0], whole["collected"][0]):
        np.testing.assert_array_equal(a, b)
    total = int(want.T.sum()) + want.tokens                        # the seed's: nodes and channels
    in_flight = sum(rep["in_flight"] for rep in reps.values())
    assert in_flight == whole["in_flight"]
    assert int(tokens.sum()) + in_flight == total == int(whole["tokens"].sum()) + whole["in_flight"]
    assert_shares(reps, cut.channel, cut.count, out_off, 2000)


# ---- 5. unseedable -----------------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["host", "device"])
def test_what_cannot_be_seeded_stops_every_rank_at_time_0(transport):
    import restorecheck as R
    import graphcheck as GC
    n, deg, gseed = SMALL
    src, dst = G.regular_graph(n, deg, gseed)
    shape = GC.clg.GraphSim()
    shape.set_topology(np.full(n, 50), src, dst, id_width=3)
    csrc, cdst = shape.channels()
    e = csrc.size
    out_off = PR.out_offsets(n, csrc)
    c = int(out_off[300]) + 1                                  # a channel of rank 1: rank 0's share is empty
    tokens = np.full(n, 50)

    def seed_of(k):
        counts = np.zeros(e, dtype=np.int64)
        counts[c] = k
        return R.Seed(tokens, np.concatenate([[0], np.cumsum(counts)]), [1 + j % 3 for j in range(k)], csrc, cdst,
                      shape.node_ids())

    ops = [("tick", 10), ("snap", int(csrc[c])), ("drain",)]   # (the seeded channel has emptied: its marker fits)
    sched = [(7 * i + 3) % 5 for i in range(10 + e)]           # the 10 seeded draws and one marker per channel
    cases = [
        as_job_cut(seed_of(10), 0, ("hash", 5), fifo_slots=8, ops=[("tick", 3)], status=FIFO_OVERFLOW),
        as_job_cut(seed_of(8), 1, ("hash", 5), fifo_slots=8, ops=ops, status=0),
        as_job_cut(seed_of(10), 2, ("schedule", sched[:9]), fifo_slots=16, ops=[("tick", 3)], status=DELAY_EXHAUSTED),
        as_job_cut(seed_of(10), 3, ("schedule", sched), fifo_slots=16, ops=ops, status=0),
    ]
    reps = spawn(2, kind="unseedable", cuts=cases, transport=transport)
    for i, case in enumerate(cases):
        both = {r: reps[r][i] for r in range(2)}
        k = int(case["count"][0])
        assert_shares(both, case["channel"], case["count"], out_off, n)
        assert both[0]["share"] == (0, 0, 0, 0) and both[1]["share"] == (0, 1, 0, k)
        if case["status"]:
            for rep in both.values():                          # every rank, the empty-handed one included
                assert rep["after_start"] == (case["status"], case["status"], 0)
                assert (rep["frozen"], rep["status"], rep["time"]) == (case["status"], case["status"], 0)
                assert rep["counters"]["push"] == 0 and rep["in_flight"] == 0          # nothing was queued
            np.testing.assert_array_equal(both[0]["results"][1], tokens)
        else:
            oe = R.oracle_equivalent(seed_of(k), case["delay"], ops)
            assert oe.status == 0 and oe.complete(0)
            assert all(rep["after_start"] == (0, 0, 0) for rep in both.values())
            assert_results_are_oracle(both, oe)


# ---- 6. errors (one process) -------------------------------------------------------------------
def test_errors_and_a_failed_begin_leaves_the_graph_whole():
    import graphcheck as GC
    import restorecheck as R
    import test_graph_restore_gpu as RT
    cl = GC.cl
    g, o = RT.scenario("10nodes.top", "10nodes.events")
    seed = R.seed_of_oracle(o, 0, *g.channels())               # 10 messages on one channel
    n = g.num_nodes
    share = np.full(4, -1, dtype=np.int64)

    def begin_seeded(r, lo, hi):
        return r._L.cl_graph_part_begin_seeded(r._h, lo, hi)

    r = g.restore(0)                                           # (it inherits the scenario's Go seed)
    L = r._L
    assert L.cl_graph_part_begin(r._h, 0, n) == cl.E_STATE     # as before
    assert begin_seeded(r, 0, n) == cl.E_STATE and b"delay" in L.cl_last_error()
    assert L.cl_graph_part_seed_share(r._h, share.ctypes.data) == cl.E_STATE
    r.set_delay_hash(3)
    for lo, hi in ((1, n), (0, n - 1), (0, n + 1), (-256, n), (256, n)):
        assert begin_seeded(r, lo, hi) == cl.E_INVALID, (lo, hi)
    r.trace_enable(64)
    assert begin_seeded(r, 0, n) == cl.E_STATE
    r.trace_enable(0)
    r.Tick(1)                                                  # a program
    assert begin_seeded(r, 0, n) == cl.E_STATE
    assert L.cl_graph_part_seed_share(r._h, share.ctypes.data) == cl.E_STATE and (share == -1).all()
    ops = [("tick", 1), ("snap", 0), ("drain",)]
    R.run_engine(r, ops[1:])                                   # after all that it runs unpartitioned
    GC.compare(r, R.oracle_equivalent(seed, ("hash", 3), ops))

    r = g.restore(0)
    r.set_delay_hash(3)
    assert begin_seeded(r, 0, n) == 0                          # one rank that owns everything
    assert begin_seeded(r, 0, n) == cl.E_STATE                 # twice
    assert L.cl_graph_part_begin(r._h, 0, n) == cl.E_STATE
    assert L.cl_graph_part_seed_share(r._h, share.ctypes.data) == 0 and share.tolist() == [0, 1, 0, 10]
    assert r.status() == 0 and r.counters()["push"] == 10 and r.seed_info == seed.info(0)
    np.testing.assert_array_equal(r.node_tokens_array(), seed.T)
    assert r.checksums()["in_flight"] == seed.tokens
    ordinary = GC.scenario_engine("10nodes.top", "10nodes.events", RT.SEED)
    assert begin_seeded(ordinary, 0, n) == cl.E_STATE          # not restored, with a device
