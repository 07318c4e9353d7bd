"""Helpers for the tests of GraphSim.restore (cl_graph_restore): the two runs a restored graph must
be indistinguishable from, built with calls that know nothing of restore.

TEST HELPER.  A Seed is the content of one completed snapshot as cl_graph_collect_snapshot returns
it: the tokenMap T, and per channel c (in channel order) the recorded payloads m[c][0..k_c).  With
no synthetic traffic, a graph restored from it equals a fresh run B of the same topology whose
node tokens are T'[v] = T[v] + (payloads recorded on v's out-channels) and whose first host events
are SendTokens(src(c), dest(c), m[c][j]) in (c, j) order: the sends leave T at the nodes, queue the
messages with delay draws 0..M-1 at time 0, and count M pushes.
  oracle_equivalent   B on the CPU oracle (the reference restated), then a continuation;
  engine_equivalent   B on the engine, then the same continuation;
  compare_engines     everything two engine runs can be asked, exact;
  step_tokens         node tokens after each of the first single ticks (pins every receiveTime).
A continuation is a list of ("snap", rank) | ("tick", k) | ("send", src rank, dest rank, n) |
("drain",); a delay source is ("go", seed) | ("hash", seed) | ("schedule", delays)."""
import numpy as np

import graphcheck as GC
import oracle as O
import tablecheck as T

clg = GC.clg
EVENT_COUNTERS = ("push", "peek", "pop_tok", "pop_mk", "recorded", "completed")


class Seed:
    def __init__(self, tokens, off, vals, src, dst, ids):
        self.T = np.asarray(tokens, dtype=np.int64)
        self.off = np.asarray(off, dtype=np.int64)
        self.vals = np.asarray(vals, dtype=np.int64)
        self.src, self.dst, self.ids = np.asarray(src), np.asarray(dst), list(ids)
        assert self.off.size == self.src.size + 1 and self.off[-1] == self.vals.size and (self.T >= 0).all()

    @property
    def counts(self):
        return np.diff(self.off)

    @property
    def msgs(self):
        return int(self.vals.size)

    @property
    def tokens(self):
        return int(self.vals.sum())

    @property
    def channels(self):
        return int((self.counts > 0).sum())

    def t_prime(self):
        """T[v] + the payloads recorded on v's out-channels."""
        cs = np.concatenate([[0], np.cumsum(self.vals)])
        per_ch = cs[self.off[1:]] - cs[self.off[:-1]]
        return self.T + np.bincount(self.src, weights=per_ch, minlength=self.T.size).astype(np.int64)

    def sends(self):
        """(src rank, dest rank, payload) in (c, j) order."""
        c = np.repeat(np.arange(self.src.size), self.counts)
        return list(zip(self.src[c].tolist(), self.dst[c].tolist(), self.vals.tolist()))

    def info(self, sid):
        """What GraphSim.seed_info must report."""
        return {"source_sid": sid, "channels": self.channels, "msgs": self.msgs, "tokens": self.tokens,
                "max_ch_msgs": int(self.counts.max()) if self.counts.size else 0,
                "unit_payloads": int((self.vals == 1).all()), "node_tokens": int(self.T.sum())}


def seed_of_oracle(o, sid, src, dst):
    assert o.complete(sid)
    tok, off, vals = o.collect_channels(sid)
    return Seed(tok, off, vals, src, dst, o.node_ids())


def run_oracle(o, ops, ids, max_drain=10000):
    for op in ops:
        if o.status:
            break
        if op[0] == "snap":
            o.start_snapshot(ids[op[1]])
        elif op[0] == "tick":
            for _ in range(op[1]):
                if o.tick():
                    break
        elif op[0] == "send":
            o.send_tokens(ids[op[1]], ids[op[2]], op[3])
        else:
            assert op == ("drain",)
            o.drain(max_drain)
    return o


def run_engine(g, ops):
    for op in ops:
        if op[0] == "snap":
            g.start_snapshot_rank(op[1])
        elif op[0] == "tick":
            g.Tick(op[1])
        elif op[0] == "send":
            g.send_tokens_rank(op[1], op[2], op[3])
        else:
            assert op == ("drain",)
            g.drain()
    g.flush()
    return g


def set_delay(x, delay):
    """The delay source on an OracleSim or a GraphSim."""
    kind, val = delay
    if isinstance(x, O.OracleSim):
        {"go": x.seed_go, "hash": x.use_counter_hash, "schedule": x.use_schedule}[kind](val)
    else:
        {"go": x.set_delay_go_seed, "hash": x.set_delay_hash, "schedule": x.set_delay_schedule}[kind](val)


def oracle_equivalent(seed, delay, ops=(), log=False, max_drain=10000):
    o = O.OracleSim()
    set_delay(o, delay)
    if log:
        o.log_enable()
    ids = seed.ids
    for v, t in enumerate(seed.t_prime().tolist()):
        assert o.add_node(ids[v], t) == 0
    for a, b in zip(seed.src.tolist(), seed.dst.tolist()):
        assert o.add_link(ids[a], ids[b]) == 0
    assert o.node_ids() == ids
    for a, b, m in seed.sends():
        if o.send_tokens(ids[a], ids[b], m):
            break
    return run_oracle(o, ops, ids, max_drain)


def engine_equivalent(seed, delay, ops=(), fifo_slots=16, lanes=0, run=True):
    """B on the engine, through calls that exist without restore."""
    g = clg.GraphSim(fifo_slots=fifo_slots)
    g.set_push_lanes(lanes)
    ids = seed.ids
    for v, t in enumerate(seed.t_prime().tolist()):
        g.AddNode(ids[v], t)
    for a, b in zip(seed.src.tolist(), seed.dst.tolist()):
        g.AddLink(ids[a], ids[b])
    set_delay(g, delay)
    assert g.node_ids() == ids
    for a, b, m in seed.sends():
        g.send_tokens_rank(a, b, m)
    return run_engine(g, ops) if run else g


def compare_engines(r, b):
    """Every query of two finished engine runs, exact."""
    assert r.status() == b.status() and r.time() == b.time()
    np.testing.assert_array_equal(r.node_tokens_array(), b.node_tokens_array())
    assert r.counters() == b.counters()
    assert r.checksums() == b.checksums()
    ns = r.num_snapshots
    assert ns == b.num_snapshots
    for sid in range(ns):
        assert r.snapshot_tick(sid) == b.snapshot_tick(sid), sid
        if r.snapshot_tick(sid) < 0:
            continue
        for x, y in zip(r.collect_arrays(sid), b.collect_arrays(sid)):
            np.testing.assert_array_equal(x, y)
    T.assert_rows_equal(r.snapshot_table().rows, b.snapshot_table().rows)
    if ns:
        assert r.snapshot_wave() == b.snapshot_wave()


def step_tokens(g, ticks=6):
    """Node tokens after each of the next `ticks` single ticks."""
    out = []
    for _ in range(ticks):
        g.Tick(1)
        g.flush()
        out.append(g.node_tokens_array())
    return np.array(out)


def check_time0(r, seed, sid):
    """A restored graph flushed with no event: the recorded cut and nothing else."""
    r.flush()
    assert r.status() == 0 and r.time() == 0 and r.num_snapshots == 0
    np.testing.assert_array_equal(r.node_tokens_array(), seed.T)
    c = r.counters()
    assert c["push"] == seed.msgs and c["ticks"] == 0
    assert all(c[k] == 0 for k in EVENT_COUNTERS if k != "push"), c
    s = r.checksums()
    assert s["ok"] == 1 and s["in_flight"] == seed.tokens and s["final_residual"] == 0
    assert s["delivered"] == s["completed"] == s["cut_residual"] == 0
    assert r.seed_info == seed.info(sid)
