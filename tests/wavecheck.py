"""Expected marker tree and marker-wave profile (graph.py MarkerTree / SnapshotWave,
include/clgraph.h cl_graph_snapshot_tree / cl_graph_snapshot_wave) restated from the CPU oracle
alone.

TEST HELPER.  Everything comes from the Logger of an OracleSim (o.log_enable()):
  tablecheck.creation_epochs  initiator, start epoch and per node the creation epoch of every sid;
  parent[sid, v]              the `other` field (the sender) of the first LOG_RECV_MARKER(sid)
                              delivered to v, -1 at the LOG_START node, -2 where there is none;
  depth[sid, v]               filled in ascending epoch order, depth[v] = depth[parent] + 1 --
                              which asserts that every parent was created strictly earlier.
The wave rows follow from the bin rules of clgraph.h.  All comparisons are exact."""
import functools

import numpy as np

import graphcheck as GC
import tablecheck as T

clg = GC.clg
HEAD = len(clg.WAVE_HEAD)
W = {f: i for i, f in enumerate(clg.WAVE_HEAD)}
I64_MAX, I64_MIN = T.I64_MAX, T.I64_MIN


class Expected:
    """parent, tick, depth: int64[S, N] (-2 / -1 / -1 where a node has no local snapshot);
    origin[S]: the start epoch."""

    def __init__(self, o):
        n, s = len(o.node_ids()), o.num_snapshots
        self.initiator, self.origin, self.tick = T.creation_epochs(o)
        self.parent = np.full((s, n), -2, dtype=np.int64)
        for _, kind, node, other, data, _ in o.log():
            if kind == T.LOG_START:
                self.parent[data, node] = -1
            elif kind == T.LOG_RECV_MARKER and self.parent[data, node] == -2:
                self.parent[data, node] = other
        np.testing.assert_array_equal(self.parent != -2, self.tick >= 0)
        self.depth = np.full((s, n), -1, dtype=np.int64)
        for sid in range(s):
            par, ep, dep = self.parent[sid], self.tick[sid], self.depth[sid]
            made = np.nonzero(par != -2)[0]
            for v in made[np.argsort(ep[made], kind="stable")]:
                if par[v] == -1:
                    assert v == self.initiator[sid] and ep[v] == self.origin[sid]
                    dep[v] = 0
                else:
                    assert 0 <= ep[par[v]] < ep[v], (sid, v)        # the parent was created strictly earlier
                    dep[v] = dep[par[v]] + 1                        # (so its depth is already known)
            assert (dep[made] >= 0).all()

    def trees(self, sid_lo=0, sid_hi=None):
        hi = self.parent.shape[0] if sid_hi is None else sid_hi
        return [clg.MarkerTree(self.parent[s], self.tick[s], 0, s) for s in range(sid_lo, hi)]

    def rows(self, lat_bins, lat_width, depth_bins, origins=None, node_lo=0, node_hi=None):
        """The wave rows of all sids over the nodes [node_lo, node_hi) (default: all), latencies
        from `origins` (default: the start epochs)."""
        s, n = self.parent.shape
        hi = n if node_hi is None else node_hi
        org = self.origin if origins is None else np.asarray(origins, dtype=np.int64)
        out = np.zeros((s, HEAD + lat_bins + depth_bins), dtype=np.int64)
        for sid in range(s):
            r = out[sid]
            r[W["sid"]], r[W["origin"]] = sid, org[sid]
            r[W["lat_min"]], r[W["lat_max"]], r[W["depth_max"]] = I64_MAX, I64_MIN, -1
            ep, dep = self.tick[sid, node_lo:hi], self.depth[sid, node_lo:hi]
            made = ep >= 0
            if not made.any():
                continue
            lat = ep[made] - org[sid]
            r[W["created"]] = lat.size
            r[W["lat_sum"]], r[W["lat_sumsq"]] = lat.sum(), (lat * lat).sum()
            r[W["lat_min"]], r[W["lat_max"]] = lat.min(), lat.max()
            b = np.where(lat < 0, 0, np.minimum(lat // lat_width, lat_bins - 1))
            r[HEAD:HEAD + lat_bins] = np.bincount(b, minlength=lat_bins)
            if depth_bins:
                d = dep[made]
                r[W["depth_sum"]], r[W["depth_sumsq"]], r[W["depth_max"]] = d.sum(), (d * d).sum(), d.max()
                r[HEAD + lat_bins:] = np.bincount(np.minimum(d, depth_bins - 1), minlength=depth_bins)
        return out


def assert_wave(got, want_rows, spec):
    """A SnapshotWave against expected rows, word by word."""
    assert got.spec == tuple(spec)
    assert got.rows.shape == want_rows.shape, (got.rows.shape, want_rows.shape)
    for f, i in W.items():
        np.testing.assert_array_equal(got.rows[:, i], want_rows[:, i], err_msg=f"word {f}")
    np.testing.assert_array_equal(got.lat_hist, want_rows[:, HEAD:HEAD + spec[0]], err_msg="lat_hist")
    np.testing.assert_array_equal(got.depth_hist, want_rows[:, HEAD + spec[0]:], err_msg="depth_hist")
    assert (got.broken == 0).all()


def assert_trees(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.parent, w.parent, err_msg=f"parent of sid {w.sid}")
        if g.tick is not None:
            np.testing.assert_array_equal(g.tick, w.tick, err_msg=f"tick of sid {w.sid}")


@functools.lru_cache(maxsize=None)
def powerlaw_drained():
    p, o, table = T.powerlaw_drained()
    return p, o, table, Expected(o)


@functools.lru_cache(maxsize=None)
def powerlaw_undrained():
    p, o, table = T.powerlaw_undrained()
    return p, o, table, Expected(o)


def ring_program(n=600, start=200):
    """A directed ring of n nodes with 10 tokens each, one snapshot at step 1 from rank `start`,
    no traffic: the marker walks the whole ring, so the tree is one chain of depth n - 1."""
    src = np.arange(n, dtype=np.int32)
    return GC.Program(np.full(n, 10), src, (src + 1) % n, 2, traffic_seed=1, thresh=0, traffic_steps=0,
                      snap_step=[1], snap_rank=[start], delay_seed=5)


@functools.lru_cache(maxsize=None)
def ring_drained():
    p = ring_program()
    o = GC.oracle_program(p, drain=True, log=True)
    return p, o, Expected(o)
