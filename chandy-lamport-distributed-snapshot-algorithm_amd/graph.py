"""Graph engine: ONE reference simulation over a large topology (include/clgraph.h).

``GraphSim`` mirrors the reference simulator API (sim.go ``ChandyLamportSim``:
``AddNode``, ``AddLink``, ``ProcessEvent``, ``Tick``, ``StartSnapshot``,
``CollectSnapshot``) for a single run whose nodes and channels span the whole GPU --
BASELINE configs 4 (2^20-node random regular digraph under continuous token traffic)
and 5 (100k-node power-law graph with 4,096 overlapping snapshots) -- and runs the
reference's own test_data scenarios as well.  There is no CPU fallback: without the
HIP library or a gfx950 GPU, calls that need them raise ``ClSnapError``.
"""
import ctypes as C
import hashlib
import os

import numpy as np

from . import (ClSnapError, GlobalSnapshot, MsgSnapshot, PassTokenEvent, SnapshotEvent, _check, _p, format_log,
               COUNTER_NAMES, E_LIMIT, lib)

GSUM_NAMES = ("ok", "delivered", "completed", "cut_residual", "final_residual", "digest", "in_flight")

# cl_graph_snap_row (include/clgraph.h): one 128-byte row per snapshot id.
SNAP_ROW_FIELDS = ("sid", "initiator", "start_tick", "complete_tick", "nodes_created", "last_create_tick",
                   "node_tokens", "min_node_tokens", "max_node_tokens", "rec_msgs", "rec_tokens", "rec_channels",
                   "max_ch_msgs", "digest")
SNAP_ROW_DTYPE = np.dtype([(f, np.int64) for f in SNAP_ROW_FIELDS] + [("reserved", np.int64, (2,))])


class GraphCut(C.Structure):
    """cl_graph_cut (include/clgraph.h): 64 bytes."""
    _fields_ = [("source_sid", C.c_int64), ("n_nodes", C.c_int64), ("tokens", C.POINTER(C.c_int32)),
                ("n_entries", C.c_int64), ("channel", C.POINTER(C.c_int32)), ("count", C.POINTER(C.c_int32)),
                ("n_msgs", C.c_int64), ("msg_tokens", C.POINTER(C.c_int32))]


_SIGS = None


def glib():
    """The engine library with the cl_graph_* signatures bound."""
    global _SIGS
    L = lib()
    if _SIGS is None:
        vp, i64, i32, u64, u32, cp = C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint32, C.c_char_p
        sig = {
            "cl_graph_create": [C.POINTER(C.c_void_p)],
            "cl_graph_destroy": [vp],
            "cl_graph_set_device": [vp, i32],
            "cl_graph_add_node": [vp, cp, i64],
            "cl_graph_add_link": [vp, cp, cp],
            "cl_graph_read_topology_text": [vp, cp],
            "cl_graph_read_topology_file": [vp, cp],
            "cl_graph_set_topology": [vp, i32, i32, vp, i64, vp, vp],
            "cl_graph_generate_regular": [vp, i32, i32, i64, u64],
            "cl_graph_generate_powerlaw": [vp, i32, i32, C.c_double, i32, i64, u64],
            "cl_graph_num_nodes": [vp, vp],
            "cl_graph_num_channels": [vp, vp],
            "cl_graph_channels": [vp, vp, vp],
            "cl_graph_node_id": [vp, i32, vp, i32],
            "cl_graph_node_id_length": [vp, i32, vp],
            "cl_graph_set_push_lanes": [vp, i32],
            "cl_graph_trace_enable": [vp, i32],
            "cl_graph_trace_read": [vp, vp, i32, vp],
            "cl_graph_set_limits": [vp, i32, i32, i64],
            "cl_graph_set_delay_hash": [vp, u64],
            "cl_graph_set_delay_go_seed": [vp, i64],
            "cl_graph_set_delay_schedule": [vp, vp, i64],
            "cl_graph_set_traffic": [vp, u64, u32, i64],
            "cl_graph_send_tokens": [vp, cp, cp, i64],
            "cl_graph_send_tokens_rank": [vp, i32, i32, i64],
            "cl_graph_start_snapshot": [vp, cp, vp],
            "cl_graph_start_snapshot_rank": [vp, i32, vp],
            "cl_graph_tick": [vp, i32],
            "cl_graph_drain": [vp],
            "cl_graph_read_events_text": [vp, cp, vp],
            "cl_graph_read_events_file": [vp, cp, vp],
            "cl_graph_flush": [vp],
            "cl_graph_rerun": [vp],
            "cl_graph_synchronize": [vp],
            "cl_graph_run_time": [vp, vp, vp, vp],
            "cl_graph_phase_time": [vp, vp, vp],
            "cl_graph_debug_poison_outputs": [vp],
            "cl_graph_device_bytes": [vp, vp],
            "cl_graph_get_status": [vp, vp],
            "cl_graph_get_time": [vp, vp],
            "cl_graph_num_snapshots": [vp, vp],
            "cl_graph_node_tokens": [vp, vp],
            "cl_graph_snapshot_tick": [vp, i32, vp],
            "cl_graph_collect_snapshot": [vp, i32, vp, vp, vp, i64],
            "cl_graph_get_counters": [vp, vp],
            "cl_graph_get_checksums": [vp, vp],
            "cl_graph_snapshot_table": [vp, i32, i32, vp],
            "cl_graph_table_time": [vp, vp],
            "cl_graph_snapshot_wave": [vp, i32, i32, vp, vp, vp, i64],
            "cl_graph_wave_time": [vp, vp, vp],
            "cl_graph_set_wave_scratch": [vp, i64],
            "cl_graph_snapshot_tree": [vp, i32, i32, vp, vp],
            "cl_graph_collect_sparse": [vp, i32, i32, vp, vp, vp, vp, i64, vp, i64, vp, vp],
            "cl_graph_sparse_time": [vp, vp],
            "cl_graph_snapshot_profile": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64],
            "cl_graph_profile_time": [vp, vp],
            "cl_graph_set_profile_slices": [vp, i32],
            "cl_graph_restore": [vp, i32, C.POINTER(C.c_void_p)],
            "cl_graph_seed_info_of": [vp, vp],
            "cl_graph_restore_time": [vp, vp, vp],
            "cl_graph_restore_cut": [vp, C.POINTER(GraphCut), C.POINTER(C.c_void_p)],
            "cl_graph_part_begin": [vp, i32, i32],
            "cl_graph_part_begin_seeded": [vp, i32, i32],
            "cl_graph_part_seed_share": [vp, vp],
            "cl_graph_part_snapshot": [vp, i32, vp],
            "cl_graph_part_pick": [vp, vp, i64, vp],
            "cl_graph_part_receive": [vp, vp, i64, vp, i64, vp],
            "cl_graph_part_tally": [vp, i32, vp, i64, vp],
            "cl_graph_part_bases": [vp, vp, vp, i64, vp],
            "cl_graph_part_push": [vp, i32, vp, i64],
            "cl_graph_part_freeze": [vp, i32],
            "cl_graph_part_dev_bind": [vp, i32, i32, i32, i64, vp, vp, vp, vp],
            "cl_graph_part_dev_seal": [vp],
            "cl_graph_part_dev_pick": [vp],
            "cl_graph_part_dev_receive": [vp],
            "cl_graph_part_dev_tally": [vp, i32],
            "cl_graph_part_dev_bases": [vp],
            "cl_graph_part_dev_push": [vp, i32],
            "cl_graph_set_stream": [vp, vp],
        }
        for name, args in sig.items():
            f = getattr(L, name)
            f.restype, f.argtypes = C.c_int, args
        L.cl_counter_hash.restype, L.cl_counter_hash.argtypes = u64, [u64, u64, u64]
        _SIGS = sig
    return L


def counter_hash(seed, a, b):
    """The synthetic workloads' counter hash (cg_hash, cg_engine.h)."""
    return glib().cl_counter_hash(seed, a, b)


class SnapshotTable:
    """Per-snapshot summary rows (SNAP_ROW_DTYPE) of GraphSim.snapshot_table, reduced on the
    device: when each snapshot started and completed, how far its marker wave got, what it
    recorded, and its term of the content digest."""

    _SUMS = ("nodes_created", "node_tokens", "rec_msgs", "rec_tokens", "rec_channels", "digest")
    _CHANNEL = ("rec_msgs", "rec_tokens", "rec_channels", "max_ch_msgs", "digest")

    def __init__(self, rows):
        self.rows = np.ascontiguousarray(rows, dtype=SNAP_ROW_DTYPE).reshape(-1)

    def __len__(self):
        return self.rows.size

    def __eq__(self, other):
        return isinstance(other, SnapshotTable) and np.array_equal(self.rows, other.rows)

    __hash__ = None

    def __repr__(self):
        return f"SnapshotTable({self.rows!r})"

    def _since_start(self, field):
        a, b = self.rows[field], self.rows["start_tick"]
        return np.where((a < 0) | (b < 0), np.int64(-1), a - b)

    @property
    def latency(self):
        """complete_tick - start_tick per row; -1 where either is -1."""
        return self._since_start("complete_tick")

    @property
    def spread(self):
        """last_create_tick - start_tick per row (how long the marker wave has run); -1 where
        either is -1."""
        return self._since_start("last_create_tick")

    def cut_residual(self, total_tokens):
        """|node_tokens + rec_tokens - total| per row (the consistency of its cut); 0 where the
        snapshot is not complete.  Its sum is the run's CL_GSUM_CUT_RESIDUAL."""
        r = self.rows
        d = np.abs(r["node_tokens"] + r["rec_tokens"] - np.int64(total_tokens))
        return np.where(r["complete_tick"] >= 0, d, np.int64(0))

    def digest_sum(self):
        """The rows' digests summed modulo 2^64, as an int64: CL_GSUM_DIGEST over all sids."""
        return int(self.rows["digest"].astype(np.uint64).sum(dtype=np.uint64).astype(np.int64))

    def merge(self, other):
        """The table of two parts of one partitioned run (the same sids in the same order):
        sums add, extremes combine, the one part that owns the initiator reports it and the
        start; a snapshot some part has not completed is incomplete, and its channel fields
        and digest are 0."""
        a, b = self.rows, other.rows
        if a.shape != b.shape or not np.array_equal(a["sid"], b["sid"]):
            raise ValueError("merge needs tables of the same snapshot ids in the same order")
        out = a.copy()
        with np.errstate(over="ignore"):
            for f in self._SUMS:
                out[f] = (a[f].astype(np.uint64) + b[f].astype(np.uint64)).astype(np.int64)
        for f in ("initiator", "start_tick", "last_create_tick", "max_node_tokens", "max_ch_msgs"):
            out[f] = np.maximum(a[f], b[f])
        out["min_node_tokens"] = np.minimum(a["min_node_tokens"], b["min_node_tokens"])
        done = (a["complete_tick"] >= 0) & (b["complete_tick"] >= 0)
        out["complete_tick"] = np.where(done, np.maximum(a["complete_tick"], b["complete_tick"]), np.int64(-1))
        for f in self._CHANNEL:
            out[f] = np.where(done, out[f], np.int64(0))
        return SnapshotTable(out)


# Head words of a cl_graph_snapshot_wave row (include/clgraph.h CL_WV_*): word i is WAVE_HEAD[i];
# lat_hist[lat_bins] and depth_hist[depth_bins] follow.
WAVE_HEAD = ("sid", "origin", "created", "lat_sum", "lat_sumsq", "lat_min", "lat_max", "depth_sum", "depth_sumsq",
             "depth_max", "broken", "reserved")
WAVE_MAX_BINS = 1024      # CL_GRAPH_WAVE_MAX_BINS
WAVE_SPEC_DTYPE = np.dtype([(f, np.int32) for f in ("lat_bins", "lat_width", "depth_bins", "reserved")])
_WV = {f: i for i, f in enumerate(WAVE_HEAD)}


class SnapshotWave:
    """Marker-wave profile rows of GraphSim.snapshot_wave, reduced on the device: per snapshot
    id the moments and the histogram of the nodes' creation latency (creation tick - origin; bin
    = latency < 0 ? 0 : min(latency // lat_width, lat_bins - 1)) and, with depth_bins > 0, of
    their depth in the marker tree (bin = min(depth, depth_bins - 1)).

      rows    int64[ns, len(WAVE_HEAD) + lat_bins + depth_bins]; the head words by name through
              word(name), the common ones as properties
      spec    (lat_bins, lat_width, depth_bins)"""

    def __init__(self, rows, lat_bins, lat_width=1, depth_bins=0):
        self.lat_bins, self.lat_width, self.depth_bins = int(lat_bins), int(lat_width), int(depth_bins)
        self.rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, self.row_words)

    @property
    def spec(self):
        return self.lat_bins, self.lat_width, self.depth_bins

    @property
    def row_words(self):
        return len(WAVE_HEAD) + self.lat_bins + self.depth_bins

    def __len__(self):
        return self.rows.shape[0]

    def __eq__(self, other):
        return isinstance(other, SnapshotWave) and self.spec == other.spec and np.array_equal(self.rows, other.rows)

    __hash__ = None

    def __repr__(self):
        return f"SnapshotWave({len(self)} snapshots, lat_bins={self.lat_bins}, lat_width={self.lat_width}, " \
               f"depth_bins={self.depth_bins})"

    def word(self, name):
        """Head word `name` (WAVE_HEAD) of every row."""
        return self.rows[:, _WV[name]]

    sid = property(lambda self: self.word("sid"))
    origin = property(lambda self: self.word("origin"))
    created = property(lambda self: self.word("created"))
    broken = property(lambda self: self.word("broken"))

    @property
    def lat_hist(self):
        return self.rows[:, len(WAVE_HEAD):len(WAVE_HEAD) + self.lat_bins]

    @property
    def depth_hist(self):
        return self.rows[:, len(WAVE_HEAD) + self.lat_bins:]

    @staticmethod
    def _ratio(a, b):
        out = np.full(a.shape, np.nan)
        np.divide(a, b, out=out, where=b > 0)
        return out

    @property
    def mean_latency(self):
        """lat_sum / created per row; nan where nothing was created."""
        return self._ratio(self.word("lat_sum").astype(np.float64), self.created)

    @property
    def mean_depth(self):
        """depth_sum over the nodes that have a depth; nan with the depth off or none."""
        return self._ratio(self.word("depth_sum").astype(np.float64), self.depth_hist.sum(axis=1))

    def coverage(self):
        """float[ns, lat_bins]: the share of the created nodes whose latency lies in bins 0..b --
        how far the wave had got by the end of bin b; 0 where nothing was created."""
        c = np.cumsum(self.lat_hist, axis=1).astype(np.float64)
        out = np.zeros_like(c)
        np.divide(c, self.created[:, None], out=out, where=self.created[:, None] > 0)
        return out

    def merge(self, other):
        """The profile of two parts of one partitioned run (the same sids, spec and origins, else
        ValueError): counts, sums and histograms add (the squares modulo 2^64), extremes combine."""
        if not isinstance(other, SnapshotWave) or self.spec != other.spec:
            raise ValueError("merge needs profiles of the same spec")
        a, b = self.rows, other.rows
        if a.shape != b.shape or not np.array_equal(self.sid, other.sid):
            raise ValueError("merge needs profiles of the same snapshot ids in the same order")
        if not np.array_equal(self.origin, other.origin):
            raise ValueError("merge needs profiles measured from the same origins")
        with np.errstate(over="ignore"):
            out = (a.astype(np.uint64) + b.astype(np.uint64)).astype(np.int64)     # sums and histograms
        for f in ("sid", "origin", "reserved"):
            out[:, _WV[f]] = a[:, _WV[f]]
        for f in ("lat_max", "depth_max"):
            out[:, _WV[f]] = np.maximum(a[:, _WV[f]], b[:, _WV[f]])
        out[:, _WV["lat_min"]] = np.minimum(a[:, _WV["lat_min"]], b[:, _WV["lat_min"]])
        return SnapshotWave(out, *self.spec)


class MarkerTree:
    """The marker tree of one snapshot over the node ranks [node_lo, node_lo + len(parent))
    (GraphSim.snapshot_tree): parent[v - node_lo] is the rank of the node whose marker created v's
    local snapshot, -1 at the initiator, -2 where there is no local snapshot; tick the creation
    epoch (-1 likewise), or None."""

    def __init__(self, parent, tick=None, node_lo=0, sid=-1):
        self.parent = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1)
        self.tick = None if tick is None else np.ascontiguousarray(tick, dtype=np.int32).reshape(-1)
        if self.tick is not None and self.tick.size != self.parent.size:
            raise ValueError("parent and tick cover different nodes")
        self.node_lo, self.sid = int(node_lo), int(sid)

    def __len__(self):
        return self.parent.size

    def __eq__(self, other):
        if not isinstance(other, MarkerTree):
            return NotImplemented
        return self.node_lo == other.node_lo and np.array_equal(self.parent, other.parent) and \
            (self.tick is None) == (other.tick is None) and (self.tick is None or np.array_equal(self.tick, other.tick))

    __hash__ = None

    def __repr__(self):
        return f"MarkerTree(sid {self.sid}, nodes [{self.node_lo}, {self.node_lo + len(self)}), " \
               f"{int((self.parent != -2).sum())} created)"

    @property
    def created(self):
        return self.parent != -2

    def _whole(self):
        n = self.parent.size
        if self.node_lo != 0:
            raise ValueError("the tree of a part: gather the parts first (PartitionedGraphSim.snapshot_tree)")
        if ((self.parent < -2) | (self.parent >= n)).any():
            raise ValueError("a parent outside the tree's nodes")
        return n

    def depth(self):
        """int64 per node: tree edges up to the initiator (the initiator: 0), the definition of
        the device's depth fields, by pointer doubling in numpy; -1 where there is no local
        snapshot, or where the chain does not end at the initiator (it reaches a node without a
        local snapshot).  ValueError on a cycle."""
        self._whole()
        anc = self.parent.astype(np.int64)
        hops = (anc >= 0).astype(np.int64)
        for _ in range(64):
            live = np.nonzero(anc >= 0)[0]
            if live.size == 0:
                return np.where(anc == -1, hops, np.int64(-1))
            a = anc[live]
            up, more = anc[a], hops[a]
            anc[live], hops[live] = up, hops[live] + more
        raise ValueError("the parents hold a cycle")

    def path(self, v):
        """The ranks from v up to the initiator, both included.  ValueError if v holds no local
        snapshot or its chain does not end at the initiator."""
        n = self._whole()
        out, u = [], int(v)
        if not 0 <= u < n:
            raise IndexError(f"node {v} outside [0, {n})")
        while len(out) <= n:
            p = int(self.parent[u])
            if p == -2:
                raise ValueError(f"node {u} holds no local snapshot")
            out.append(u)
            if p == -1:
                return out
            u = p
        raise ValueError("the parents hold a cycle")


# cl_graph_sparse_info (include/clgraph.h): 8 x int64.
SPARSE_INFO_FIELDS = ("n_sids", "n_complete", "n_entries", "n_msgs", "unit_payloads", "node_lo", "node_hi",
                      "reserved")
SPARSE_INFO_DTYPE = np.dtype([(f, np.int64) for f in SPARSE_INFO_FIELDS])

# cl_graph_seed_info (include/clgraph.h): 8 x int64.
SEED_INFO_FIELDS = ("source_sid", "channels", "msgs", "tokens", "max_ch_msgs", "unit_payloads", "node_tokens",
                    "reserved")
SEED_INFO_DTYPE = np.dtype([(f, np.int64) for f in SEED_INFO_FIELDS])

_U64 = np.uint64


def _mix64(z):
    """mix64 (cl_engine.h) on uint64 arrays."""
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _U64(30))) * _U64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94d049bb133111eb)
    return z ^ (z >> _U64(31))


def _cg_hash(seed, a, b):
    """cg_hash (cg_engine.h) of a scalar a and a uint64 array b."""
    with np.errstate(over="ignore"):
        h = _mix64(np.asarray(_U64(seed) ^ (_U64(a) * _U64(0x9E3779B97F4A7C15))))
        return _mix64(h ^ (b * _U64(0xD6E8FEB86659FD93)))


class SparseSnapshots:
    """The recorded channel state of the snapshots [sid_lo, sid_lo + len(complete)), compacted
    on the device (GraphSim.collect_sparse, cl_graph_collect_sparse): one entry per channel
    with at least one recorded message of a completed snapshot, ordered by snapshot id, then
    channel index.

      complete[r]     1 iff snapshot sid_lo + r completed (an incomplete one has no entries)
      row_offsets     int64[len + 1]: the entries of snapshot sid_lo + r are [row_offsets[r],
                      row_offsets[r + 1])
      channel, count  int32 per entry: the channel (index into GraphSim.channels()) and its
                      recorded messages
      msg_offsets     int64[entries + 1]: entry i's payloads are msg_tokens[msg_offsets[i] :
                      msg_offsets[i + 1]], in delivery order
      msg_tokens      int32 payloads, or None when they were not asked for
      tokens          int32[len, node_hi - node_lo] recorded node tokens (a row of -1 for an
                      incomplete snapshot), or None
      node_lo/hi      the node ranks the object covers (a part of a partitioned run, else all)"""

    def __init__(self, sid_lo, complete, row_offsets, channel, count, msg_tokens=None, tokens=None, node_lo=0,
                 node_hi=0):
        self.sid_lo = int(sid_lo)
        self.complete = np.ascontiguousarray(complete, dtype=np.int32).reshape(-1)
        self.row_offsets = np.ascontiguousarray(row_offsets, dtype=np.int64).reshape(-1)
        self.channel = np.ascontiguousarray(channel, dtype=np.int32).reshape(-1)
        self.count = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
        self.msg_offsets = np.zeros(self.count.size + 1, dtype=np.int64)
        np.cumsum(self.count, dtype=np.int64, out=self.msg_offsets[1:])
        self.msg_tokens = None if msg_tokens is None else np.ascontiguousarray(msg_tokens, dtype=np.int32).reshape(-1)
        self.node_lo, self.node_hi = int(node_lo), int(node_hi)
        self.tokens = None if tokens is None else \
            np.ascontiguousarray(tokens, dtype=np.int32).reshape(self.complete.size, self.node_hi - self.node_lo)
        if self.row_offsets.size != self.complete.size + 1 or self.row_offsets[-1] != self.channel.size or \
                self.channel.size != self.count.size:
            raise ValueError("row_offsets, channel and count do not describe the same entries")
        if self.msg_tokens is not None and self.msg_tokens.size != self.msg_offsets[-1]:
            raise ValueError("msg_tokens does not hold the entries' messages")

    def __len__(self):
        return self.complete.size

    @property
    def sid_hi(self):
        return self.sid_lo + self.complete.size

    @property
    def n_entries(self):
        return self.channel.size

    @property
    def n_msgs(self):
        return int(self.msg_offsets[-1])

    def __eq__(self, other):
        if not isinstance(other, SparseSnapshots):
            return NotImplemented
        same = lambda a, b: (a is None) == (b is None) and (a is None or np.array_equal(a, b))  # noqa: E731
        return (self.sid_lo, self.node_lo, self.node_hi) == (other.sid_lo, other.node_lo, other.node_hi) and \
            all(same(getattr(self, f), getattr(other, f))
                for f in ("complete", "row_offsets", "channel", "count", "msg_tokens", "tokens"))

    __hash__ = None

    def __repr__(self):
        return (f"SparseSnapshots(sids [{self.sid_lo}, {self.sid_hi}), {int(self.complete.sum())} complete, "
                f"{self.n_entries} entries, {self.n_msgs} messages, nodes [{self.node_lo}, {self.node_hi}))")

    def _row(self, sid):
        r = sid - self.sid_lo
        if not 0 <= r < self.complete.size:
            raise IndexError(f"snapshot {sid} outside [{self.sid_lo}, {self.sid_hi})")
        return r

    def _need_complete(self, sid):
        r = self._row(sid)
        if not self.complete[r]:
            raise ClSnapError(-9, f"snapshot {sid} has not completed")
        return r

    def entries(self, sid):
        """(channel, count, payloads) of snapshot sid: its entries' channels and message counts,
        and one payload slice per entry (None without payloads)."""
        r = self._row(sid)
        a, b = int(self.row_offsets[r]), int(self.row_offsets[r + 1])
        pay = None
        if self.msg_tokens is not None:
            pay = [self.msg_tokens[self.msg_offsets[i]:self.msg_offsets[i + 1]] for i in range(a, b)]
        return self.channel[a:b], self.count[a:b], pay

    def dense(self, sid, n_channels):
        """(tokens, offsets[n_channels + 1], messages) as int64: what GraphSim.collect_arrays
        returns (tokens None when the object holds none); ClSnapError(-9) if sid has not
        completed."""
        r = self._need_complete(sid)
        if self.msg_tokens is None:
            raise ValueError("dense needs the payloads (collect_sparse(payloads=True))")
        a, b = int(self.row_offsets[r]), int(self.row_offsets[r + 1])
        cnt = np.zeros(n_channels, dtype=np.int64)
        cnt[self.channel[a:b]] = self.count[a:b]
        off = np.zeros(n_channels + 1, dtype=np.int64)
        np.cumsum(cnt, out=off[1:])
        msg = self.msg_tokens[self.msg_offsets[a]:self.msg_offsets[b]].astype(np.int64)   # (channel order already)
        tok = None if self.tokens is None else self.tokens[r].astype(np.int64)
        return tok, off, msg

    def digest(self, sid, n_nodes, n_channels):
        """Snapshot sid's term of CL_GSUM_DIGEST (cg_kernels.hip k_checks_snap; the `digest` of
        its SnapshotTable row), as an int64, from the sparse contents: the recorded tokens of
        every node, and of every channel its message count and payload sum -- (0, 0) for the
        channels without an entry.  Needs the token plane of all n_nodes nodes and the payloads."""
        r = self._need_complete(sid)
        if self.tokens is None or (self.node_lo, self.node_hi) != (0, n_nodes):
            raise ValueError("digest needs the token plane of every node (collect_sparse(tokens=True))")
        if self.msg_tokens is None:
            raise ValueError("digest needs the payloads (collect_sparse(payloads=True))")
        a, b = int(self.row_offsets[r]), int(self.row_offsets[r + 1])
        with np.errstate(over="ignore"):
            h = _cg_hash(0x5107, sid, np.arange(n_nodes, dtype=_U64))
            total = _mix64(h ^ self.tokens[r].astype(np.uint32).astype(_U64)).sum(dtype=_U64)
            word = np.zeros(n_channels, dtype=_U64)                  # (count << 32) | payload sum (low 32 bits)
            cs = np.concatenate([[0], np.cumsum(self.msg_tokens, dtype=np.int64)])
            sums = cs[self.msg_offsets[a + 1:b + 1]] - cs[self.msg_offsets[a:b]]
            word[self.channel[a:b]] = (self.count[a:b].astype(_U64) << _U64(32)) | \
                sums.astype(np.uint32).astype(_U64)
            hc = _cg_hash(0xC4A1, sid, np.arange(n_channels, dtype=_U64))
            total = total + _mix64(hc ^ word).sum(dtype=_U64)
        return int(np.asarray(total, dtype=_U64).astype(np.int64))

    def snapshot(self, sid, sim):
        """GlobalSnapshot of sid like sim.CollectSnapshot(sid): messages in (dest, src,
        delivery) order.  sim supplies the node ids and the channel list."""
        r = self._need_complete(sid)
        ids = sim.node_ids()
        if self.tokens is None or (self.node_lo, self.node_hi) != (0, len(ids)):
            raise ValueError("snapshot needs the token plane of every node (collect_sparse(tokens=True))")
        ch, cnt, pay = self.entries(sid)
        if pay is None:
            raise ValueError("snapshot needs the payloads (collect_sparse(payloads=True))")
        src, dst = sim.channels()
        order = np.lexsort((src[ch], dst[ch]))
        msgs = [MsgSnapshot(ids[src[ch[i]]], ids[dst[ch[i]]], int(t)) for i in order for t in pay[i]]
        return GlobalSnapshot(sid, dict(zip(ids, self.tokens[r].tolist())), msgs)

    def cut(self, sid, sim=None, topology=False):
        """Snapshot sid as a SnapshotCut: what GraphSim.restore_cut takes and SnapshotCut.save
        writes.  Needs the token plane of all nodes and the payloads (ValueError otherwise, like
        snapshot), so the merged result of PartitionedGraphSim.collect_sparse(tokens=True) serves;
        ClSnapError(E_NOT_COMPLETE) if sid has not completed.  sim (any GraphSim of the topology,
        a fresh template included) supplies n_channels and the topology key, and with
        topology=True the channel list and node ids that GraphSim.from_cut needs."""
        r = self._need_complete(sid)
        if self.tokens is None or self.node_lo != 0 or (sim is not None and self.node_hi != sim.num_nodes):
            raise ValueError("cut needs the token plane of every node (collect_sparse(tokens=True))")
        if self.msg_tokens is None:
            raise ValueError("cut needs the payloads (collect_sparse(payloads=True))")
        if topology and sim is None:
            raise ValueError("cut needs a sim to take the topology from")
        a, b = int(self.row_offsets[r]), int(self.row_offsets[r + 1])
        msg = self.msg_tokens[self.msg_offsets[a]:self.msg_offsets[b]]
        src = dst = ids = None
        if topology:
            src, dst = sim.channels()
            ids = _ids_array(sim)
        return SnapshotCut(sid, self.tokens[r], self.channel[a:b], self.count[a:b], msg,
                           n_channels=None if sim is None else sim.num_channels,
                           topology_key=None if sim is None else sim.topology_key(), src=src, dst=dst, ids=ids)

    @staticmethod
    def merge(parts):
        """The SparseSnapshots of a partitioned run from its parts' (the same sids; disjoint
        node ranges, so disjoint channels): per sid the entries of all parts sorted by channel;
        complete is the AND over the parts, and a sid some part has not completed has no
        entries and a token row of -1; token rows are concatenated in node_lo order.  Payloads
        and tokens are kept when every part holds them.  A pure host function."""
        parts = sorted(parts, key=lambda p: p.node_lo)
        if not parts:
            raise ValueError("merge needs at least one part")
        first = parts[0]
        ns = len(first)
        for a, b in zip(parts, parts[1:]):
            if b.sid_lo != first.sid_lo or len(b) != ns:
                raise ValueError("merge needs parts of the same snapshot ids")
            if b.node_lo != a.node_hi:
                raise ValueError("merge needs parts of adjacent node ranges")
        complete = np.ones(ns, dtype=np.int32)
        for p in parts:
            complete &= (p.complete != 0).astype(np.int32)
        with_msgs = all(p.msg_tokens is not None for p in parts)
        with_tokens = all(p.tokens is not None for p in parts)
        # every part's entries of the complete sids, keyed by (row, channel)
        row, chan, cnt, msgs = [], [], [], []
        for p in parts:
            prow = np.repeat(np.arange(ns, dtype=np.int64), np.diff(p.row_offsets))
            keep = complete[prow] != 0
            row.append(prow[keep]), chan.append(p.channel[keep]), cnt.append(p.count[keep])
            if with_msgs:
                msgs.append(p.msg_tokens[np.repeat(keep, p.count)])
        row, chan, cnt = np.concatenate(row), np.concatenate(chan), np.concatenate(cnt)
        order = np.lexsort((chan, row))
        msg_tokens = None
        if with_msgs:
            allm = np.concatenate(msgs)
            start = np.zeros(cnt.size + 1, dtype=np.int64)
            np.cumsum(cnt, dtype=np.int64, out=start[1:])
            c = cnt[order].astype(np.int64)
            # message j of the merged entry i sits at start[order[i]] + j of the concatenation
            within = np.arange(int(c.sum()), dtype=np.int64) - np.repeat(np.cumsum(c) - c, c)
            msg_tokens = allm[np.repeat(start[:-1][order], c) + within]
        row_offsets = np.zeros(ns + 1, dtype=np.int64)
        np.cumsum(np.bincount(row, minlength=ns), out=row_offsets[1:])
        tokens = None
        if with_tokens:
            tokens = np.concatenate([p.tokens for p in parts], axis=1)
            tokens[complete == 0] = -1
        return SparseSnapshots(first.sid_lo, complete, row_offsets, chan[order], cnt[order], msg_tokens, tokens,
                               parts[0].node_lo, parts[-1].node_hi)


# cl_graph_snapshot_profile (include/clgraph.h): head word i is PROFILE_HEAD[i] (CL_PF_*), hist[msg_bins]
# follows; one 32-byte entry per channel, one row of CL_PF_NODE_WORDS int64 per node.
PROFILE_HEAD = ("n_sids", "n_used", "node_lo", "node_hi", "channels", "active", "entries", "msgs", "tokens",
                "max_msgs", "max_peak", "max_snaps", "unit_payloads", "reserved13", "reserved14", "reserved15")
PROFILE_MAX_BINS = 1024   # CL_GRAPH_PROFILE_MAX_BINS
PROFILE_SPEC_DTYPE = np.dtype([(f, np.int32) for f in ("msg_bins", "msg_width", "min_msgs", "reserved")])
PROFILE_ENTRY_DTYPE = np.dtype([("channel", np.int32), ("snaps", np.int32), ("peak", np.int32), ("peak_sid", np.int32),
                                ("msgs", np.int64), ("tokens", np.int64)])
PROFILE_NODE_FIELDS = ("tok_sum", "tok_sumsq", "tok_min", "tok_max", "lat_sum", "lat_max", "in_msgs", "in_tokens")
PROFILE_NODE_DTYPE = np.dtype([(f, np.int64) for f in PROFILE_NODE_FIELDS])
_PF = {f: i for i, f in enumerate(PROFILE_HEAD)}


class SnapshotProfile:
    """Node and channel profile of GraphSim.snapshot_profile, reduced on the device over the used
    snapshots of a range -- the transposed view of the table, the wave and the sparse collect.

      sid_lo    first snapshot id of the range; used int32[ns]: 1 where row r (sid_lo + r) was used
                (the caller's mask and the snapshot's completion), n_used their count
      head      int64[len(PROFILE_HEAD)], by name through word(name); hist int64[msg_bins]: owned
                channels by min(msgs // msg_width, msg_bins - 1)
      entries   PROFILE_ENTRY_DTYPE, one per owned channel with msgs >= min_msgs, ascending channel
      node      PROFILE_NODE_DTYPE over the owned nodes [node_lo, node_hi), or None
      origins   what the latencies were measured from: the caller's int64[ns], None for the
                snapshots' start ticks"""

    def __init__(self, sid_lo, used, head, hist, entries, node=None, origins=None, msg_width=1, min_msgs=1):
        self.sid_lo = int(sid_lo)
        self.used = np.ascontiguousarray(used, dtype=np.int32).reshape(-1)
        self.head = np.ascontiguousarray(head, dtype=np.int64).reshape(-1)
        if self.head.size != len(PROFILE_HEAD):
            raise ValueError(f"a profile head has {len(PROFILE_HEAD)} words")
        self.hist = np.ascontiguousarray(hist, dtype=np.int64).reshape(-1)
        self.entries = np.ascontiguousarray(entries, dtype=PROFILE_ENTRY_DTYPE).reshape(-1)
        self.node = None if node is None else np.ascontiguousarray(node, dtype=PROFILE_NODE_DTYPE).reshape(-1)
        self.origins = None if origins is None else np.ascontiguousarray(origins, dtype=np.int64).reshape(-1)
        self.msg_width, self.min_msgs = int(msg_width), int(min_msgs)

    @property
    def spec(self):
        return self.hist.size, self.msg_width, self.min_msgs

    def word(self, name):
        """Head word `name` (PROFILE_HEAD)."""
        return int(self.head[_PF[name]])

    n_used = property(lambda self: self.word("n_used"))
    node_lo = property(lambda self: self.word("node_lo"))
    node_hi = property(lambda self: self.word("node_hi"))

    def __len__(self):
        return self.used.size

    def _same_call(self, other):
        """The same range, spec, used rows and origins."""
        return (self.sid_lo == other.sid_lo and self.spec == other.spec and np.array_equal(self.used, other.used)
                and (self.origins is None) == (other.origins is None)
                and (self.origins is None or np.array_equal(self.origins, other.origins)))

    def __eq__(self, other):
        return (isinstance(other, SnapshotProfile) and self._same_call(other)
                and np.array_equal(self.head, other.head) and np.array_equal(self.hist, other.hist)
                and np.array_equal(self.entries, other.entries) and (self.node is None) == (other.node is None)
                and (self.node is None or np.array_equal(self.node, other.node)))

    __hash__ = None

    def __repr__(self):
        return f"SnapshotProfile(sids {self.sid_lo}..{self.sid_lo + len(self)}, {self.n_used} used, " \
               f"nodes {self.node_lo}..{self.node_hi}, {self.entries.size} entries)"

    def _node_mean(self, field):
        if self.node is None:
            raise ValueError("the profile was taken without node rows")
        a = self.node[field].astype(np.float64)
        return a / self.n_used if self.n_used > 0 else np.full(a.shape, np.nan)

    def mean_tokens(self):
        """Mean recorded balance of every owned node over the used snapshots; nan with none used."""
        return self._node_mean("tok_sum")

    def var_tokens(self):
        """Population variance of every owned node's recorded balance over the used snapshots (how
        much it swings from cut to cut); nan with none used."""
        return self._node_mean("tok_sumsq") - self.mean_tokens() ** 2

    def mean_latency(self):
        """Mean creation tick - origin of every owned node over the used snapshots; nan with none used."""
        return self._node_mean("lat_sum")

    def hottest(self, k):
        """The entries of the k largest msgs, ties by lower channel."""
        e = self.entries
        return e[np.lexsort((e["channel"], -e["msgs"]))[:max(int(k), 0)]]

    def by_receiver(self, dst):
        """The entries summed by receiving node: a structured array over the owned nodes (node,
        channels, msgs, tokens); dst[c] = destination rank of channel c (GraphSim.channels())."""
        lo, hi = self.node_lo, self.node_hi
        v = np.asarray(dst, dtype=np.int64)[self.entries["channel"]] - lo
        out = np.zeros(hi - lo, dtype=[(f, np.int64) for f in ("node", "channels", "msgs", "tokens")])
        out["node"] = np.arange(lo, hi)
        out["channels"] = np.bincount(v, minlength=hi - lo)
        np.add.at(out["msgs"], v, self.entries["msgs"])
        np.add.at(out["tokens"], v, self.entries["tokens"])
        return out

    @staticmethod
    def merge(parts):
        """The profile of a partitioned run from its parts', in rank order (contiguous node ranges,
        so every channel belongs to exactly one part): node rows are concatenated, entries merged by
        ascending channel; hist and the head's counts add, its maxima take the maximum.  ValueError
        on differing range, spec, used rows or origins, or on node ranges that do not abut."""
        parts = list(parts)
        if not parts:
            raise ValueError("merge needs at least one part")
        first = parts[0]
        for a, b in zip(parts, parts[1:]):
            if not isinstance(b, SnapshotProfile) or not first._same_call(b) or len(first) != len(b):
                raise ValueError("merge needs parts of the same range, spec, used rows and origins")
            if b.node_lo != a.node_hi:
                raise ValueError("merge needs parts of adjacent node ranges, in rank order")
        head = first.head.copy()
        for f in ("channels", "active", "entries", "msgs", "tokens"):
            head[_PF[f]] = sum(p.word(f) for p in parts)
        for f in ("max_msgs", "max_peak", "max_snaps"):
            head[_PF[f]] = max(p.word(f) for p in parts)
        head[_PF["unit_payloads"]] = min(p.word("unit_payloads") for p in parts)
        head[_PF["node_hi"]] = parts[-1].node_hi
        entries = np.concatenate([p.entries for p in parts])
        entries = entries[np.argsort(entries["channel"], kind="stable")]
        node = None
        if all(p.node is not None for p in parts):
            node = np.concatenate([p.node for p in parts])
        return SnapshotProfile(first.sid_lo, first.used, head, sum(p.hist for p in parts), entries, node, first.origins,
                               first.msg_width, first.min_msgs)


def _ids_array(sim):
    """sim.node_ids() as a numpy S array (kept on the sim: the ids of a graph never change)."""
    a = getattr(sim, "_ids_s", None)
    if a is None:
        a = np.array([i.encode() for i in sim.node_ids()], dtype="S")
        try:
            sim._ids_s = a
        except AttributeError:
            pass
    return a


def _bulk_id_width(ids):
    """w if the S array ids is exactly "N" + the rank zero-padded to one width w (what
    set_topology(id_width=w) names its nodes), else 0."""
    w = ids.dtype.itemsize - 1
    n = ids.size
    if not 1 <= w <= 10 or n == 0 or len(str(n - 1)) > w:
        return 0
    b = np.ascontiguousarray(ids).view(np.uint8).reshape(n, w + 1)
    digits = b[:, 1:].astype(np.int64) - 48
    if (b[:, 0] != ord("N")).any() or (digits < 0).any() or (digits > 9).any():
        return 0
    value = digits @ (10 ** np.arange(w - 1, -1, -1, dtype=np.int64))
    return w if np.array_equal(value, np.arange(n, dtype=np.int64)) else 0


def topology_key(n, src, dst):
    """A 64-bit key of a topology in rank order: the 8-byte blake2b digest, read as a
    little-endian unsigned int, of int64 N, int64 E and the int32 bytes of the channel list
    (src, then dst) as GraphSim.channels returns it.  A pure host function."""
    s = np.ascontiguousarray(src, dtype="<i4").reshape(-1)
    d = np.ascontiguousarray(dst, dtype="<i4").reshape(-1)
    if s.size != d.size:
        raise ValueError("src and dst differ in length")
    h = hashlib.blake2b(digest_size=8)
    h.update(np.array([n, s.size], dtype="<i8").tobytes())
    h.update(s.tobytes())
    h.update(d.tobytes())
    return int.from_bytes(h.digest(), "little")


class SnapshotCut:
    """One recorded cut held on the host: what a completed snapshot contains, in the layout
    GraphSim.restore_cut (cl_graph_restore_cut) takes and save / load keep in a file.

      source_sid      the snapshot id it came from (reported back by seed_info, not interpreted)
      tokens          int32[N] the tokenMap, rank order
      channel, count  int32 per entry: the channels with recorded messages (index into
                      GraphSim.channels(), strictly ascending) and how many each holds
      msg_tokens      int32 payloads in entry order, delivery order within; None: all ones
      n_channels      E of the topology it belongs to, topology_key its key (topology_key());
                      None when unknown -- restore_cut refuses such a cut
      src, dst, ids   optionally the topology itself: the channel list and the node ids in rank
                      order (numpy S array), all three or none; GraphSim.from_cut needs them

    The constructor checks only that the lengths agree (ValueError); the contents are checked on
    the device by restore_cut."""

    _ARRAYS = ("tokens", "channel", "count", "msg_tokens", "src", "dst", "ids")

    def __init__(self, source_sid, tokens, channel, count, msg_tokens=None, n_channels=None, topology_key=None,
                 src=None, dst=None, ids=None):
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)  # noqa: E731
        self.source_sid = int(source_sid)
        self.tokens, self.channel, self.count = i32(tokens), i32(channel), i32(count)
        self.msg_tokens = None if msg_tokens is None else i32(msg_tokens)
        self.n_channels = None if n_channels is None else int(n_channels)
        self.topology_key = None if topology_key is None else int(topology_key)
        if self.channel.size != self.count.size:
            raise ValueError("channel and count differ in length")
        if self.msg_tokens is not None and self.msg_tokens.size != self.msgs:
            raise ValueError("msg_tokens does not hold the entries' messages")
        if self.n_channels is not None and not 0 <= self.channel.size <= self.n_channels:
            raise ValueError("more entries than channels")
        if len({src is None, dst is None, ids is None}) != 1:
            raise ValueError("src, dst and ids come together or not at all")
        self.src = self.dst = self.ids = None
        if src is not None:
            self.src, self.dst = i32(src), i32(dst)
            self.ids = np.ascontiguousarray(ids).reshape(-1)
            if self.ids.dtype.kind != "S":
                self.ids = np.array([str(i).encode() for i in self.ids.tolist()], dtype="S")
            if self.src.size != self.dst.size or (self.n_channels is not None and self.src.size != self.n_channels):
                raise ValueError("src and dst do not list n_channels channels")
            if self.ids.size != self.tokens.size:
                raise ValueError("ids and tokens differ in length")

    @property
    def msgs(self):
        return int(self.count.sum(dtype=np.int64))

    @property
    def channels(self):
        return int(self.channel.size)

    @property
    def payload_tokens(self):
        return self.msgs if self.msg_tokens is None else int(self.msg_tokens.sum(dtype=np.int64))

    @property
    def has_topology(self):
        return self.src is not None

    def info(self):
        """What seed_info of a graph restored from this cut must report."""
        return {"source_sid": self.source_sid, "channels": self.channels, "msgs": self.msgs,
                "tokens": self.payload_tokens, "max_ch_msgs": int(self.count.max()) if self.count.size else 0,
                "unit_payloads": int(self.msg_tokens is None or bool((self.msg_tokens == 1).all())),
                "node_tokens": int(self.tokens.sum(dtype=np.int64))}

    def dense(self):
        """(tokens, offsets[n_channels + 1], messages) as int64, like GraphSim.collect_arrays."""
        if self.n_channels is None:
            raise ValueError("dense needs n_channels")
        cnt = np.zeros(self.n_channels, dtype=np.int64)
        cnt[self.channel] = self.count
        off = np.zeros(self.n_channels + 1, dtype=np.int64)
        np.cumsum(cnt, out=off[1:])
        msg = np.ones(self.msgs, dtype=np.int64) if self.msg_tokens is None else self.msg_tokens.astype(np.int64)
        return self.tokens.astype(np.int64), off, msg

    def __eq__(self, other):
        if not isinstance(other, SnapshotCut):
            return NotImplemented
        same = lambda a, b: (a is None) == (b is None) and (a is None or np.array_equal(a, b))  # noqa: E731
        return (self.source_sid, self.n_channels, self.topology_key) == \
            (other.source_sid, other.n_channels, other.topology_key) and \
            all(same(getattr(self, f), getattr(other, f)) for f in self._ARRAYS)

    __hash__ = None

    def __repr__(self):
        return (f"SnapshotCut(sid {self.source_sid}, {self.tokens.size} nodes, {self.channels} entries, "
                f"{self.msgs} messages{', with topology' if self.has_topology else ''})")

    def save(self, path):
        """Writes the cut to path with numpy.savez (an .npz of plain arrays, no pickle)."""
        d = {f: getattr(self, f) for f in self._ARRAYS if getattr(self, f) is not None}
        d["source_sid"] = np.array(self.source_sid, dtype=np.int64)
        if self.n_channels is not None:
            d["n_channels"] = np.array(self.n_channels, dtype=np.int64)
        if self.topology_key is not None:
            d["topology_key"] = np.array(self.topology_key, dtype=np.uint64)
        with open(path, "wb") as f:
            np.savez(f, **d)

    @staticmethod
    def load(path):
        """The cut save wrote to path (numpy.load, allow_pickle=False)."""
        with np.load(path, allow_pickle=False) as z:
            get = lambda f: z[f] if f in z.files else None  # noqa: E731
            scalar = lambda f: None if f not in z.files else int(z[f])  # noqa: E731
            return SnapshotCut(int(z["source_sid"]), z["tokens"], z["channel"], z["count"], get("msg_tokens"),
                               scalar("n_channels"), scalar("topology_key"), get("src"), get("dst"), get("ids"))


class GraphSim:
    """One reference simulator (sim.go ChandyLamportSim) on the GPU, state in HBM."""

    def __init__(self, device=0, fifo_slots=16, max_snapshots=0, max_drain_ticks=10000):
        self._L = glib()
        self._pid = os.getpid()
        h = C.c_void_p()
        _check(self._L.cl_graph_create(C.byref(h)))
        self._h = h
        self.device = device
        _check(self._L.cl_graph_set_device(self._h, device))
        _check(self._L.cl_graph_set_limits(self._h, fifo_slots, max_snapshots, max_drain_ticks))
        self._ids = None

    @classmethod
    def _of_handle(cls, L, h, device, ids=None):
        """The GraphSim that owns the native graph h (made by a restore call)."""
        r = object.__new__(cls)
        r._L, r._h, r.device, r._ids, r._pid = L, h, device, ids, os.getpid()
        return r

    def __del__(self):
        # Only the process that made the graph destroys it.  A forked child (a multiprocessing
        # manager, a worker pool) holds copies of its parent's objects, and its garbage collector
        # may finalise them; the native graph's streams and buffers are the parent's, and a HIP
        # call on them from the child crashes it.
        h = getattr(self, "_h", None)
        if h and getattr(self, "_pid", None) == os.getpid():
            self._L.cl_graph_destroy(h)
        self._h = None

    # ---- topology -----------------------------------------------------------------
    def AddNode(self, node_id, tokens):             # sim.go:40
        _check(self._L.cl_graph_add_node(self._h, node_id.encode(), tokens))

    def AddLink(self, src, dest):                   # sim.go:46
        _check(self._L.cl_graph_add_link(self._h, src.encode(), dest.encode()))

    def read_topology_file(self, path):             # test_common.go:29
        _check(self._L.cl_graph_read_topology_file(self._h, path.encode()))

    def read_topology_text(self, text):
        _check(self._L.cl_graph_read_topology_text(self._h, text.encode()))

    def set_topology(self, tokens, src, dst, id_width=0):
        tok = np.ascontiguousarray(tokens, dtype=np.int64)
        s = np.ascontiguousarray(src, dtype=np.int32)
        d = np.ascontiguousarray(dst, dtype=np.int32)
        _check(self._L.cl_graph_set_topology(self._h, tok.size, id_width, _p(tok), s.size, _p(s), _p(d)))

    def generate_regular(self, n_nodes, degree=8, tokens=100, seed=0):
        _check(self._L.cl_graph_generate_regular(self._h, n_nodes, degree, tokens, seed))

    def generate_powerlaw(self, n_nodes, targets=8, exponent=0.9, ring=True, tokens=100, seed=0):
        _check(self._L.cl_graph_generate_powerlaw(self._h, n_nodes, targets, exponent, 1 if ring else 0,
                                                  tokens, seed))

    # ---- configuration --------------------------------------------------------------
    def set_limits(self, fifo_slots=16, max_snapshots=0, max_drain_ticks=10000):
        _check(self._L.cl_graph_set_limits(self._h, fifo_slots, max_snapshots, max_drain_ticks))

    def set_delay_hash(self, seed):
        _check(self._L.cl_graph_set_delay_hash(self._h, seed))

    def set_delay_go_seed(self, seed):
        _check(self._L.cl_graph_set_delay_go_seed(self._h, seed))

    def set_delay_schedule(self, delays):
        d = np.ascontiguousarray(delays, dtype=np.uint8).ravel()
        _check(self._L.cl_graph_set_delay_schedule(self._h, _p(d), d.size))

    def set_traffic(self, seed, threshold, steps):
        _check(self._L.cl_graph_set_traffic(self._h, seed, threshold, steps))

    def set_push_lanes(self, lanes):
        """Force the push kernel's lanes per node (0 automatic, 1 or 4): diagnostics and
        tests -- results are identical on either path."""
        _check(self._L.cl_graph_set_push_lanes(self._h, lanes))

    # ---- events -------------------------------------------------------------------------
    def ProcessEvent(self, event):                  # sim.go:58
        if isinstance(event, PassTokenEvent):
            _check(self._L.cl_graph_send_tokens(self._h, event.src.encode(), event.dest.encode(), event.tokens))
        elif isinstance(event, SnapshotEvent):
            self.StartSnapshot(event.nodeId)
        else:
            raise ClSnapError(-1, f"Error unknown event: {event!r}")

    def send_tokens_rank(self, src, dest, n):
        _check(self._L.cl_graph_send_tokens_rank(self._h, src, dest, n))

    def Tick(self, n=1):                            # sim.go:71
        _check(self._L.cl_graph_tick(self._h, n))

    def StartSnapshot(self, node_id):               # sim.go:105
        sid = C.c_int32(-1)
        _check(self._L.cl_graph_start_snapshot(self._h, node_id.encode(), C.byref(sid)))
        return sid.value

    def start_snapshot_rank(self, rank):
        sid = C.c_int32(-1)
        _check(self._L.cl_graph_start_snapshot_rank(self._h, rank, C.byref(sid)))
        return sid.value

    def drain(self):                                # test_common.go:123-137
        _check(self._L.cl_graph_drain(self._h))

    def read_events_file(self, path):               # test_common.go:79 (incl. drain)
        n = C.c_int32(0)
        _check(self._L.cl_graph_read_events_file(self._h, path.encode(), C.byref(n)))
        return n.value

    def read_events_text(self, text):
        n = C.c_int32(0)
        _check(self._L.cl_graph_read_events_text(self._h, text.encode(), C.byref(n)))
        return n.value

    # ---- execution ----------------------------------------------------------------------
    def flush(self):
        _check(self._L.cl_graph_flush(self._h))

    def rerun(self):
        _check(self._L.cl_graph_rerun(self._h))

    def synchronize(self):
        _check(self._L.cl_graph_synchronize(self._h))

    def run_time(self):
        """(device ms of the runs since the previous call, runs, ticks) -- HIP events."""
        ms, r, t = C.c_double(0), C.c_int64(0), C.c_int64(0)
        _check(self._L.cl_graph_run_time(self._h, C.byref(ms), C.byref(r), C.byref(t)))
        return ms.value, r.value, t.value

    def poison_outputs(self):
        """Overwrite the result planes with 0xA5 bytes (cl_graph_debug_poison_outputs)."""
        _check(self._L.cl_graph_debug_poison_outputs(self._h))

    def phase_time(self):
        """Latest run: ((ms, ticks) before the first drain, (ms, ticks) of the drains)."""
        ms = np.zeros(2, dtype=np.float64)
        t = np.zeros(2, dtype=np.int64)
        _check(self._L.cl_graph_phase_time(self._h, _p(ms), _p(t)))
        return (float(ms[0]), int(t[0])), (float(ms[1]), int(t[1]))

    # ---- queries ------------------------------------------------------------------------
    def _get(self, fn, ctype, *args):
        v = ctype(0)
        _check(fn(self._h, *args, C.byref(v)))
        return v.value

    @property
    def num_nodes(self):
        return self._get(self._L.cl_graph_num_nodes, C.c_int32)

    @property
    def num_channels(self):
        return self._get(self._L.cl_graph_num_channels, C.c_int64)

    @property
    def num_snapshots(self):
        return self._get(self._L.cl_graph_num_snapshots, C.c_int32)

    @property
    def device_bytes(self):
        return self._get(self._L.cl_graph_device_bytes, C.c_int64)

    def channels(self):
        e = self.num_channels
        s = np.zeros(e, dtype=np.int32)
        d = np.zeros(e, dtype=np.int32)
        _check(self._L.cl_graph_channels(self._h, _p(s), _p(d)))
        return s, d

    def _node_id(self, rank, cap):
        buf = C.create_string_buffer(cap)
        _check(self._L.cl_graph_node_id(self._h, rank, buf, cap))
        return buf.value.decode()

    def node_ids(self):
        if self._ids is None:
            cap = 64
            buf = C.create_string_buffer(cap)
            out = []
            for r in range(self.num_nodes):
                rc = self._L.cl_graph_node_id(self._h, r, buf, cap)
                if rc == -7:                             # longer id: size the buffer to it
                    cap = self._get(self._L.cl_graph_node_id_length, C.c_int32, r) + 1
                    buf = C.create_string_buffer(cap)
                    rc = self._L.cl_graph_node_id(self._h, r, buf, cap)
                _check(rc)
                out.append(buf.value.decode())
            self._ids = out
        return self._ids

    def status(self):
        return self._get(self._L.cl_graph_get_status, C.c_int32)

    def time(self):
        return self._get(self._L.cl_graph_get_time, C.c_int64)

    def node_tokens_array(self):
        out = np.zeros(self.num_nodes, dtype=np.int64)
        _check(self._L.cl_graph_node_tokens(self._h, _p(out)))
        return out

    def node_tokens(self):
        return dict(zip(self.node_ids(), self.node_tokens_array().tolist()))

    def snapshot_tick(self, sid):
        return self._get(self._L.cl_graph_snapshot_tick, C.c_int32, sid)

    def collect_arrays(self, sid):
        """(tokens[N] rank order, offsets[E+1], messages) with channels in (src, dest)
        rank order; raises ClSnapError(-9) if the snapshot has not completed."""
        n, e = self.num_nodes, self.num_channels
        tok = np.zeros(n, dtype=np.int64)
        off = np.zeros(e + 1, dtype=np.int64)
        cap = 1 << 16
        while True:
            msg = np.zeros(cap, dtype=np.int64)
            rc = self._L.cl_graph_collect_snapshot(self._h, sid, _p(tok), _p(off), _p(msg), cap)
            if rc == -7 and off[e] > cap:
                cap = int(off[e])
                continue
            _check(rc)
            return tok, off, msg[:off[e]]

    def CollectSnapshot(self, snapshot_id):         # sim.go:134
        """GlobalSnapshot, messages in (dest, src, delivery) order."""
        tok, off, msg = self.collect_arrays(snapshot_id)
        ids = self.node_ids()
        src, dst = self.channels()
        order = np.lexsort((src, dst))
        msgs = [MsgSnapshot(ids[src[c]], ids[dst[c]], int(msg[k]))
                for c in order for k in range(off[c], off[c + 1])]
        return GlobalSnapshot(snapshot_id, dict(zip(ids, tok.tolist())), msgs)

    def counters(self):
        out = np.zeros(len(COUNTER_NAMES), dtype=np.int64)
        _check(self._L.cl_graph_get_counters(self._h, _p(out)))
        return dict(zip(COUNTER_NAMES, out.tolist()))

    def checksums(self):
        out = np.zeros(len(GSUM_NAMES), dtype=np.int64)
        _check(self._L.cl_graph_get_checksums(self._h, _p(out)))
        return dict(zip(GSUM_NAMES, out.tolist()))

    def snapshot_table(self, sid_lo=0, sid_hi=None):
        """SnapshotTable of the snapshots [sid_lo, sid_hi) (default: all), reduced on the
        device in one pass (cl_graph_snapshot_table): 128 bytes per snapshot reach the host."""
        if sid_hi is None:
            sid_hi = self.num_snapshots
        rows = np.zeros(max(sid_hi - sid_lo, 0), dtype=SNAP_ROW_DTYPE)
        _check(self._L.cl_graph_snapshot_table(self._h, sid_lo, sid_hi, _p(rows) if rows.size else None))
        return SnapshotTable(rows)

    def table_time(self):
        """Device ms of the latest snapshot_table call's kernels (HIP events)."""
        return self._get(self._L.cl_graph_table_time, C.c_double)

    def snapshot_wave(self, sid_lo=0, sid_hi=None, lat_bins=64, lat_width=1, depth_bins=32, origins=None):
        """SnapshotWave of the snapshots [sid_lo, sid_hi) (default: all), reduced on the device
        from the node records (cl_graph_snapshot_wave): how the marker wave of each spread over
        time and, with depth_bins > 0, how deep the tree is that it took.  origins (one tick per
        snapshot) replaces the start tick the latencies are measured from; a part of a
        partitioned run needs it, and takes depth_bins=0."""
        if sid_hi is None:
            sid_hi = self.num_snapshots
        ns = max(sid_hi - sid_lo, 0)
        spec = np.zeros(1, dtype=WAVE_SPEC_DTYPE)
        spec["lat_bins"], spec["lat_width"], spec["depth_bins"] = lat_bins, lat_width, depth_bins
        rw = len(WAVE_HEAD) + max(int(lat_bins), 0) + max(int(depth_bins), 0)
        out = np.zeros((max(ns, 1), rw), dtype=np.int64)
        org = None
        if origins is not None:
            org = np.ascontiguousarray(origins, dtype=np.int64).reshape(-1)
            if org.size != ns:
                raise ValueError(f"{org.size} origins for {ns} snapshots")
            org = np.concatenate([org, np.zeros(1, dtype=np.int64)])       # (never an empty buffer)
        _check(self._L.cl_graph_snapshot_wave(self._h, sid_lo, sid_hi, _p(spec), None if org is None else _p(org),
                                              _p(out), ns * rw))
        return SnapshotWave(out[:ns], lat_bins, lat_width, depth_bins)

    def wave_time(self):
        """(device ms of the latest snapshot_wave call's kernels, its pointer-doubling rounds)."""
        ms, rounds = C.c_double(0), C.c_int32(0)
        _check(self._L.cl_graph_wave_time(self._h, C.byref(ms), C.byref(rounds)))
        return ms.value, rounds.value

    def set_wave_scratch(self, nbytes=0):
        """Bytes of device scratch one chunk of snapshot ids may take in snapshot_wave and
        snapshot_tree (0: the default, 256 MiB).  The results do not depend on it."""
        _check(self._L.cl_graph_set_wave_scratch(self._h, nbytes))

    def _tree_planes(self, sid_lo, sid_hi, ticks, width):
        """(parent, tick | None) int32[ns, width] of one cl_graph_snapshot_tree call."""
        ns = max(sid_hi - sid_lo, 0)
        parent = np.zeros((max(ns, 1), width), dtype=np.int32)
        tick = np.zeros((max(ns, 1), width), dtype=np.int32) if ticks else None
        _check(self._L.cl_graph_snapshot_tree(self._h, sid_lo, sid_hi, _p(parent), None if tick is None else _p(tick)))
        return parent[:ns], None if tick is None else tick[:ns]

    def snapshot_tree(self, sid_lo=0, sid_hi=None, ticks=True):
        """One MarkerTree per snapshot of [sid_lo, sid_hi) (default: all): the creating sender
        and, with ticks, the creation epoch of every node, packed on the device
        (cl_graph_snapshot_tree)."""
        if sid_hi is None:
            sid_hi = self.num_snapshots
        parent, tick = self._tree_planes(sid_lo, sid_hi, ticks, self.num_nodes)
        return [MarkerTree(parent[r], None if tick is None else tick[r], 0, sid_lo + r) for r in range(len(parent))]

    def _collect_sparse(self, sid_lo, sid_hi, complete=None, row_offsets=None, channel=None, count=None, ent_cap=0,
                        msg_tokens=None, msg_cap=0, tokens=None):
        """One cl_graph_collect_sparse call: (return code, info record)."""
        ptr = lambda a: None if a is None else _p(a)  # noqa: E731
        info = np.zeros(1, dtype=SPARSE_INFO_DTYPE)
        rc = self._L.cl_graph_collect_sparse(self._h, sid_lo, sid_hi, ptr(complete), ptr(row_offsets), ptr(channel),
                                             ptr(count), ent_cap, ptr(msg_tokens), msg_cap, ptr(tokens), _p(info))
        return rc, info[0]

    def collect_sparse(self, sid_lo=0, sid_hi=None, tokens=False, payloads=True):
        """SparseSnapshots of the snapshots [sid_lo, sid_hi) (default: all): the entries
        (channel, count) of the completed ones, compacted on the device, with their payloads
        (payloads=True) and the plane of recorded node tokens (tokens=True).  One sizing call
        and one fetch (cl_graph_collect_sparse); nothing sized by the channel count reaches
        the host."""
        if sid_hi is None:
            sid_hi = self.num_snapshots
        ns = max(sid_hi - sid_lo, 0)
        complete = np.zeros(ns, dtype=np.int32)
        row_offsets = np.zeros(ns + 1, dtype=np.int64)
        rc, info = self._collect_sparse(sid_lo, sid_hi, complete, row_offsets)      # the sizing call
        if rc != E_LIMIT:
            _check(rc)
        ne, nm = int(info["n_entries"]), int(info["n_msgs"])
        lo, hi = int(info["node_lo"]), int(info["node_hi"])
        channel, count = np.zeros(ne, dtype=np.int32), np.zeros(ne, dtype=np.int32)
        msg = np.zeros(nm, dtype=np.int32) if payloads else None
        tok = np.zeros((ns, hi - lo), dtype=np.int32) if tokens else None
        if ns and (rc == E_LIMIT or payloads or tokens):
            rc, info = self._collect_sparse(sid_lo, sid_hi, complete, row_offsets, channel, count, ne, msg, nm, tok)
            _check(rc)
        if msg is None and info["unit_payloads"]:
            msg = np.ones(nm, dtype=np.int32)          # (no history: every payload is 1)
        return SparseSnapshots(sid_lo, complete, row_offsets, channel, count, msg, tok, lo, hi)

    def sparse_time(self):
        """Device ms of the latest collect_sparse call's kernels (HIP events)."""
        return self._get(self._L.cl_graph_sparse_time, C.c_double)

    def _snapshot_profile(self, sid_lo, sid_hi, spec, use=None, origins=None, head=None, used=None, node_rows=None,
                          entries=None, ent_cap=0):
        """One cl_graph_snapshot_profile call: the return code."""
        ptr = lambda a: None if a is None else _p(a)  # noqa: E731
        return self._L.cl_graph_snapshot_profile(self._h, sid_lo, sid_hi, ptr(spec), ptr(use), ptr(origins), ptr(head),
                                                 ptr(used), ptr(node_rows), ptr(entries), ent_cap)

    def snapshot_profile(self, sid_lo=0, sid_hi=None, use=None, nodes=True, min_msgs=1, msg_bins=64, msg_width=1,
                         origins=None, max_entries=1 << 16):
        """SnapshotProfile of the snapshots [sid_lo, sid_hi) (default: all), reduced on the device
        over the used ones (cl_graph_snapshot_profile): per channel the recorded messages, their
        payloads, the snapshots with one and the peak with its sid; per node (nodes=True) the
        moments of its recorded balance and of its creation latency.  use (one flag per snapshot)
        masks the range, e.g. from the table; incomplete snapshots are never used.  Channels with
        msgs >= min_msgs come back as entries: the call is made with max_entries capacity and once
        more with the exact size if they do not fit.  origins (one tick per snapshot) replaces
        the start ticks; a part of a partitioned run needs it with nodes=True."""
        if sid_hi is None:
            sid_hi = self.num_snapshots
        ns = max(sid_hi - sid_lo, 0)
        spec = np.zeros(1, dtype=PROFILE_SPEC_DTYPE)
        spec["msg_bins"], spec["msg_width"], spec["min_msgs"] = msg_bins, msg_width, min_msgs
        nb = min(max(int(msg_bins), 0), PROFILE_MAX_BINS)
        head = np.zeros(len(PROFILE_HEAD) + nb, dtype=np.int64)
        used = np.zeros(ns + 1, dtype=np.int32)                                # (never an empty buffer)
        mask = org = None
        if use is not None:
            mask = (np.asarray(use).reshape(-1) != 0).astype(np.int32)
            if mask.size != ns:
                raise ValueError(f"{mask.size} use flags for {ns} snapshots")
            mask = np.concatenate([mask, np.zeros(1, dtype=np.int32)])
        if origins is not None:
            org = np.ascontiguousarray(origins, dtype=np.int64).reshape(-1)
            if org.size != ns:
                raise ValueError(f"{org.size} origins for {ns} snapshots")
            org = np.concatenate([org, np.zeros(1, dtype=np.int64)])
        rows = np.zeros(max(self.num_nodes, 1), dtype=PROFILE_NODE_DTYPE) if nodes else None
        cap = max(int(max_entries), 0)
        entries = np.zeros(max(cap, 1), dtype=PROFILE_ENTRY_DTYPE)
        rc = self._snapshot_profile(sid_lo, sid_hi, spec, mask, org, head, used, rows, entries, cap)
        if rc == E_LIMIT:                                                      # the head is written: the exact size
            cap = int(head[_PF["entries"]])
            entries = np.zeros(max(cap, 1), dtype=PROFILE_ENTRY_DTYPE)
            rc = self._snapshot_profile(sid_lo, sid_hi, spec, mask, org, head, used, rows, entries, cap)
        _check(rc)
        width = int(head[_PF["node_hi"]] - head[_PF["node_lo"]])
        if nodes and ns == 0:                                                  # (nothing ran: the identities)
            rows[:] = (0, 0, np.iinfo(np.int64).max, np.iinfo(np.int64).min, 0, np.iinfo(np.int64).min, 0, 0)
        return SnapshotProfile(sid_lo, used[:ns], head[:len(PROFILE_HEAD)], head[len(PROFILE_HEAD):],
                               entries[:int(head[_PF["entries"]])], rows[:width] if nodes else None,
                               None if org is None else org[:ns], msg_width, min_msgs)

    def profile_time(self):
        """Device ms of the latest snapshot_profile call's kernels (HIP events)."""
        return self._get(self._L.cl_graph_profile_time, C.c_double)

    def set_profile_slices(self, slices=0):
        """Slices of the used snapshots the profile's passes run in (0: automatic).  The results
        do not depend on it."""
        _check(self._L.cl_graph_set_profile_slices(self._h, slices))

    # ---- restore: a run that begins in a recorded cut (cl_graph_restore) ----------------
    def restore(self, sid):
        """A new, independent GraphSim whose time-0 state is the completed snapshot sid of this
        run: the same topology, node tokens = the snapshot's tokenMap, every channel's queue
        holding its recorded messages (head first, delay draws in (channel, position) order
        under the new graph's delay source), built and seeded by kernels on the device.  It
        inherits the device, limits, push lanes and delay source; traffic, trace and further
        events are set on it like on any graph.  ClSnapError: E_INVALID for an unknown sid,
        E_NOT_COMPLETE if it has not completed, E_STATE for a partitioned source or a run that is
        not OK.  A partitioned run is restored from through its merged cut:
        PartitionedGraphSim.collect_sparse(tokens=True), SparseSnapshots.cut, restore_cut; and a
        restored graph runs partitioned when PartitionedGraphSim is made of it (from_cut, restore)."""
        h = C.c_void_p()
        _check(self._L.cl_graph_restore(self._h, sid, C.byref(h)))
        return GraphSim._of_handle(self._L, h, self.device, self._ids)

    def topology_key(self):
        """topology_key of this graph's own topology (freezes it like any call that needs rank
        order; host only)."""
        if getattr(self, "_key", None) is None:
            self._key = topology_key(self.num_nodes, *self.channels())
        return self._key

    def cut(self, sid, topology=False):
        """The completed snapshot sid as a SnapshotCut on the host (collect_sparse of the one
        sid with tokens and payloads); with topology=True it carries the channel list and the
        node ids, which SnapshotCut.save then keeps and from_cut needs.
        ClSnapError(E_NOT_COMPLETE) if the snapshot has not completed."""
        return self.collect_sparse(sid, sid + 1, tokens=True).cut(sid, sim=self, topology=topology)

    def restore_cut(self, cut):
        """restore from a cut held on the host (cl_graph_restore_cut): a saved one, the merged
        cut of a partitioned run, or one written by hand.  This graph is the template: it
        supplies the topology, device, limits, push lanes and delay source, need never have run,
        is not changed, and may be destroyed afterwards.  ValueError if the cut's topology key
        or channel count is not this topology's; the arrays are then uploaded and checked by a
        kernel, and ClSnapError(E_INVALID) names the first element that breaks a rule
        (include/clgraph.h).  The result is a graph as restore returns it."""
        if not isinstance(cut, SnapshotCut):
            raise TypeError("restore_cut takes a SnapshotCut")
        if cut.n_channels != self.num_channels or cut.topology_key != self.topology_key():
            raise ValueError("the cut belongs to another topology (n_channels or topology_key differ)")
        ip = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        rec = GraphCut(cut.source_sid, cut.tokens.size, ip(cut.tokens), cut.channel.size, ip(cut.channel),
                       ip(cut.count), cut.msgs if cut.msg_tokens is None else cut.msg_tokens.size, ip(cut.msg_tokens))
        h = C.c_void_p()
        _check(self._L.cl_graph_restore_cut(self._h, C.byref(rec), C.byref(h)))
        return GraphSim._of_handle(self._L, h, self.device, self._ids)

    @classmethod
    def from_cut(cls, cut, device=0, fifo_slots=16, max_snapshots=0, max_drain_ticks=10000):
        """A graph restored from a cut that carries its topology (GraphSim.cut(sid,
        topology=True), SnapshotCut.load): what a fresh process starts from.  The template is
        built from the saved channel list and ids -- in bulk (set_topology) when the ids are "N" +
        the rank zero-padded to one width, else node by node -- and must come out in the saved
        rank order (ValueError otherwise).  Set the delay source on the result before its first flush, as on
        any restored graph."""
        return cls.template_of_cut(cut, device, fifo_slots, max_snapshots, max_drain_ticks).restore_cut(cut)

    @classmethod
    def template_of_cut(cls, cut, device=0, fifo_slots=16, max_snapshots=0, max_drain_ticks=10000):
        """The template from_cut restores on: a fresh graph of the topology the cut carries, never
        flushed (host only).  ValueError for a cut without topology or ids out of rank order."""
        if not cut.has_topology:
            raise ValueError("from_cut needs a cut saved with topology=True")
        n = cut.tokens.size
        t = cls(device, fifo_slots, max_snapshots, max_drain_ticks)
        w = _bulk_id_width(cut.ids)
        if w:
            t.set_topology(cut.tokens, cut.src, cut.dst, id_width=w)
            # (set_topology names rank r "N" + r padded to w: the saved ids, as just checked; the
            # ends are read back, the rest are the engine's by the same rule)
            same = t.num_nodes == n and all(t._get(t._L.cl_graph_node_id_length, C.c_int32, r) == w + 1 and
                                            t._node_id(r, w + 2) == cut.ids[r].decode() for r in (0, n - 1))
        else:
            ids = [i.decode() for i in cut.ids.tolist()]
            for v in range(n):
                t.AddNode(ids[v], int(cut.tokens[v]))
            for a, b in zip(cut.src.tolist(), cut.dst.tolist()):
                t.AddLink(ids[a], ids[b])
            same = n > 0 and t.node_ids() == ids
        if not same:
            raise ValueError("the saved node ids are not in rank order")
        return t

    @property
    def seed_info(self):
        """The seed of a restored graph as a dict (SEED_INFO_FIELDS); ClSnapError for a graph
        not made by restore."""
        info = np.zeros(1, dtype=SEED_INFO_DTYPE)
        _check(self._L.cl_graph_seed_info_of(self._h, _p(info)))
        return {f: int(info[0][f]) for f in SEED_INFO_FIELDS if f != "reserved"}

    def restore_time(self):
        """(device ms of the kernels of the restore call that made this graph, device ms of the
        seed kernel of its latest run from the initial state -- 0.0 before any)."""
        build, seed = C.c_double(0), C.c_double(0)
        _check(self._L.cl_graph_restore_time(self._h, C.byref(build), C.byref(seed)))
        return build.value, seed.value

    # ---- device event trace: the reference's debug Logger (logger.go:12-76) ------------
    def trace_enable(self, capacity=1 << 16):
        """Record the Logger from the next run on (capacity records; 0 = off)."""
        _check(self._L.cl_graph_trace_enable(self._h, capacity))

    def trace(self):
        """LogEvents in Logger order: (epoch, kind, node rank, other rank | -1, data,
        nodeTokens); kinds LOG_* (include/clsnap.h CL_LOG_*)."""
        n = C.c_int32(0)
        _check(self._L.cl_graph_trace_read(self._h, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 6), dtype=np.int32)
        _check(self._L.cl_graph_trace_read(self._h, _p(out), n.value, C.byref(n)))
        return [tuple(int(x) for x in r) for r in out[:n.value]]

    def pretty_print(self):
        """Logger.PrettyPrint (logger.go:55-64) as text."""
        return format_log(self.node_ids(), self.trace())


def bucket_capacity(src, dst, span, world):
    """Rows per device-exchange bucket of the partitioned mode: the most nodes of one rank
    with a channel into another rank's nodes (rank r owns node ranks [r * span, (r + 1) *
    span)).  Each sender delivers at most one packet per tick (sim.go:90), so this bounds
    the deliveries from r to q, the broadcast reports q sends r about r's senders, and r's
    replies to them."""
    w = world
    key = np.unique(np.asarray(src, dtype=np.int64) * w + np.asarray(dst, dtype=np.int64) // span)
    pair = (key // w) // span * w + key % w
    cnt = np.bincount(pair, minlength=w * w).reshape(w, w)
    np.fill_diagonal(cnt, 0)
    return max(int(cnt.max()), 1)


class PartitionedGraphSim:
    """ONE simulation over a graph split into contiguous node-rank ranges, one range per
    process / GPU (graph-partitioned mode, DESIGN.md §11, include/clgraph.h
    cl_graph_part_*).  Every rank builds the same topology and program; per tick the
    ranks exchange deliveries, broadcast-trigger reports, trigger totals and draw replies
    with dist.exchange_rows / allgather_ints (RCCL over xGMI with exchange_device="cuda",
    gloo on host tensors).  Results are gathered on every rank: the run equals the
    whole-graph engine's and the oracle's bit for bit (tests/test_partition_gpu.py).

    There is no reference counterpart (the reference runs one process); the exchange
    steps restate the tick of sim.go:71-95 across ranks (tests/partition_model.py is the
    same protocol on the CPU).

    sim is a GraphSim before its first event.  A restored one (GraphSim.restore / restore_cut /
    from_cut) begins in its cut: this rank queues the messages of its own nodes' out-channels
    (cl_graph_part_begin_seeded), and seed_share is the slice (entry lo, entry hi, message lo,
    message hi) of the cut it took -- None for a run from the topology's initial state."""

    def __init__(self, sim, rank, world, exchange_device="cpu", transport="host"):
        from . import dist as D
        if transport not in ("host", "device"):
            raise ValueError(f"transport {transport!r}: 'host' or 'device'")
        self.D, self.g, self.rank, self.world = D, sim, rank, world
        self.dev = exchange_device
        self.transport = transport
        n = sim.num_nodes
        blocks = -(-n // 256)
        per = -(-blocks // world)
        self.span = per * 256                    # node ranks per rank, block-aligned
        self.lo, self.hi = min(n, rank * self.span), min(n, (rank + 1) * self.span)
        if self.lo >= self.hi:
            raise ValueError(f"{world} ranks over {blocks} node blocks of 256: rank {rank} would own no nodes")
        self.n = n
        self._L = sim._L
        # a restored graph begins in its cut: this rank queues its own channels' share of the seed
        info = np.zeros(1, dtype=SEED_INFO_DTYPE)
        self.seed_share = None
        if self._L.cl_graph_seed_info_of(sim._h, _p(info)) == 0:
            _check(self._L.cl_graph_part_begin_seeded(sim._h, self.lo, self.hi))
            share = np.zeros(4, dtype=np.int64)
            _check(self._L.cl_graph_part_seed_share(sim._h, _p(share)))
            self.seed_share = tuple(int(x) for x in share)
        else:
            _check(self._L.cl_graph_part_begin(sim._h, self.lo, self.hi))
        self.time = 0
        self.n_sids = 0
        self._frozen = 0
        if transport == "device":
            self._dev_setup()

    @property
    def frozen(self):
        """Nonzero once the run stopped (every rank stops at the same step).  The device
        transport decides it on the device (cl_graph_part_dev_bases): read back here."""
        return self.g.status() if self.transport == "device" else self._frozen

    # ---- device-resident exchange (clgraph.h cl_graph_part_dev_*) ----------------------
    def bucket_capacity(self):
        """Rows per exchange bucket for this graph and rank split (bucket_capacity below)."""
        src, dst = self.g.channels()
        return bucket_capacity(src, dst, self.span, self.world)

    def _dev_setup(self):
        import torch
        dev = torch.device("cuda", self.g.device)
        self.cap = self.bucket_capacity()
        rows = self.world * (self.cap + 1)
        self._send = torch.zeros(2 * rows, dtype=torch.int64, device=dev)    # 16-B rows
        self._recv = torch.zeros_like(self._send)
        self._tsend = torch.zeros(4, dtype=torch.int64, device=dev)
        self._trecv = torch.zeros(4 * self.world, dtype=torch.int64, device=dev)
        self._stream = torch.cuda.Stream(device=dev)
        self.g._stream_ref = self._stream          # (outlives the engine's use of it)
        _check(self._L.cl_graph_set_stream(self.g._h, C.c_void_p(self._stream.cuda_stream)))
        _check(self._L.cl_graph_part_dev_bind(self.g._h, self.world, self.rank, self.span, self.cap,
                                              C.c_void_p(self._send.data_ptr()), C.c_void_p(self._recv.data_ptr()),
                                              C.c_void_p(self._tsend.data_ptr()), C.c_void_p(self._trecv.data_ptr())))

    def _a2a(self):
        """Bucket q of send to rank q, rank q's bucket for this rank into recv bucket q (RCCL
        on the device buffers; gloo rehearsals stage them through host memory)."""
        import torch
        import torch.distributed as dist
        with torch.cuda.stream(self._stream):
            if self.dev == "cuda":
                dist.all_to_all_single(self._recv, self._send)
            else:
                h = self._send.cpu()                # (after the engine's launches on this stream)
                r = torch.empty_like(h)
                dist.all_to_all_single(r, h)
                self._recv.copy_(r)

    def _gather(self):
        import torch
        import torch.distributed as dist
        with torch.cuda.stream(self._stream):
            if self.dev == "cuda":
                dist.all_gather_into_tensor(self._trecv, self._tsend)
            else:
                h = self._tsend.cpu()
                out = [torch.empty_like(h) for _ in range(self.world)]
                dist.all_gather(out, h)
                self._trecv.copy_(torch.cat(out))

    def _dev_finish(self, step):
        """reports -> tally -> totals -> bases + replies -> push, all on the device."""
        L, h = self._L, self.g._h
        self._a2a()
        _check(L.cl_graph_part_dev_tally(h, step))
        self._gather()
        _check(L.cl_graph_part_dev_bases(h))
        self._a2a()
        _check(L.cl_graph_part_dev_push(h, step))

    def owner(self, v):
        return np.asarray(v) // self.span

    def _by_owner(self, rows, col):
        if len(rows) == 0:
            return [np.zeros((0, rows.shape[1] if rows.ndim == 2 else 1), dtype=np.int64)] * self.world
        own = self.owner(rows[:, col])
        return [rows[own == r].astype(np.int64) for r in range(self.world)]

    def _finish_step(self, step, reports_by_src):
        """tally -> allgather totals -> bases -> replies -> push (the end of a tick, and the
        step-0 traffic with no reports)."""
        mine = np.concatenate([r for r in reports_by_src if len(r)] or [np.zeros((0, 2), dtype=np.int64)])
        rep = np.ascontiguousarray(mine, dtype=np.int32)
        tot = np.zeros(3, dtype=np.int64)
        _check(self._L.cl_graph_part_tally(self.g._h, step, _p(rep), len(rep), _p(tot)))
        allt = self.D.allgather_ints(tot.tolist(), self.dev)
        frozen = int(allt[:, 2].max())
        if frozen:                  # a device froze (its totals are stale): every device stops here
            if not tot[2]:
                _check(self._L.cl_graph_part_freeze(self.g._h, frozen))
            self._frozen = frozen
            return
        r = self.rank
        bases = np.array([allt[:r, 0].sum(), allt[:, 0].sum(), allt[:r, 1].sum(), allt[:, 1].sum()], dtype=np.int64)
        s0 = np.ascontiguousarray(rep[:, 0]) if len(rep) else np.zeros(0, dtype=np.int32)
        draw0 = np.zeros(max(len(s0), 1), dtype=np.int64)
        _check(self._L.cl_graph_part_bases(self.g._h, _p(bases), _p(s0), len(s0), _p(draw0)))
        replies, o = [], 0
        for src_rows in reports_by_src:            # back to the ranks that reported them
            k = len(src_rows)
            replies.append(np.stack([s0[o:o + k].astype(np.int64), draw0[o:o + k]], axis=1) if k
                           else np.zeros((0, 2), dtype=np.int64))
            o += k
        back = self.D.exchange_rows(replies, 2, self.dev)
        rows = np.ascontiguousarray(np.concatenate([b for b in back if len(b)] or [np.zeros((0, 2), dtype=np.int64)]),
                                    dtype=np.int64)
        _check(self._L.cl_graph_part_push(self.g._h, step, _p(rows), len(rows)))

    def start(self):
        """The step-0 traffic (the whole-graph engine runs it at reset)."""
        if self.transport == "device":
            _check(self._L.cl_graph_part_dev_seal(self.g._h))      # no reports
            self._dev_finish(0)
            return
        self._finish_step(0, [np.zeros((0, 2), dtype=np.int64)] * self.world)

    def start_snapshot_rank(self, node):            # sim.go:105 (called on every rank)
        sid = C.c_int32(-1)
        _check(self._L.cl_graph_part_snapshot(self.g._h, node, C.byref(sid)))
        self.n_sids += 1
        return sid.value

    def tick(self):                                 # sim.go:71-95 across the ranks
        h = self.g._h
        if self.transport == "device":              # no host round trip (a frozen run's kernels return)
            _check(self._L.cl_graph_part_dev_pick(h))
            self.time += 1
            self._a2a()
            _check(self._L.cl_graph_part_dev_receive(h))
            self._dev_finish(self.time)
            return
        if self._frozen:                            # (the run stopped on every rank)
            return
        out = np.zeros((max(self.hi - self.lo, 1), 4), dtype=np.int32)
        m = C.c_int64(0)
        _check(self._L.cl_graph_part_pick(h, _p(out), out.shape[0], C.byref(m)))
        self.time += 1
        inbox = self.D.exchange_rows(self._by_owner(out[:m.value], 1), 4, self.dev)
        rows = np.ascontiguousarray(np.concatenate([b for b in inbox if len(b)] or [np.zeros((0, 4), dtype=np.int64)]),
                                    dtype=np.int32)
        reps = np.zeros((max(len(rows), 1), 2), dtype=np.int32)
        q = C.c_int64(0)
        _check(self._L.cl_graph_part_receive(h, _p(rows), len(rows), _p(reps), reps.shape[0], C.byref(q)))
        got = self.D.exchange_rows(self._by_owner(reps[:q.value], 0), 2, self.dev)
        self._finish_step(self.time, got)

    def run_program(self, steps, snap_step=(), snap_rank=()):
        """The synthetic program: for step k, snapshots scheduled at k,
        one tick (whose end pushes the traffic of step k + 1)."""
        self.start()
        si = 0
        for k in range(steps):
            while si < len(snap_step) and snap_step[si] == k:
                self.start_snapshot_rank(int(snap_rank[si]))
                si += 1
            self.tick()

    def completion_ticks(self):
        """Global completion tick of each snapshot (-1 if some rank's nodes are not all done):
        the latest of the ranks' local completion ticks."""
        loc = [self.g.snapshot_tick(s) for s in range(self.n_sids)]
        allc = self.D.allgather_ints(loc or [0], self.dev)[:, :len(loc)]
        return [int(allc[:, s].max()) if (allc[:, s] >= 0).all() else -1 for s in range(len(loc))]

    def drain(self, max_ticks=10000):
        """test_common.go:123-137 across the ranks: tick until every snapshot started so far
        has completed on every rank, then maxDelay + 1 more ticks."""
        for _ in range(max_ticks + 1):
            if self.frozen:
                return False
            if all(x >= 0 for x in self.completion_ticks()):
                for _ in range(6):
                    self.tick()
                return True
            self.tick()
        return False

    def snapshot_table(self):
        """The whole run's SnapshotTable on every rank: the parts' tables (each rank's nodes and
        the channels into them), all-gathered and merged."""
        mine = self.g.snapshot_table(0, self.n_sids)
        words = mine.rows.view(np.int64).ravel()
        allw = self.D.allgather_ints(words.tolist() or [0], self.dev)[:, :words.size]
        parts = [SnapshotTable(np.ascontiguousarray(w).view(SNAP_ROW_DTYPE)) for w in allw]
        out = parts[0]
        for t in parts[1:]:
            out = out.merge(t)
        return out

    def snapshot_wave(self, sid_lo=0, sid_hi=None, lat_bins=64, lat_width=1):
        """The whole run's latency profile (SnapshotWave with depth_bins=0) on every rank: the
        origins are the start ticks of the merged snapshot_table, each part reduces its own nodes
        against them, and the parts' rows are all-gathered and merged.  The depth needs the whole
        tree: snapshot_tree(sid).depth()."""
        if sid_hi is None:
            sid_hi = self.n_sids
        origins = self.snapshot_table().rows["start_tick"][sid_lo:sid_hi]
        mine = self.g.snapshot_wave(sid_lo, sid_hi, lat_bins, lat_width, 0, origins=origins)
        words = mine.rows.ravel()
        allw = self.D.allgather_ints(words.tolist() or [0], self.dev)[:, :words.size]
        out = None
        for w in allw:
            part = SnapshotWave(np.ascontiguousarray(w), lat_bins, lat_width, 0)
            out = part if out is None else out.merge(part)
        return out

    def snapshot_tree(self, sid, ticks=True):
        """The whole MarkerTree of snapshot sid on every rank: the parts' planes (each rank's
        nodes; the parents are global ranks) all-gathered in rank order."""
        parent, tick = self.g._tree_planes(sid, sid + 1, ticks, self.hi - self.lo)
        mine = np.concatenate([parent[0], tick[0]] if ticks else [parent[0]]).astype(np.int64)
        pad = np.full((2 if ticks else 1) * self.span - mine.size, -2, dtype=np.int64)   # (equal lengths)
        allw = self.D.allgather_ints(np.concatenate([mine, pad]).tolist(), self.dev)
        ps, ts = [], []
        for r, w in enumerate(allw):
            k = min(self.n, (r + 1) * self.span) - min(self.n, r * self.span)
            ps.append(w[:k])
            ts.append(w[k:2 * k])
        return MarkerTree(np.concatenate(ps), np.concatenate(ts) if ticks else None, 0, sid)

    def collect_sparse(self, sid_lo=0, sid_hi=None, tokens=False, payloads=True):
        """The whole run's SparseSnapshots on every rank: the parts' sparse collects (each
        rank's nodes and the channels into them), gathered and merged (SparseSnapshots.merge)."""
        import torch.distributed as dist
        mine = self.g.collect_sparse(sid_lo, self.n_sids if sid_hi is None else sid_hi, tokens, payloads)
        fields = ("sid_lo", "complete", "row_offsets", "channel", "count", "msg_tokens", "tokens", "node_lo",
                  "node_hi")
        allp = [None] * self.world
        dist.all_gather_object(allp, tuple(getattr(mine, f) for f in fields))
        return SparseSnapshots.merge([SparseSnapshots(*p) for p in allp])

    def snapshot_profile(self, sid_lo=0, sid_hi=None, use=None, nodes=True, min_msgs=1, msg_bins=64, msg_width=1,
                         max_entries=1 << 16, parts=False):
        """The whole run's SnapshotProfile on every rank (a collective): the used snapshots are the
        caller's mask AND the completion of the merged snapshot_table, the origins its start ticks;
        each part profiles its own nodes and the channels into them, and the parts are gathered and
        merged (SnapshotProfile.merge).  parts=True: (merged, [the parts in rank order])."""
        import torch.distributed as dist
        if sid_hi is None:
            sid_hi = self.n_sids
        rows = self.snapshot_table().rows[sid_lo:sid_hi]
        mask = rows["complete_tick"] >= 0
        if use is not None:
            mask = mask & (np.asarray(use).reshape(-1) != 0)
        mine = self.g.snapshot_profile(sid_lo, sid_hi, mask, nodes, min_msgs, msg_bins, msg_width, rows["start_tick"],
                                       max_entries)
        fields = ("sid_lo", "used", "head", "hist", "entries", "node", "origins", "msg_width", "min_msgs")
        allp = [None] * self.world
        dist.all_gather_object(allp, tuple(getattr(mine, f) for f in fields))
        got = [SnapshotProfile(*p) for p in allp]
        merged = SnapshotProfile.merge(got)
        return (merged, got) if parts else merged

    # ---- restore: a partitioned run that begins in a recorded cut (cl_graph_part_begin_seeded) ----
    def cut(self, sid, topology=False):
        """The completed snapshot sid of the whole run as a SnapshotCut, on every rank (a
        collective: collect_sparse of the one sid with tokens, merged); GraphSim.cut's arguments."""
        return self.collect_sparse(sid, sid + 1, tokens=True).cut(sid, sim=self.g, topology=topology)

    @classmethod
    def from_cut(cls, cut, rank, world, template=None, configure=None, exchange_device="cpu", transport="host",
                 **limits):
        """This rank's part of a partitioned run whose time-0 state is the cut: every rank holds
        the whole cut (like every array of the mode), restores it on its own unpartitioned
        template and queues the messages of its own nodes' out-channels, with their draw indices
        among all of the cut's (seed_share: the slice of entries and messages).  world need not
        be that of the run that wrote the cut: GraphSim.cut of an unpartitioned run serves too.
        template: a GraphSim of the topology, as restore_cut takes it (limits, push lanes, delay
        source); None builds one from a cut with topology=True (GraphSim.template_of_cut, **limits
        its device, fifo_slots, max_snapshots, max_drain_ticks).  configure(r) runs on the restored
        GraphSim before the partition begins: set_delay_hash / set_delay_schedule, set_traffic,
        set_limits.  start() then runs the step-0 traffic and, for a cut that cannot be seeded
        (status FIFO_OVERFLOW or DELAY_EXHAUSTED), stops every rank at time 0."""
        if template is None:
            if not cut.has_topology:
                raise ValueError("from_cut needs a template, or a cut saved with topology=True")
            template = GraphSim.template_of_cut(cut, **limits)
        elif limits:
            raise ValueError("the limits are the template's")
        r = template.restore_cut(cut)
        if configure is not None:
            configure(r)
        return cls(r, rank, world, exchange_device=exchange_device, transport=transport)

    def restore(self, sid, template=None, configure=None, **limits):
        """A new partitioned run over the same ranks, transport and exchange device whose time-0
        state is the completed snapshot sid of this one (a collective: cut, then from_cut)."""
        return PartitionedGraphSim.from_cut(self.cut(sid, topology=template is None), self.rank, self.world, template,
                                            configure, self.dev, self.transport, **limits)

    def results(self):
        """(status, final tokens[n], completion ticks, counters, {sid: (tokens[n], offsets,
        payloads)} for completed snapshots), gathered on every rank."""
        import torch.distributed as dist
        g = self.g
        cnt = g.counters()
        st = g.status()
        tok = g.node_tokens_array()[self.lo:self.hi]
        ct = self.completion_ticks()
        src, dst = g.channels()
        mine = (dst >= self.lo) & (dst < self.hi)
        snaps = {}
        for sid, c in enumerate(ct):
            if c < 0:
                continue
            t, off, msg = g.collect_arrays(sid)
            per = [msg[off[k]:off[k + 1]] for k in np.nonzero(mine)[0]]
            snaps[sid] = (t[self.lo:self.hi], np.nonzero(mine)[0], per)
        allr = [None] * self.world
        dist.all_gather_object(allr, (st, tok, cnt, snaps))
        status = max(r[0] for r in allr)
        tokens = np.concatenate([r[1] for r in allr])
        counters = {k: sum(r[2][k] for r in allr) for k in ("push", "peek", "pop_tok", "pop_mk", "recorded")}
        counters["completed"] = sum(1 for x in ct if x >= 0)
        out = {}
        e = len(src)
        for sid in snaps:
            stok = np.concatenate([r[3][sid][0] for r in allr])
            lists = [None] * e
            for r in allr:
                for c, m in zip(r[3][sid][1], r[3][sid][2]):
                    lists[c] = m
            off = np.zeros(e + 1, dtype=np.int64)
            off[1:] = np.cumsum([len(x) for x in lists])
            vals = np.concatenate(lists) if e else np.zeros(0, dtype=np.int64)
            out[sid] = (stok, off, vals)
        return status, tokens, ct, counters, out
