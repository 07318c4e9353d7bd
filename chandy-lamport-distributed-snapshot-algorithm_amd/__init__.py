"""MI355X-native batch engine for the reference's Chandy-Lamport simulator hot path.

The reference (Go package ``chandy_lamport``) simulates one run: ``ChandyLamportSim``
(sim.go) with ``AddNode/AddLink/ProcessEvent/Tick/StartSnapshot/CollectSnapshot`` and
nodes exchanging tokens and markers over FIFO channels (node.go, queue.go).  This
package runs ``n_instances`` such simulations at once on one gfx950 GPU through the C
ABI in ``include/clsnap.h`` (library ``lib/libclsnap.so``, built in-tree).  Each
instance is the reference run under its own delay stream; by default instance ``i``
uses Go's ``rand.Seed(seed_base + i)`` stream, so instance 0 with the reference seed
reproduces the reference's golden snapshots.

The Python layer is a thin mirror of the reference API (same method names and argument
meaning); there is no CPU fallback: if the library or a gfx950 GPU is missing, calls
that need them raise ``ClSnapError``.
"""
import ctypes as C
import os
from fractions import Fraction

import numpy as np

__all__ = ["ChandyLamportSim", "SnapshotStats", "STATS_LAYOUT_FIELDS", "SnapshotSelection", "SELECT_CLAUSE_DTYPE",
           "InstanceSet", "SnapshotCrosstab", "CROSSTAB_AXIS_DTYPE", "SnapshotGroups", "GROUP_TERM_DTYPE", "group_key",
           "SnapshotTopK", "SnapshotQuantiles", "QUANTILE_DTYPE", "ORDER_MAX_K", "ORDER_MAX_QUANTILES",
           "order_plane_device", "quantile_rank",
"GlobalSnapshot", "MsgSnapshot", "PassTokenEvent", "SnapshotEvent",
           "ClSnapError", "lib", "go_delay_schedule", "go_delay_schedule_device", "go_delay_schedule_jump",
           "DELAYGEN_MAX_DRAWS", "go_int63", "go_intn", "REFERENCE_SEED",
           "INST_OK", "INST_FATAL_INSUFFICIENT_TOKENS", "INST_FATAL_UNKNOWN_DEST",
           "INST_FIFO_OVERFLOW", "INST_HANG", "INST_DELAY_EXHAUSTED", "COUNTER_NAMES",
           "SUM_NAMES", "MAX_DELAY", "E_INVALID", "E_UNKNOWN_NODE", "E_DUPLICATE_NODE", "E_PARSE",
           "E_IO", "E_DEVICE", "E_LIMIT", "E_STATE", "E_NOT_COMPLETE"]

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libclsnap.so")
if os.environ.get("CLSNAP_VARIANT"):  # diagnostic ablation builds (Makefile `variant`)
    LIB_PATH = os.path.join(HERE, "lib", f"libclsnap_{os.environ['CLSNAP_VARIANT']}.so")

REFERENCE_SEED = 8053172852482175523 + 1  # snapshot_test.go:9,20 rand.Seed(seed + 1)
MAX_DELAY = 5                              # sim.go:10
DELAYGEN_MAX_DRAWS = 4096                  # include/clsnap.h CL_DELAYGEN_MAX_DRAWS

(INST_OK, INST_FATAL_INSUFFICIENT_TOKENS, INST_FATAL_UNKNOWN_DEST, INST_FIFO_OVERFLOW,
 INST_HANG, INST_DELAY_EXHAUSTED) = range(6)
COUNTER_NAMES = ("push", "peek", "pop_tok", "pop_mk", "recorded", "completed", "instances", "ticks")
SUM_NAMES = ("instances", "ok", "fatal", "other", "delivered", "snapshot_hash", "cut_residual",
             "final_residual", "completed", "in_flight")

# the C ABI's return codes (include/clsnap.h CL_E_*)
(E_INVALID, E_UNKNOWN_NODE, E_DUPLICATE_NODE, E_PARSE, E_IO, E_DEVICE, E_LIMIT, E_STATE,
 E_NOT_COMPLETE) = range(-1, -10, -1)
_ERRORS = {E_INVALID: "invalid", E_UNKNOWN_NODE: "unknown node", E_DUPLICATE_NODE: "duplicate node",
           E_PARSE: "parse", E_IO: "io", E_DEVICE: "device", E_LIMIT: "limit", E_STATE: "state",
           E_NOT_COMPLETE: "not complete"}


class ClSnapError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{_ERRORS.get(code, code)}] {msg}")
        self.code = code


_lib = None


def lib():
    """Load lib/libclsnap.so (build it with __graft_entry__.build() or `make`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ClSnapError(-6, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    vp, i64, i32, cp, pp = C.c_void_p, C.c_int64, C.c_int32, C.c_char_p, C.POINTER(C.c_void_p)
    sig = {
        "cl_sim_create": [i64, pp],
        "cl_sim_destroy": [vp],
        "cl_add_node": [vp, cp, i64],
        "cl_add_link": [vp, cp, cp],
        "cl_read_topology_file": [vp, cp],
        "cl_read_topology_text": [vp, cp],
        "cl_set_device": [vp, i32],
        "cl_set_limits": [vp, i32, i64],
        "cl_set_delay_go_seeds": [vp, i64],
        "cl_set_delay_schedule": [vp, vp, i64],
        "cl_send_tokens": [vp, cp, cp, i64],
        "cl_start_snapshot": [vp, cp, vp],
        "cl_tick": [vp, i32],
        "cl_drain": [vp],
        "cl_read_events_file": [vp, cp, vp],
        "cl_read_events_text": [vp, cp, vp],
        "cl_flush": [vp],
        "cl_rerun": [vp],
        "cl_synchronize": [vp],
        "cl_last_kernel_ms": [vp, vp],
        "cl_kernel_time": [vp, vp, vp],
        "cl_replay_spill_free": [vp, vp],
        "cl_replay_mapped": [vp, vp],
        "cl_records_blocked": [vp, vp],
        "cl_instance_hashes": [vp, i64, i64, vp],
        "cl_debug_poison_outputs": [vp],
        "cl_replay_split": [vp, vp, vp],
        "cl_replay_plan_of": [vp, vp, i64, i32, i32, vp, vp, vp, vp],
        "cl_num_nodes": [vp, vp],
        "cl_node_id": [vp, i32, vp],
        "cl_num_channels": [vp, vp],
        "cl_channel": [vp, i32, vp, vp],
        "cl_num_snapshots": [vp, vp],
        "cl_num_instances": [vp, vp],
        "cl_delay_draws_needed": [vp, vp],
        "cl_device_bytes": [vp, vp],
        "cl_get_status": [vp, vp],
        "cl_get_time": [vp, vp],
        "cl_node_tokens": [vp, i64, vp],
        "cl_snapshot_tick": [vp, i32, i64, vp],
        "cl_collect_snapshot": [vp, i32, i64, vp, vp, vp, i64],
        "cl_poll_snapshot": [vp, i32, i64, i64, vp],
        "cl_wait_snapshot": [vp, i32, i64, i64, i64, vp],
        "cl_collect_snapshot_range": [vp, i32, i64, i64, vp, vp, vp, vp, i64],
        "cl_collect_snapshot_packed": [vp, i32, i64, i64, vp, vp, vp, vp, i64, vp],
        "cl_collect_time": [vp, vp],
        "cl_get_counters": [vp, i32, vp],
        "cl_get_checksums": [vp, vp],
        "cl_go_delay_schedule": [i64, i64, i64, vp],
        "cl_go_int63": [i64, i64, vp],
        "cl_go_intn": [i64, i32, i64, vp],
        "cl_trace_enable": [vp, i64, i32, i32],
        "cl_trace_read": [vp, i64, vp, i32, vp],
        "cl_set_exec_engine": [vp, i32],
        "cl_exec_engine": [vp, vp],
        "cl_jit_stats": [vp, vp],
        "cl_lanes_compile_check": [vp, vp, vp, i64],
        "cl_set_program_kernels": [vp, i32],
        "cl_exec_program_kernels": [vp, vp],
        "cl_exec_program_cover": [vp, vp],
        "cl_lanes_program_compile_check": [vp, vp, vp, vp, i64],
        "cl_stats_layout_of": [vp, vp, vp],
        "cl_snapshot_stats": [vp, i32, i64, i64, vp, vp, i64],
        "cl_stats_time": [vp, vp],
        "cl_snapshot_census": [vp, i32, i64, i64, vp, vp, vp, vp],
        "cl_census_time": [vp, vp],
        "cl_collect_snapshot_list": [vp, i32, vp, i64, vp, vp, vp, vp, i64, vp],
        "cl_select_instances": [vp, i32, i64, i64, vp, i32, vp, vp, i64, vp],
        "cl_select_time": [vp, vp],
        "cl_select_stage_times": [vp, vp, vp],
        "cl_snapshot_ticks": [vp, i32, i64, i64, vp],
        "cl_iset_from_clauses": [vp, i32, i64, i64, vp, i32, pp, vp],
        "cl_iset_from_list": [vp, vp, i64, pp],
        "cl_iset_combine": [vp, vp, vp, i32],
        "cl_iset_count": [vp, i64, i64, vp],
        "cl_iset_read": [vp, i64, i64, vp, i64, vp],
        "cl_iset_destroy": [vp],
        "cl_iset_time": [vp, vp],
        "cl_snapshot_stats_in": [vp, i32, i64, i64, vp, vp, vp, i64],
        "cl_snapshot_census_in": [vp, i32, i64, i64, vp, vp, vp, vp, vp],
        "cl_select_instances_in": [vp, i32, i64, i64, vp, vp, i32, vp, vp, i64, vp],
        "cl_snapshot_crosstab": [vp, i64, i64, vp, vp, vp, i64],
        "cl_snapshot_crosstab_in": [vp, i64, i64, vp, vp, vp, vp, i64],
        "cl_crosstab_time": [vp, vp],
        "cl_snapshot_groups": [vp, i64, i64, vp, i32, vp, vp, vp, vp, vp],
        "cl_snapshot_groups_in": [vp, i64, i64, vp, vp, i32, vp, vp, vp, vp, vp],
        "cl_groups_time": [vp, vp],
        "cl_groups_stage_times": [vp, vp],
        "cl_snapshot_topk": [vp, i64, i64, vp, i32, i64, vp, vp, vp],
        "cl_snapshot_topk_in": [vp, i64, i64, vp, vp, i32, i64, vp, vp, vp],
        "cl_snapshot_quantiles": [vp, i64, i64, vp, vp, i32, vp, vp, vp],
        "cl_snapshot_quantiles_in": [vp, i64, i64, vp, vp, vp, i32, vp, vp, vp],
        "cl_snapshot_values": [vp, i64, i64, vp, vp, vp],
        "cl_snapshot_values_in": [vp, i64, i64, vp, vp, vp, vp],
        "cl_order_time": [vp, vp],
        "cl_order_stage_times": [vp, vp],
        "cl_order_plane_device": [i32, vp, vp, i64, i32, i64, vp, vp, vp, vp, i32, vp, vp, vp],
        "cl_set_delay_go_seed_list": [vp, vp, i64],
        "cl_set_delay_generator": [vp, i32],
        "cl_delay_generator": [vp, vp],
        "cl_delay_gen_time": [vp, vp, vp, vp],
        "cl_go_delay_schedule_jump": [i64, vp, i64, i64, vp, vp],
        "cl_go_delay_schedule_device": [i32, i64, vp, i64, i64, vp, vp, vp],
    }
    for name, args in sig.items():
        if os.environ.get("CLSNAP_VARIANT") and not hasattr(L, name):
            continue  # (an older diagnostic build: entry points added since are absent)
        f = getattr(L, name)
        f.restype, f.argtypes = C.c_int, args
    L.cl_status_string.restype, L.cl_status_string.argtypes = cp, [i32]
    L.cl_last_error.restype, L.cl_last_error.argtypes = cp, []
    if hasattr(L, "cl_group_key"):
        L.cl_group_key.restype, L.cl_group_key.argtypes = C.c_uint64, [vp, i32]
    _lib = L
    return L


# Logger record kinds (include/clsnap.h CL_LOG_*)
LOG_SENT_TOKEN, LOG_SENT_MARKER, LOG_RECV_TOKEN, LOG_RECV_MARKER, LOG_START, LOG_END = range(6)


def jit_stats():
    """Run-time kernel compilations of this process: (total ms, count)."""
    ms, n = C.c_double(), C.c_int64()
    _check(lib().cl_jit_stats(C.byref(ms), C.byref(n)))
    return ms.value, n.value


def format_log(ids, records):
    """Logger.PrettyPrint (logger.go:55-64) of (epoch, kind, node, other, data, tokens)
    records: LogEvent.String / the record String methods (logger.go:25-50,
    common.go:75-122)."""
    name = lambda r: ids[r] if r >= 0 else "?"  # noqa: E731  (no link: the dest string is not kept)
    lines, epoch = [], None
    for ep, kind, node, other, data, tokens in records:
        if ep != epoch:
            lines.append(f"Time {ep}:")
            epoch = ep
        if kind == LOG_SENT_TOKEN:
            rec, pre = f"{ids[node]} sent {data} tokens to {name(other)}", True
        elif kind == LOG_SENT_MARKER:
            rec, pre = f"{ids[node]} sent marker({data}) to {name(other)}", False
        elif kind == LOG_RECV_TOKEN:
            rec, pre = f"{ids[node]} received {data} tokens from {name(other)}", True
        elif kind == LOG_RECV_MARKER:
            rec, pre = f"{ids[node]} received marker({data}) from {name(other)}", False
        elif kind == LOG_START:
            rec, pre = f"{ids[node]} startSnapshot({data})", True
        else:
            rec, pre = f"{ids[node]} endSnapshot({data})", False
        lines.append(f"\t{ids[node]} has {tokens} token(s)\n\t{rec}" if pre else f"\t{rec}")
    return "\n".join(lines) + ("\n" if lines else "")


def _check(rc):
    if rc != 0:
        raise ClSnapError(rc, lib().cl_last_error().decode())
    return rc


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def go_delay_schedule(seed_base, n, draws):
    """uint8[n, draws]: rand.Intn(5) draws of rand.Seed(seed_base + i) (sim.go:101)."""
    out = np.empty((n, draws), dtype=np.uint8)
    _check(lib().cl_go_delay_schedule(seed_base, n, draws, _p(out)))
    return out


def replay_plan_of(final_ticks, spilled, insts_per_wave, can_split):
    """The replay planning policy on the host (cl_replay_plan_of; no device): (order int32[n],
    mapped, split_slot, n_spilled) for per-instance final ticks and spill flags (None: none)."""
    t = np.ascontiguousarray(final_ticks, dtype=np.int32)
    sp = None if spilled is None else np.ascontiguousarray(spilled, dtype=np.uint8)
    if sp is not None and sp.shape != t.shape:
        raise ClSnapError(E_INVALID, "one spill flag per final tick")
    order = np.empty(t.size, dtype=np.int32)
    mapped, split, n_sp = C.c_int32(), C.c_int64(), C.c_int64()
    _check(lib().cl_replay_plan_of(_p(t), None if sp is None else _p(sp), t.size, int(insts_per_wave),
                                   1 if can_split else 0, _p(order), C.byref(mapped), C.byref(split),
                                   C.byref(n_sp)))
    return order, bool(mapped.value), split.value, n_sp.value


def _seed_rows(seed_base, n, seeds):
    """(seed_base, seeds array or None, n) of the schedule utilities: ``seeds`` overrides both."""
    if seeds is None:
        if n is None:
            raise ClSnapError(E_INVALID, "give n (rows of seed_base + i) or seeds")
        return int(seed_base), None, int(n)
    s = np.ascontiguousarray(seeds, dtype=np.int64)
    if s.ndim != 1 or (n is not None and int(n) != s.size):
        raise ClSnapError(E_INVALID, "seeds must be int64[n]")
    return 0, s, int(s.size)


def go_delay_schedule_jump(seed_base=0, n=None, draws=0, seeds=None, return_info=False):
    """go_delay_schedule from the generator's closed form (csrc/cl_gorand.h), on the host: row i
    from ``seeds[i]``, or from ``seed_base + i``.  With return_info: (schedule, rows that met an
    Intn rejection and were regenerated sequentially)."""
    base, s, n = _seed_rows(seed_base, n, seeds)
    out = np.empty((n, draws), dtype=np.uint8)
    rej = C.c_int64(0)
    _check(lib().cl_go_delay_schedule_jump(base, None if s is None else _p(s), n, draws, _p(out), C.byref(rej)))
    return (out, rej.value) if return_info else out


def go_delay_schedule_device(seed_base=0, n=None, draws=0, seeds=None, device=0, return_info=False):
    """go_delay_schedule generated by the gfx950 kernel (cl_go_delay_schedule_device) and copied
    back.  With return_info: (schedule, rows patched on the host, kernel ms)."""
    base, s, n = _seed_rows(seed_base, n, seeds)
    out = np.empty((n, draws), dtype=np.uint8)
    patched, ms = C.c_int64(0), C.c_double(0)
    _check(lib().cl_go_delay_schedule_device(device, base, None if s is None else _p(s), n, draws, _p(out),
                                             C.byref(patched), C.byref(ms)))
    return (out, patched.value, ms.value) if return_info else out


def go_int63(seed, n):
    out = np.empty(n, dtype=np.int64)
    _check(lib().cl_go_int63(seed, n, _p(out)))
    return out


def go_intn(seed, bound, n):
    out = np.empty(n, dtype=np.int32)
    _check(lib().cl_go_intn(seed, bound, n, _p(out)))
    return out


class PassTokenEvent:  # common.go:61-65
    def __init__(self, src, dest, tokens):
        self.src, self.dest, self.tokens = src, dest, tokens


class SnapshotEvent:  # common.go:67-70
    def __init__(self, node_id):
        self.nodeId = node_id


class MsgSnapshot:  # common.go:20-24
    __slots__ = ("src", "dest", "tokens")

    def __init__(self, src, dest, tokens):
        self.src, self.dest, self.tokens = src, dest, tokens

    def __repr__(self):
        return f"{self.src} -> {self.dest}: token({self.tokens})"

    def astuple(self):
        return (self.src, self.dest, self.tokens)


class GlobalSnapshot:  # common.go:13-17
    def __init__(self, sid, token_map, messages):
        self.id, self.tokenMap, self.messages = sid, token_map, messages


# cl_stats_layout (include/clsnap.h), field by field: int64 word offsets into the flat result
STATS_LAYOUT_FIELDS = (
    "n_nodes", "n_channels", "tick_lo", "tick_bins", "msg_bins",
    "total_words", "sum_begin", "sum_end", "min_begin", "min_end", "max_begin", "max_end",
    "instances", "ok", "sample", "tick_sum", "tick_sumsq", "tick_hist", "msgs_sum", "msgs_sumsq",
    "inflight_sum", "inflight_sumsq", "node_sum", "node_sumsq", "ch_msgs_sum", "ch_msgs_sumsq",
    "ch_tok_sum", "ch_tok_sumsq", "ch_msg_hist",
    "min_tick", "min_msgs", "min_inflight", "min_node", "min_ch_msgs", "min_ch_tok",
    "max_tick", "max_msgs", "max_inflight", "max_node", "max_ch_msgs", "max_ch_tok")
STATS_INT64_MAX, STATS_INT64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


class SnapshotStats:
    """The result of ``ChandyLamportSim.snapshot_stats``: named numpy views over the flat int64
    array ``raw`` (cl_snapshot_stats, include/clsnap.h).

    ``layout`` maps the cl_stats_layout field names to word offsets.  Scalars (``instances``,
    ``ok``, ``sample``, ``tick_sum``, ``min_tick``, ...) read as ints; ``tick_hist[tick_bins]``,
    ``node_sum[N]``, ``ch_msgs_sum[C]``, ``ch_msg_hist[C, msg_bins]``, ``min_node[N]``, ... are
    views.  The sums of squares are modulo 2**64."""

    MOMENT_FIELDS = ("tick", "msgs", "inflight", "node", "ch_msgs", "ch_tok")

    def __init__(self, layout, raw):
        self.layout = dict(layout)
        self.raw = np.ascontiguousarray(raw, dtype=np.int64)
        L = self.layout
        if self.raw.shape != (L["total_words"],):
            raise ValueError(f"SnapshotStats: raw must hold {L['total_words']} int64 words")
        n, c, t, m = L["n_nodes"], L["n_channels"], L["tick_bins"], L["msg_bins"]
        shapes = {"tick_hist": (t,), "node_sum": (n,), "node_sumsq": (n,), "ch_msg_hist": (c, m)}
        for k in ("ch_msgs_sum", "ch_msgs_sumsq", "ch_tok_sum", "ch_tok_sumsq"):
            shapes[k] = (c,)
        for p in ("min_", "max_"):
            shapes[p + "node"] = (n,)
            shapes[p + "ch_msgs"] = shapes[p + "ch_tok"] = (c,)
        self._shapes = shapes

    def __getattr__(self, name):
        L = self.__dict__.get("layout")
        if L is None or name not in STATS_LAYOUT_FIELDS[12:]:
            raise AttributeError(name)
        shape = self._shapes.get(name)
        if shape is None:
            return int(self.raw[L[name]])
        size = int(np.prod(shape))
        return self.raw[L[name]:L[name] + size].reshape(shape)

    def _moments(self, field):
        if field not in self.MOMENT_FIELDS:
            raise ValueError(f"SnapshotStats: field must be one of {self.MOMENT_FIELDS}")
        s = np.atleast_1d(getattr(self, field + "_sum"))
        q = np.atleast_1d(getattr(self, field + "_sumsq"))
        return [int(x) for x in s.ravel()], [int(x) & (2**64 - 1) for x in q.ravel()], field in self.MOMENT_FIELDS[:3]

    def mean(self, field):
        """Mean over the sample of "tick", "msgs", "inflight" (floats) or "node", "ch_msgs",
        "ch_tok" (float arrays); nan on an empty sample."""
        s, _, scalar = self._moments(field)
        n = self.sample
        out = np.array([x / n if n else np.nan for x in s], dtype=np.float64)
        return float(out[0]) if scalar else out

    def variance(self, field):
        """Population variance over the sample, from the exact integer moments (valid while the
        true sum of squares is below 2**64); nan on an empty sample."""
        s, q, scalar = self._moments(field)
        n = self.sample
        out = np.array([(n * b - a * a) / (n * n) if n else np.nan for a, b in zip(s, q)], dtype=np.float64)
        return float(out[0]) if scalar else out

    def merge(self, other):
        """The statistics of the union of two disjoint samples (other ranks, other instance
        ranges): SUM, MIN and MAX over the three sections.  Raises ValueError when the layouts differ."""
        if not isinstance(other, SnapshotStats) or other.layout != self.layout:
            raise ValueError("SnapshotStats.merge: the layouts differ")
        L = self.layout
        raw = np.empty_like(self.raw)
        a, b = L["sum_begin"], L["sum_end"]
        raw[a:b] = (self.raw[a:b].view(np.uint64) + other.raw[a:b].view(np.uint64)).view(np.int64)  # wraps
        a, b = L["min_begin"], L["min_end"]
        raw[a:b] = np.minimum(self.raw[a:b], other.raw[a:b])
        a, b = L["max_begin"], L["max_end"]
        raw[a:b] = np.maximum(self.raw[a:b], other.raw[a:b])
        return SnapshotStats(L, raw)

    def __eq__(self, other):
        return (isinstance(other, SnapshotStats) and other.layout == self.layout
                and bool(np.array_equal(other.raw, self.raw)))

    __hash__ = None


# cl_census_class / cl_census_spec / cl_census_info (include/clsnap.h)
CENSUS_CLASS_DTYPE = np.dtype([("key", np.uint64), ("count", np.int64), ("first_inst", np.int64),
                               ("min_tick", np.int32), ("max_tick", np.int32)])


class _CensusSpec(C.Structure):
    _fields_ = [("max_classes", C.c_int64), ("lds_slots", C.c_int32)]


def _sort_classes(classes):
    """count descending, then key ascending (unsigned): the order cl_snapshot_census returns."""
    order = np.lexsort((classes["key"], -classes["count"]))
    return np.ascontiguousarray(classes[order])


class SnapshotCensus:
    """The result of ``ChandyLamportSim.snapshot_census``: the distinct global snapshots of a batch.

    ``classes`` is a structured array (CENSUS_CLASS_DTYPE: key, count, first_inst, min_tick,
    max_tick) of the returned classes, ordered by count descending, then key ascending;
    ``n_classes`` counts all distinct keys, also those beyond ``max_classes``.  ``class_of``
    (or None) maps each instance of the range to its class index, -1 outside the sample.  Classes
    are keyed by the 64-bit snapshot content hash."""

    def __init__(self, snapshot_id, instances, ok, sample, n_classes, classes, class_of=None):
        self.snapshot_id = int(snapshot_id)
        self.instances, self.ok, self.sample, self.n_classes = int(instances), int(ok), int(sample), int(n_classes)
        self.classes = np.ascontiguousarray(classes, dtype=CENSUS_CLASS_DTYPE)
        self.class_of = class_of

    @property
    def n_returned(self):
        return int(self.classes.shape[0])

    def frequency(self, k):
        """Share of the sample in returned class k; nan on an empty sample."""
        return float(self.classes["count"][k]) / self.sample if self.sample else float("nan")

    def merge(self, other, offset=0):
        """The census of the union of two disjoint instance sets (other ranks, other ranges);
        ``offset`` is added to ``other``'s instance indices.  Same key: counts add, first_inst and
        min_tick take the minimum, max_tick the maximum.  Re-sorted; class_of is dropped.  Raises
        ValueError when either side was truncated (n_returned < n_classes) or the snapshot ids differ."""
        if not isinstance(other, SnapshotCensus) or other.snapshot_id != self.snapshot_id:
            raise ValueError("SnapshotCensus.merge: not a census of the same snapshot id")
        if self.n_returned < self.n_classes or other.n_returned < other.n_classes:
            raise ValueError("SnapshotCensus.merge: a truncated census (n_returned < n_classes) cannot be merged")
        b = other.classes.copy()
        b["first_inst"] += offset
        both = np.concatenate([self.classes, b])
        keys, inv = np.unique(both["key"], return_inverse=True)
        out = np.zeros(keys.size, dtype=CENSUS_CLASS_DTYPE)
        out["key"] = keys
        out["first_inst"] = np.iinfo(np.int64).max
        out["min_tick"] = np.iinfo(np.int32).max
        out["max_tick"] = np.iinfo(np.int32).min
        np.add.at(out["count"], inv, both["count"])
        np.minimum.at(out["first_inst"], inv, both["first_inst"])
        np.minimum.at(out["min_tick"], inv, both["min_tick"])
        np.maximum.at(out["max_tick"], inv, both["max_tick"])
        return SnapshotCensus(self.snapshot_id, self.instances + other.instances, self.ok + other.ok,
                              self.sample + other.sample, keys.size, _sort_classes(out))

    def snapshots(self, sim):
        """One GlobalSnapshot per returned class: its representative's contents, all collected in
        one collect_snapshot_list call."""
        tok, _, off, msg = sim.collect_snapshot_list(self.snapshot_id, self.classes["first_inst"])
        ids, chans = sim.node_ids(), sim.channels()
        ch = len(chans)
        order = sorted(range(ch), key=lambda c: (chans[c][1], chans[c][0]))
        out = []
        for r in range(self.n_returned):
            msgs = [MsgSnapshot(ids[chans[c][0]], ids[chans[c][1]], int(msg[k]))
                    for c in order for k in range(off[r * ch + c], off[r * ch + c + 1])]
            out.append(GlobalSnapshot(self.snapshot_id, {ids[v]: int(tok[r, v]) for v in range(len(ids))}, msgs))
        return out

    def __eq__(self, other):
        return (isinstance(other, SnapshotCensus) and self.snapshot_id == other.snapshot_id
                and (self.instances, self.ok, self.sample, self.n_classes)
                == (other.instances, other.ok, other.sample, other.n_classes)
                and self.classes.tobytes() == other.classes.tobytes())

    __hash__ = None


# cl_select_clause (include/clsnap.h) and the CL_SEL_* field codes, by name
SELECT_CLAUSE_DTYPE = np.dtype([("field", np.int32), ("index", np.int32), ("flags", np.int32),
                                ("reserved", np.int32), ("lo", np.int64), ("hi", np.int64)])
SELECT_FIELDS = ("tick", "msgs", "inflight", "node", "ch_msgs", "ch_tok", "key")
SELECT_NOT = 1
SELECT_MAX_CLAUSES = 8


def _field_index(what, field, index, ids, chans):
    """The `index` of a select clause or crosstab axis as the C ABI takes it: a node id or rank
    ("node"), a channel number or (src, dest) pair of ids or ranks ("ch_msgs", "ch_tok"), None for
    the fields that take none; ids = node ids by rank, chans = (src rank, dest rank) per channel."""
    if field == "node":
        if isinstance(index, str):
            if index not in ids:
                raise ValueError(f"{what}: no node {index!r}")
            index = ids.index(index)
    elif field in ("ch_msgs", "ch_tok"):
        if isinstance(index, (tuple, list)):
            pair = tuple(ids.index(x) if isinstance(x, str) and x in ids else x for x in index)
            if pair not in chans:
                raise ValueError(f"{what}: no channel {tuple(index)!r}")
            index = chans.index(pair)
    elif index is None:
        index = 0
    if index is None or isinstance(index, (str, tuple, list)):
        raise ValueError(f"{what}: {field!r} does not take index {index!r}")
    return int(index)


def _select_clauses(where, ids, chans):
    """`where` of ChandyLamportSim.select_instances as a SELECT_CLAUSE_DTYPE array; ids = node ids
    by rank, chans = (src rank, dest rank) per channel."""
    where = list(where)
    out = np.zeros(len(where), dtype=SELECT_CLAUSE_DTYPE)
    i64 = np.iinfo(np.int64)
    for q, clause in enumerate(where):
        if len(clause) not in (4, 5) or (len(clause) == 5 and clause[4] != "not"):
            raise ValueError(f"select clause {q}: (field, index, lo, hi) or (field, index, lo, hi, 'not')")
        field, index, lo, hi = clause[:4]
        if field not in SELECT_FIELDS:
            raise ValueError(f"select clause {q}: field must be one of {SELECT_FIELDS}")
        index = _field_index(f"select clause {q}", field, index, ids, chans)
        if field == "key":
            lo, hi = 0 if lo is None else int(lo), 2**64 - 1 if hi is None else int(hi)
            if not (0 <= lo < 2**64 and 0 <= hi < 2**64):
                raise ValueError(f"select clause {q}: key bounds are uint64 values")
            lo, hi = (int(np.array(v, dtype=np.uint64).view(np.int64)) for v in (lo, hi))
        else:
            lo, hi = i64.min if lo is None else int(lo), i64.max if hi is None else int(hi)
        out[q] = (SELECT_FIELDS.index(field), int(index), SELECT_NOT if len(clause) == 5 else 0, 0, lo, hi)
    return out


# cl_group_term (include/clsnap.h): a term of snapshot_groups
GROUP_TERM_DTYPE = np.dtype([("sid", np.int32), ("field", np.int32), ("index", np.int32), ("reserved", np.int32)])
GROUPS_MAX_TERMS = 8


def _group_terms(terms, ids, chans):
    """`terms` of ChandyLamportSim.snapshot_groups, each (sid, field, index) or (sid, field), as a
    GROUP_TERM_DTYPE array; ValueError for anything the C call would have to refuse by shape."""
    if isinstance(terms, np.ndarray) and terms.dtype == GROUP_TERM_DTYPE:
        terms = [(int(t["sid"]), SELECT_FIELDS[int(t["field"])], int(t["index"])) for t in terms.ravel()]
    if isinstance(terms, (str, bytes)) or not hasattr(terms, "__iter__"):
        raise ValueError("group terms: a sequence of (sid, field, index)")
    terms = list(terms)
    if not 1 <= len(terms) <= GROUPS_MAX_TERMS:
        raise ValueError(f"group terms: 1 to {GROUPS_MAX_TERMS} terms")
    out = np.zeros(len(terms), dtype=GROUP_TERM_DTYPE)
    for k, term in enumerate(terms):
        what = f"group term {k}"
        if not isinstance(term, (tuple, list)) or len(term) not in (2, 3):
            raise ValueError(f"{what}: (sid, field, index)")
        sid, field = term[:2]
        if isinstance(sid, bool) or not isinstance(sid, (int, np.integer)) or not 0 <= sid <= np.iinfo(np.int32).max:
            raise ValueError(f"{what}: sid must be an integer >= 0")
        if not isinstance(field, str) or field not in SELECT_FIELDS:
            raise ValueError(f"{what}: field must be one of {SELECT_FIELDS}")
        index = _field_index(what, field, term[2] if len(term) == 3 else None, ids, chans)
        if not 0 <= index <= np.iinfo(np.int32).max:
            raise ValueError(f"{what}: index {index} out of range")
        out[k] = (sid, SELECT_FIELDS.index(field), index, 0)
    return out


def group_key(values):
    """The 64-bit key of a tuple of int64 term values (cl_group_key): what SnapshotGroups.groups["key"]
    holds for the group with these values.  Host only."""
    v = np.ascontiguousarray(values, dtype=np.int64).ravel()
    return int(lib().cl_group_key(_p(v) if v.size else None, v.size))


class SnapshotGroups:
    """The result of ``ChandyLamportSim.snapshot_groups``: GROUP BY over a tuple of snapshot quantities.

    ``terms`` is the GROUP_TERM_DTYPE array of the call.  ``groups`` is a structured array
    (CENSUS_CLASS_DTYPE: key, count, first_inst, and the min / max completion tick of terms[0]'s
    snapshot) of the returned groups, ordered by count descending, then key ascending;
    ``values[g]`` is group g's tuple (int64; a "key" term's value is the uint64 hash's bit pattern).
    ``n_groups`` counts all groups, also those beyond ``max_groups``.  ``group_of`` (or None) maps
    each instance of the range to its group index, -1 outside the sample.  Groups are keyed by the
    64-bit ``group_key`` of the tuple: equal keys mean the same group."""

    def __init__(self, terms, instances, ok, sample, n_groups, groups, values, group_of=None):
        self.terms = np.ascontiguousarray(terms, dtype=GROUP_TERM_DTYPE).ravel()
        self.instances, self.ok, self.sample, self.n_groups = int(instances), int(ok), int(sample), int(n_groups)
        self.groups = np.ascontiguousarray(groups, dtype=CENSUS_CLASS_DTYPE)
        self.values = np.ascontiguousarray(values, dtype=np.int64).reshape(self.groups.shape[0], self.terms.size)
        self.group_of = group_of

    @property
    def n_returned(self):
        return int(self.groups.shape[0])

    def frequency(self, g):
        """Share of the sample in returned group g; nan on an empty sample."""
        return float(self.groups["count"][g]) / self.sample if self.sample else float("nan")

    def merge(self, other, offset=0):
        """The groups of the union of two disjoint instance sets (other ranks, other ranges);
        ``offset`` is added to ``other``'s instance indices.  Same key: counts add, first_inst and
        min_tick take the minimum, max_tick the maximum, the values ride along.  Re-sorted; group_of
        is dropped.  Raises ValueError when either side was truncated (n_returned < n_groups) or
        the terms differ."""
        if not isinstance(other, SnapshotGroups) or other.terms.tobytes() != self.terms.tobytes():
            raise ValueError("SnapshotGroups.merge: not the groups of the same terms")
        if self.n_returned < self.n_groups or other.n_returned < other.n_groups:
            raise ValueError("SnapshotGroups.merge: truncated groups (n_returned < n_groups) cannot be merged")
        b = other.groups.copy()
        b["first_inst"] += offset
        both = np.concatenate([self.groups, b])
        vals = np.concatenate([self.values, other.values])
        keys, at, inv = np.unique(both["key"], return_index=True, return_inverse=True)
        out = np.zeros(keys.size, dtype=CENSUS_CLASS_DTYPE)
        out["key"] = keys
        out["first_inst"] = np.iinfo(np.int64).max
        out["min_tick"] = np.iinfo(np.int32).max
        out["max_tick"] = np.iinfo(np.int32).min
        np.add.at(out["count"], inv, both["count"])
        np.minimum.at(out["first_inst"], inv, both["first_inst"])
        np.minimum.at(out["min_tick"], inv, both["min_tick"])
        np.maximum.at(out["max_tick"], inv, both["max_tick"])
        order = np.lexsort((out["key"], -out["count"]))
        return SnapshotGroups(self.terms.copy(), self.instances + other.instances, self.ok + other.ok,
                              self.sample + other.sample, keys.size, out[order], vals[at][order])

    def instance_set(self, sim, g, inst_lo=0, inst_hi=None):
        """The InstanceSet of the instances of [inst_lo, inst_hi) whose tuple is that of returned
        group g: one sim.instance_set(sid, equality clauses) per distinct snapshot id of the terms,
        intersected.  For groups taken over the same range (and no set) its size is the group's count."""
        by_sid = {}
        for term, v in zip(self.terms, self.values[g]):
            field, v = SELECT_FIELDS[int(term["field"])], int(v)
            if field == "key":
                v &= 2**64 - 1
            by_sid.setdefault(int(term["sid"]), []).append((field, int(term["index"]), v, v))
        out = None
        for sid, where in by_sid.items():
            s = sim.instance_set(sid, where, inst_lo, inst_hi)
            out = s if out is None else out & s
        return out

    def __eq__(self, other):
        return (isinstance(other, SnapshotGroups) and self.terms.tobytes() == other.terms.tobytes()
                and (self.instances, self.ok, self.sample, self.n_groups)
                == (other.instances, other.ok, other.sample, other.n_groups)
                and self.groups.tobytes() == other.groups.tobytes()
                and self.values.tobytes() == other.values.tobytes())

    __hash__ = None


# cl_quantile (include/clsnap.h) and the limits of the ordering calls
QUANTILE_DTYPE = np.dtype([("num", np.int64), ("den", np.int64)])
ORDER_DESC = 1
ORDER_MAX_K = 65536
ORDER_MAX_QUANTILES = 64


def _order_term(term, ids, chans):
    """The one term of an ordering call, (sid, field, index) or (sid, field), as a GROUP_TERM_DTYPE
    array of one entry: resolved exactly as a term of snapshot_groups."""
    if isinstance(term, np.ndarray) and term.dtype == GROUP_TERM_DTYPE and term.size == 1:
        return _group_terms(term, ids, chans)
    if not isinstance(term, (tuple, list)):
        raise ValueError("order term: (sid, field, index)")
    return _group_terms([tuple(term)], ids, chans)


def _quantiles(qs):
    """`qs` of snapshot_quantiles as a QUANTILE_DTYPE array: each a (num, den) pair, a Fraction, the
    int 0 or 1, or a float taken through Fraction(q).limit_denominator(10**9)."""
    if isinstance(qs, np.ndarray) and qs.dtype == QUANTILE_DTYPE:
        qs = [(int(q["num"]), int(q["den"])) for q in qs.ravel()]
    if isinstance(qs, (str, bytes)) or not hasattr(qs, "__iter__"):
        raise ValueError("quantiles: a sequence of (num, den), Fraction, 0, 1 or float")
    qs = list(qs)
    if not 1 <= len(qs) <= ORDER_MAX_QUANTILES:
        raise ValueError(f"quantiles: 1 to {ORDER_MAX_QUANTILES} quantiles")
    out = np.zeros(len(qs), dtype=QUANTILE_DTYPE)
    for j, q in enumerate(qs):
        if isinstance(q, (tuple, list)) and len(q) == 2 and all(
                isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in q):
            num, den = int(q[0]), int(q[1])
        elif isinstance(q, Fraction):
            num, den = q.numerator, q.denominator
        elif isinstance(q, (int, np.integer)) and not isinstance(q, bool) and q in (0, 1):
            num, den = int(q), 1
        elif isinstance(q, (float, np.floating)) and 0.0 <= q <= 1.0:
            f = Fraction(float(q)).limit_denominator(10**9)
            num, den = f.numerator, f.denominator
        else:
            raise ValueError(f"quantile {j}: {q!r} is not a (num, den) pair, a Fraction, 0, 1 or a float in [0, 1]")
        if not (1 <= den < 2**63 and 0 <= num <= den):
            raise ValueError(f"quantile {j}: den >= 1 and 0 <= num <= den")
        out[j] = (num, den)
    return out


def quantile_rank(q, sample):
    """The nearest-rank position of quantile `q` (any form snapshot_quantiles takes) in a sample of
    `sample` values, as cl_snapshot_quantiles computes it: 0 if num == 0 else
    ceil(num * sample / den) - 1; -1 on an empty sample.  Host only."""
    num, den = (int(x) for x in _quantiles([q])[0].tolist())
    if sample <= 0:
        return -1
    return 0 if num == 0 else -((-num * int(sample)) // den) - 1


def _order_keys(values, descending):
    """The uint64 keys whose ascending order is the order of an ordering call: the value with its
    sign bit flipped, complemented for descending (csrc/cl_analytics.h order_key)."""
    k = np.ascontiguousarray(values, dtype=np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    return ~k if descending else k


class SnapshotTopK:
    """The result of ``ChandyLamportSim.snapshot_topk``: ORDER BY a snapshot quantity LIMIT k.

    ``term`` is the GROUP_TERM_DTYPE array (one entry) of the call, ``descending`` its direction,
    ``k`` what was asked for.  ``insts`` (int64, absolute) are the first ``n_returned = min(k,
    sample)`` instances of the order -- ascending by (value, instance), or value descending with
    the instance still ascending -- and ``values`` their values.  ``instances``, ``ok`` and
    ``sample`` are those of snapshot_stats over the same range."""

    def __init__(self, term, descending, k, instances, ok, sample, insts, values):
        self.term = np.ascontiguousarray(term, dtype=GROUP_TERM_DTYPE).ravel()
        self.descending, self.k = bool(descending), int(k)
        self.instances, self.ok, self.sample = int(instances), int(ok), int(sample)
        self.insts = np.ascontiguousarray(insts, dtype=np.int64).ravel()
        self.values = np.ascontiguousarray(values, dtype=np.int64).ravel()
        if self.term.size != 1 or self.insts.shape != self.values.shape:
            raise ValueError("SnapshotTopK: one term, and one value per instance")

    @property
    def n_returned(self):
        return int(self.insts.shape[0])

    @property
    def snapshot_id(self):
        return int(self.term["sid"][0])

    def collect(self, sim):
        """The contents of the listed instances: sim.collect_snapshot_list(sid, insts)."""
        return sim.collect_snapshot_list(self.snapshot_id, self.insts)

    def instance_set(self, sim):
        """The listed instances as an InstanceSet of `sim`."""
        return sim.instance_set_from(self.insts)

    def seeds(self, seed_base):
        """seed_base + insts: what set_delay_go_seed_list takes to re-run exactly these instances."""
        return np.int64(seed_base) + self.insts

    def merge(self, other, offset=0):
        """The top-k over the union of two disjoint instance sets (other ranks, other ranges);
        ``offset`` is added to ``other``'s instance indices.  Exact: the top-k of a union lies within
        the union of the parts' top-k.  Raises ValueError unless both are of the same term,
        direction and k."""
        if (not isinstance(other, SnapshotTopK) or other.term.tobytes() != self.term.tobytes()
                or other.descending != self.descending or other.k != self.k):
            raise ValueError("SnapshotTopK.merge: not the top-k of the same term, direction and k")
        insts = np.concatenate([self.insts, other.insts + offset])
        values = np.concatenate([self.values, other.values])
        order = np.lexsort((insts, _order_keys(values, self.descending)))[:self.k]
        return SnapshotTopK(self.term.copy(), self.descending, self.k, self.instances + other.instances,
                            self.ok + other.ok, self.sample + other.sample, insts[order], values[order])

    def __eq__(self, other):
        return (isinstance(other, SnapshotTopK) and self.term.tobytes() == other.term.tobytes()
                and (self.descending, self.k, self.instances, self.ok, self.sample)
                == (other.descending, other.k, other.instances, other.ok, other.sample)
                and bool(np.array_equal(self.insts, other.insts)) and bool(np.array_equal(self.values, other.values)))

    __hash__ = None


class SnapshotQuantiles:
    """The result of ``ChandyLamportSim.snapshot_quantiles``: exact quantiles of a snapshot quantity.

    ``q`` is the QUANTILE_DTYPE array of the call; ``ranks[j]`` the nearest-rank position of q[j]
    in the ascending order of the sample, ``0 if num == 0 else ceil(num * sample / den) - 1`` (-1
    on an empty sample), and ``values[j]`` the value there.  ``at(q)`` looks one up."""

    def __init__(self, term, q, ranks, values, sample, instances=0, ok=0):
        self.term = np.ascontiguousarray(term, dtype=GROUP_TERM_DTYPE).ravel()
        self.q = np.ascontiguousarray(q, dtype=QUANTILE_DTYPE).ravel()
        self.ranks = np.ascontiguousarray(ranks, dtype=np.int64).ravel()
        self.values = np.ascontiguousarray(values, dtype=np.int64).ravel()
        self.sample, self.instances, self.ok = int(sample), int(instances), int(ok)
        if not self.q.shape == self.ranks.shape == self.values.shape:
            raise ValueError("SnapshotQuantiles: one rank and one value per quantile")

    def at(self, q):
        """The value of quantile `q` (any form snapshot_quantiles takes), which the call asked for."""
        if self.sample == 0:
            raise ValueError("SnapshotQuantiles.at: the sample is empty")
        want = Fraction(*(int(x) for x in _quantiles([q])[0].tolist()))
        for j, (num, den) in enumerate(self.q.tolist()):
            if Fraction(num, den) == want:
                return int(self.values[j])
        raise KeyError(q)

    def __eq__(self, other):
        return (isinstance(other, SnapshotQuantiles) and self.term.tobytes() == other.term.tobytes()
                and self.q.tobytes() == other.q.tobytes() and (self.sample, self.instances, self.ok)
                == (other.sample, other.instances, other.ok) and bool(np.array_equal(self.ranks, other.ranks))
                and (self.sample == 0 or bool(np.array_equal(self.values, other.values))))

    __hash__ = None


def order_plane_device(values, in_sample=None, k=0, largest=False, qs=None, device=0, return_ms=False):
    """Engine-internal test aid (cl_order_plane_device): the select and compaction kernels of the
    ordering calls on an uploaded int64 plane, element index = instance.  Returns (insts, vals,
    q_values, q_ranks) -- the last two None without `qs` -- and the kernels' ms with return_ms."""
    v = np.ascontiguousarray(values, dtype=np.int64).ravel()
    m = None if in_sample is None else np.ascontiguousarray(in_sample, dtype=np.uint8).ravel()
    if m is not None and m.shape != v.shape:
        raise ValueError("order_plane_device: one in_sample flag per value")
    q = None if qs is None else _quantiles(qs)
    insts, vals = np.zeros(max(k, 0), dtype=np.int64), np.zeros(max(k, 0), dtype=np.int64)
    n_q = 0 if q is None else q.size
    qv, qr = np.zeros(n_q, dtype=np.int64), np.zeros(n_q, dtype=np.int64)
    n_ret, ms = C.c_int64(0), C.c_double(0)
    _check(lib().cl_order_plane_device(device, _p(v) if v.size else None, None if m is None else _p(m), v.size,
                                       ORDER_DESC if largest else 0, k, _p(insts) if k > 0 else None,
                                       _p(vals) if k > 0 else None, C.byref(n_ret), None if q is None else _p(q), n_q,
                                       _p(qv) if n_q else None, _p(qr) if n_q else None, C.byref(ms)))
    out = (insts[:n_ret.value].copy(), vals[:n_ret.value].copy(), qv if n_q else None, qr if n_q else None)
    return out + (ms.value,) if return_ms else out


class SnapshotSelection:
    """The result of ``ChandyLamportSim.select_instances``: the instances of the sample that
    satisfy every clause.

    ``instances``, ``ok`` and ``sample`` are those of snapshot_stats over the same range;
    ``n_match`` counts all matches, ``insts`` (int64, ascending) holds the first ``n_returned`` of
    them, ``ticks`` (int32, or None) their completion ticks; ``truncated`` says whether matches
    were left out."""

    def __init__(self, snapshot_id, instances, ok, sample, n_match, insts, ticks=None):
        self.snapshot_id = int(snapshot_id)
        self.instances, self.ok, self.sample, self.n_match = int(instances), int(ok), int(sample), int(n_match)
        self.insts = np.ascontiguousarray(insts, dtype=np.int64).ravel()
        self.ticks = None if ticks is None else np.ascontiguousarray(ticks, dtype=np.int32).ravel()
        if self.ticks is not None and self.ticks.shape != self.insts.shape:
            raise ValueError("SnapshotSelection: one tick per instance")

    @property
    def n_returned(self):
        return int(self.insts.shape[0])

    @property
    def truncated(self):
        return self.n_returned < self.n_match

    def collect(self, sim):
        """The contents of the selected instances: sim.collect_snapshot_list(snapshot_id, insts)."""
        return sim.collect_snapshot_list(self.snapshot_id, self.insts)

    def merge(self, other, offset=0):
        """The selection over the union of two disjoint instance sets (other ranks, other ranges);
        ``offset`` is added to ``other``'s instance indices.  The indices are concatenated and
        sorted, the counts add; ticks are kept when both sides have them.  Raises ValueError when
        either side is truncated or the snapshot ids differ."""
        if not isinstance(other, SnapshotSelection) or other.snapshot_id != self.snapshot_id:
            raise ValueError("SnapshotSelection.merge: not a selection of the same snapshot id")
        if self.truncated or other.truncated:
            raise ValueError("SnapshotSelection.merge: a truncated selection (n_returned < n_match) cannot be merged")
        insts = np.concatenate([self.insts, other.insts + offset])
        order = np.argsort(insts, kind="stable")
        ticks = None
        if self.ticks is not None and other.ticks is not None:
            ticks = np.concatenate([self.ticks, other.ticks])[order]
        return SnapshotSelection(self.snapshot_id, self.instances + other.instances, self.ok + other.ok,
                                 self.sample + other.sample, self.n_match + other.n_match, insts[order], ticks)

    def __eq__(self, other):
        return (isinstance(other, SnapshotSelection) and self.snapshot_id == other.snapshot_id
                and (self.instances, self.ok, self.sample, self.n_match)
                == (other.instances, other.ok, other.sample, other.n_match)
                and bool(np.array_equal(self.insts, other.insts))
                and (self.ticks is None) == (other.ticks is None)
                and (self.ticks is None or bool(np.array_equal(self.ticks, other.ticks))))

    __hash__ = None


ISET_AND, ISET_OR, ISET_ANDNOT = range(3)   # include/clsnap.h CL_ISET_*


# cl_crosstab_axis (include/clsnap.h) and the words of the flat result (CL_XT_*)
CROSSTAB_AXIS_DTYPE = np.dtype([("sid", np.int32), ("field", np.int32), ("index", np.int32), ("bins", np.int32),
                                ("lo", np.int64), ("width", np.int64)])
CROSSTAB_FIELDS = SELECT_FIELDS[:6]     # every select field but "key": a hash is not binnable
CROSSTAB_MAX_BINS = CROSSTAB_MAX_CELLS = 4096
(XT_INSTANCES, XT_OK, XT_SAMPLE, XT_SUM_A, XT_SUM_B, XT_SUM_AA, XT_SUM_AB, XT_SUM_BB, XT_MIN_A, XT_MIN_B, XT_MAX_A,
 XT_MAX_B, XT_CELLS) = range(13)


def _crosstab_axis(name, axis, ids, chans):
    """An axis of ChandyLamportSim.snapshot_crosstab, (sid, field, index, lo, width, bins), as a
    CROSSTAB_AXIS_DTYPE record; ValueError for anything the C call would have to refuse by shape."""
    what = f"crosstab axis {name}"
    if not isinstance(axis, (tuple, list)) or len(axis) != 6:
        raise ValueError(f"{what}: (sid, field, index, lo, width, bins)")
    sid, field, index, lo, width, bins = axis
    if field not in CROSSTAB_FIELDS:
        raise ValueError(f"{what}: field must be one of {CROSSTAB_FIELDS}")
    index = _field_index(what, field, index, ids, chans)
    i64 = np.iinfo(np.int64)
    for k, v in (("sid", sid), ("lo", lo), ("width", width), ("bins", bins)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: {k} must be an integer")
    if not (0 <= sid <= np.iinfo(np.int32).max and i64.min <= lo <= i64.max and 1 <= width <= i64.max
            and 1 <= bins <= CROSSTAB_MAX_BINS):
        raise ValueError(f"{what}: sid >= 0, int64 lo, width >= 1, 1 <= bins <= {CROSSTAB_MAX_BINS}")
    out = np.zeros(1, dtype=CROSSTAB_AXIS_DTYPE)
    out[0] = (sid, CROSSTAB_FIELDS.index(field), index, bins, lo, width)
    return out


class SnapshotCrosstab:
    """The result of ``ChandyLamportSim.snapshot_crosstab``: the joint distribution of two snapshot
    quantities over the OK instances in which the snapshots of both axes completed.

    ``axes`` is the pair of CROSSTAB_AXIS_DTYPE records, ``raw`` the flat int64 array of
    cl_snapshot_crosstab (include/clsnap.h CL_XT_*).  ``instances``, ``ok`` count the range,
    ``sample`` the joint sample; ``table`` is the int64 [bins_a, bins_b] view of the cells; ``min``
    and ``max`` are the (a, b) pairs (INT64_MAX / INT64_MIN on an empty sample).  The sums of
    products are modulo 2**64."""

    def __init__(self, axes, raw):
        a, b = (np.array(x, dtype=CROSSTAB_AXIS_DTYPE).reshape(1) for x in axes)
        self.axes = (a, b)
        self.raw = np.ascontiguousarray(raw, dtype=np.int64)
        if self.raw.shape != (XT_CELLS + self.shape[0] * self.shape[1],):
            raise ValueError(f"SnapshotCrosstab: raw must hold {XT_CELLS} + bins_a * bins_b int64 words")

    @property
    def shape(self):
        return int(self.axes[0]["bins"][0]), int(self.axes[1]["bins"][0])

    instances = property(lambda self: int(self.raw[XT_INSTANCES]))
    ok = property(lambda self: int(self.raw[XT_OK]))
    sample = property(lambda self: int(self.raw[XT_SAMPLE]))
    min = property(lambda self: (int(self.raw[XT_MIN_A]), int(self.raw[XT_MIN_B])))
    max = property(lambda self: (int(self.raw[XT_MAX_A]), int(self.raw[XT_MAX_B])))

    @property
    def table(self):
        return self.raw[XT_CELLS:].reshape(self.shape)

    def marginal(self, axis):
        """The histogram of one axis (0: a, 1: b) over the joint sample."""
        return self.table.sum(axis=1 - self._axis(axis))

    @staticmethod
    def _axis(axis):
        if axis not in (0, 1):
            raise ValueError("SnapshotCrosstab: axis must be 0 or 1")
        return axis

    def _sum(self, word):
        return int(self.raw[word])

    def _sumsq(self, word):
        return int(self.raw[word]) & (2**64 - 1)

    def mean(self, axis):
        """Mean of axis 0 (a) or 1 (b) over the sample; nan on an empty sample."""
        n = self.sample
        return self._sum(XT_SUM_A + self._axis(axis)) / n if n else float("nan")

    def variance(self, axis):
        """Population variance of an axis from the exact integer moments (valid while the true sum
        of squares is below 2**64, as SnapshotStats.variance); nan on an empty sample."""
        n, k = self.sample, self._axis(axis)
        s, q = self._sum(XT_SUM_A + k), self._sumsq(XT_SUM_BB if k else XT_SUM_AA)
        return (n * q - s * s) / (n * n) if n else float("nan")

    def covariance(self):
        """Population covariance of the two axes (valid while the true sum of products lies in
        [-2**63, 2**63): the wrapped word is read as int64); nan on an empty sample."""
        n = self.sample
        return (n * self._sum(XT_SUM_AB) - self._sum(XT_SUM_A) * self._sum(XT_SUM_B)) / (n * n) if n else float("nan")

    def correlation(self):
        """Pearson correlation of the two axes; nan on an empty sample or a constant axis."""
        va, vb = self.variance(0), self.variance(1)
        if not (va > 0 and vb > 0):
            return float("nan")
        return self.covariance() / float(np.sqrt(va) * np.sqrt(vb))

    def merge(self, other):
        """The crosstab of the union of two disjoint samples (other ranks, other instance ranges):
        a wrapping SUM over the counters, sums and cells, MIN and MAX over the extrema.  Raises
        ValueError when the axes differ."""
        if not isinstance(other, SnapshotCrosstab) or any(x.tobytes() != y.tobytes()
                                                          for x, y in zip(self.axes, other.axes)):
            raise ValueError("SnapshotCrosstab.merge: the axes differ")
        raw = (self.raw.view(np.uint64) + other.raw.view(np.uint64)).view(np.int64)  # wraps
        raw[XT_MIN_A:XT_MAX_A] = np.minimum(self.raw[XT_MIN_A:XT_MAX_A], other.raw[XT_MIN_A:XT_MAX_A])
        raw[XT_MAX_A:XT_CELLS] = np.maximum(self.raw[XT_MAX_A:XT_CELLS], other.raw[XT_MAX_A:XT_CELLS])
        return SnapshotCrosstab(self.axes, raw)

    def __eq__(self, other):
        return (isinstance(other, SnapshotCrosstab)
                and all(x.tobytes() == y.tobytes() for x, y in zip(self.axes, other.axes))
                and bool(np.array_equal(other.raw, self.raw)))

    __hash__ = None


class InstanceSet:
    """A set of instances of one ``ChandyLamportSim``, kept on the GPU as a bitmap (cl_iset).

    Made by ``sim.instance_set(snapshot_id, where)`` (the matches of select clauses; ``info`` is
    then the (instances, ok, sample, n_match) of that selection) or ``sim.instance_set_from(insts)``
    (``info`` is None).  ``a & b``, ``a | b`` and ``a - b`` give new sets; ``len(s)``, ``s.count(lo,
    hi)`` and ``s.insts(lo, hi, max_out)`` read one.  A set is only a set of indices: it stays valid
    across ``rerun()`` and engine switches, and a set made from one snapshot id may condition the
    analysis of another (``sim.snapshot_stats_in``, ``snapshot_census_in``, ``select_instances_in``).
    ``close()`` (or leaving a ``with`` block) frees the bitmap; the sim frees what is left."""

    def __init__(self, sim, handle, info=None):
        self._sim, self._h, self.info = sim, handle, info

    def _handle(self):
        if not self._h or not self._sim._h:
            raise ValueError("InstanceSet: the set is closed")
        return self._h

    def close(self):
        h, self._h = self._h, None
        if h and self._sim._h:   # (a destroyed sim has freed its sets)
            self._sim._L.cl_iset_destroy(h)

    def __del__(self):
        if getattr(self, "_h", None):
            self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _combine(self, other, op):
        if not isinstance(other, InstanceSet):
            return NotImplemented
        out = self._sim.instance_set_from(())
        _check(self._sim._L.cl_iset_combine(out._handle(), self._handle(), other._handle(), op))
        return out

    def __and__(self, other):
        return self._combine(other, ISET_AND)

    def __or__(self, other):
        return self._combine(other, ISET_OR)

    def __sub__(self, other):
        return self._combine(other, ISET_ANDNOT)

    def combine_into(self, a, b, op):
        """self = a op b in place (op one of ISET_AND, ISET_OR, ISET_ANDNOT); self may be a or b."""
        _check(self._sim._L.cl_iset_combine(self._handle(), a._handle(), b._handle(), op))
        self.info = None
        return self

    def count(self, lo=0, hi=None):
        """Members in [lo, hi)."""
        n = C.c_int64(0)
        _check(self._sim._L.cl_iset_count(self._handle(), lo, self._sim.n_instances if hi is None else hi, C.byref(n)))
        return n.value

    def __len__(self):
        return self.count()

    def insts(self, lo=0, hi=None, max_out=None):
        """The members in [lo, hi) as ascending int64 indices; at most max_out of them (the
        smallest) when given."""
        hi = self._sim.n_instances if hi is None else hi
        cap = self.count(lo, hi) if max_out is None else max_out
        out = np.zeros(max(cap, 0), dtype=np.int64)
        n = C.c_int64(0)
        _check(self._sim._L.cl_iset_read(self._handle(), lo, hi, _p(out) if cap > 0 else None, cap, C.byref(n)))
        return out[:min(n.value, max(cap, 0))].copy()


class ChandyLamportSim:
    """A batch of ``n_instances`` reference simulators (sim.go ChandyLamportSim).

    Events (``AddNode``, ``AddLink``, ``ProcessEvent``, ``Tick``, ``StartSnapshot``) are
    broadcast to every instance; results are read per instance.
    """

    def __init__(self, n_instances=1, device=0, seed_base=REFERENCE_SEED, fifo_lds_slots=None,
                 max_drain_ticks=None):
        self._L = lib()
        h = C.c_void_p()
        _check(self._L.cl_sim_create(n_instances, C.byref(h)))
        self._h = h
        self.n_instances = n_instances
        _check(self._L.cl_set_device(self._h, device))
        _check(self._L.cl_set_delay_go_seeds(self._h, seed_base))
        if fifo_lds_slots is not None or max_drain_ticks is not None:
            _check(self._L.cl_set_limits(self._h, fifo_lds_slots or 0,
                                         10000 if max_drain_ticks is None else max_drain_ticks))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.cl_sim_destroy(h)
            self._h = None

    # ---- reference API (sim.go) ---------------------------------------------
    def AddNode(self, node_id, tokens):           # sim.go:40
        _check(self._L.cl_add_node(self._h, node_id.encode(), tokens))

    def AddLink(self, src, dest):                 # sim.go:46
        _check(self._L.cl_add_link(self._h, src.encode(), dest.encode()))

    def ProcessEvent(self, event):                # sim.go:58
        if isinstance(event, PassTokenEvent):
            _check(self._L.cl_send_tokens(self._h, event.src.encode(), event.dest.encode(), event.tokens))
        elif isinstance(event, SnapshotEvent):
            self.StartSnapshot(event.nodeId)
        else:
            raise ClSnapError(-1, f"Error unknown event: {event!r}")

    def Tick(self, n=1):                          # sim.go:71
        _check(self._L.cl_tick(self._h, n))

    def StartSnapshot(self, node_id):             # sim.go:105
        sid = C.c_int32(-1)
        _check(self._L.cl_start_snapshot(self._h, node_id.encode(), C.byref(sid)))
        return sid.value

    def CollectSnapshot(self, snapshot_id, instance=0, timeout_ms=0):   # sim.go:134
        """GlobalSnapshot of one instance, messages in (dest, src, delivery) order.

        The reference blocks until the snapshot completes (sim.go:137-140): pass
        timeout_ms=-1 for that (from a collector thread while another thread drives
        the ticks), or a bound in ms; the default 0 raises ClSnapError(-9) at once if
        the snapshot has not completed."""
        if timeout_ms:
            self.wait_snapshot(snapshot_id, instance, instance + 1, timeout_ms)
        n, ch = self.num_nodes, self.num_channels
        tok = np.zeros(n, dtype=np.int64)
        off = np.zeros(ch + 1, dtype=np.int64)
        cap = 1024
        while True:
            msg = np.zeros(cap, dtype=np.int64)
            rc = self._L.cl_collect_snapshot(self._h, snapshot_id, instance, _p(tok), _p(off), _p(msg), cap)
            if rc == -7 and off[ch] > cap:
                cap = int(off[ch])
                continue
            _check(rc)
            break
        ids = self.node_ids()
        chans = self.channels()
        token_map = {ids[r]: int(tok[r]) for r in range(n)}
        order = sorted(range(ch), key=lambda c: (chans[c][1], chans[c][0]))
        msgs = [MsgSnapshot(ids[chans[c][0]], ids[chans[c][1]], int(msg[k]))
                for c in order for k in range(off[c], off[c + 1])]
        return GlobalSnapshot(snapshot_id, token_map, msgs)

    def poll_snapshot(self, snapshot_id, inst_lo=0, inst_hi=None):
        """Instances of [inst_lo, inst_hi) in which the snapshot has completed (the
        per-instance WaitGroup of sim.go:116-131); executes issued events, never ticks."""
        hi = self.n_instances if inst_hi is None else inst_hi
        v = C.c_int64(0)
        _check(self._L.cl_poll_snapshot(self._h, snapshot_id, inst_lo, hi, C.byref(v)))
        return v.value

    def wait_snapshot(self, snapshot_id, inst_lo=0, inst_hi=None, timeout_ms=-1):
        """Block until the snapshot has completed in every instance of [inst_lo,
        inst_hi); woken by the driver thread's executions.  Raises ClSnapError(-9) on
        timeout (timeout_ms >= 0)."""
        hi = self.n_instances if inst_hi is None else inst_hi
        v = C.c_int64(0)
        _check(self._L.cl_wait_snapshot(self._h, snapshot_id, inst_lo, hi, timeout_ms, C.byref(v)))
        return v.value

    def collect_snapshot_range(self, snapshot_id, inst_lo=0, inst_hi=None):
        """CollectSnapshot of many instances: (tokens[n, N] rank order, -1 where not
        complete; complete[n]; offsets[n * C + 1]; messages) -- one CSR over
        (instance, channel) with channels in (src rank, dest rank) order."""
        hi = self.n_instances if inst_hi is None else inst_hi
        k, n, ch = hi - inst_lo, self.num_nodes, self.num_channels
        tok = np.zeros((k, n), dtype=np.int64)
        done = np.zeros(k, dtype=np.int32)
        off = np.zeros(k * ch + 1, dtype=np.int64)
        cap = max(1024, 4 * k)
        while True:
            msg = np.zeros(cap, dtype=np.int64)
            rc = self._L.cl_collect_snapshot_range(self._h, snapshot_id, inst_lo, hi, _p(tok), _p(done), _p(off),
                                                   _p(msg), cap)
            if rc == -7 and off[-1] > cap:
                cap = int(off[-1])
                continue
            _check(rc)
            return tok, done.astype(bool), off, msg[:off[-1]]

    def collect_snapshot_packed(self, snapshot_id, inst_lo=0, inst_hi=None, out=None):
        """CollectSnapshot of many instances packed on the GPU (cl_collect_snapshot_packed):
        (tokens int32[n, N], complete bool[n], offsets int64[n * C + 1], messages int32).
        `out` = (tokens, complete, offsets, messages) arrays to fill (reused across calls; the
        message array is grown when too small: the returned messages are a view of the array
        actually filled, so pass that base array back in `out` to reuse it)."""
        hi = self.n_instances if inst_hi is None else inst_hi
        k, n, ch = hi - inst_lo, self.num_nodes, self.num_channels
        if out is None:
            out = (np.zeros((k, n), dtype=np.int32), np.zeros(k, dtype=np.int32),
                   np.zeros(k * ch + 1, dtype=np.int64), np.zeros(max(1024, 4 * k), dtype=np.int32))
        tok, done, off, msg = out
        # the C side writes k * N tokens, k flags, k * C + 1 offsets: a buffer sized for another
        # range would be overrun
        for name, a, shape, dt in (("tokens", tok, (k, n), np.int32), ("complete", done, (k,), np.int32),
                                   ("offsets", off, (k * ch + 1,), np.int64)):
            if not isinstance(a, np.ndarray) or a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError(f"collect_snapshot_packed: out {name} must be a C-contiguous {np.dtype(dt)} array "
                                 f"of shape {shape}")
        if not isinstance(msg, np.ndarray) or msg.dtype != np.int32 or msg.ndim != 1 or not msg.flags.c_contiguous:
            raise ValueError("collect_snapshot_packed: out messages must be a C-contiguous 1-d int32 array")
        m = C.c_int64(0)
        rc = self._L.cl_collect_snapshot_packed(self._h, snapshot_id, inst_lo, hi, _p(tok), _p(done), _p(off),
                                                _p(msg), msg.size, C.byref(m))
        if rc == -7 and m.value > msg.size:
            msg = np.zeros(m.value, dtype=np.int32)
            rc = self._L.cl_collect_snapshot_packed(self._h, snapshot_id, inst_lo, hi, _p(tok), _p(done), _p(off),
                                                    _p(msg), msg.size, C.byref(m))
        _check(rc)
        return tok, done.astype(bool), off, msg[:m.value]

    def collect_time(self):
        """Device ms of the latest packed collect's kernels."""
        ms = C.c_double(0)
        _check(self._L.cl_collect_time(self._h, C.byref(ms)))
        return ms.value

    def stats_layout(self, tick_lo=0, tick_bins=256, msg_bins=16):
        """cl_stats_layout_of as a dict (STATS_LAYOUT_FIELDS): host only, no device."""
        spec = np.array([tick_lo, tick_bins, msg_bins], dtype=np.int32)
        out = np.zeros(len(STATS_LAYOUT_FIELDS), dtype=np.int64)
        _check(self._L.cl_stats_layout_of(self._h, _p(spec), _p(out)))
        return dict(zip(STATS_LAYOUT_FIELDS, out.tolist()))

    def snapshot_stats(self, snapshot_id, inst_lo=0, inst_hi=None, tick_lo=0, tick_bins=256, msg_bins=16):
        """Distribution of snapshot `snapshot_id` over the OK instances of [inst_lo, inst_hi) in
        which it completed, reduced on the GPU (cl_snapshot_stats): a SnapshotStats with count,
        sum, sum of squares, min, max and histograms of the completion tick, each node's
        tokenMap entry, each channel's recorded messages and tokens, and the per-instance totals."""
        return self._stats(None, snapshot_id, inst_lo, inst_hi, tick_lo, tick_bins, msg_bins)

    def _stats(self, iset, snapshot_id, inst_lo, inst_hi, tick_lo, tick_bins, msg_bins):
        hi = self.n_instances if inst_hi is None else inst_hi
        layout = self.stats_layout(tick_lo, tick_bins, msg_bins)
        spec = np.array([tick_lo, tick_bins, msg_bins], dtype=np.int32)
        raw = np.zeros(layout["total_words"], dtype=np.int64)
        if iset is None:
            _check(self._L.cl_snapshot_stats(self._h, snapshot_id, inst_lo, hi, _p(spec), _p(raw), raw.size))
        else:
            _check(self._L.cl_snapshot_stats_in(self._h, snapshot_id, inst_lo, hi, iset._handle(), _p(spec), _p(raw),
                                                raw.size))
        return SnapshotStats(layout, raw)

    def snapshot_stats_in(self, snapshot_id, iset, inst_lo=0, inst_hi=None, tick_lo=0, tick_bins=256, msg_bins=16):
        """snapshot_stats over the members of the InstanceSet `iset` (cl_snapshot_stats_in): the
        sample is the members of [inst_lo, inst_hi) with status OK in which the snapshot completed;
        `instances` and `ok` still count the whole range.  A SnapshotStats like any other: it merges
        and reduces (dist.reduce_stats) unchanged."""
        return self._stats(iset, snapshot_id, inst_lo, inst_hi, tick_lo, tick_bins, msg_bins)

    def stats_time(self):
        """Device ms of the latest snapshot_stats kernel(s)."""
        ms = C.c_double(0)
        _check(self._L.cl_stats_time(self._h, C.byref(ms)))
        return ms.value

    def snapshot_census(self, snapshot_id, inst_lo=0, inst_hi=None, max_classes=4096, class_of=False, lds_slots=0):
        """The distinct global snapshots `snapshot_id` produced over the OK instances of
        [inst_lo, inst_hi) in which it completed, grouped on the GPU by content hash
        (cl_snapshot_census): a SnapshotCensus of at most `max_classes` classes, most frequent
        first.  class_of=True also returns each instance's class index.  lds_slots: 0 = the
        engine's workgroup table, -1 = none, else a power of two in [16, 4096] (results are the same)."""
        return self._census(None, snapshot_id, inst_lo, inst_hi, max_classes, class_of, lds_slots)

    def _census(self, iset, snapshot_id, inst_lo, inst_hi, max_classes, class_of, lds_slots):
        hi = self.n_instances if inst_hi is None else inst_hi
        spec = _CensusSpec(max_classes, lds_slots)
        classes = np.zeros(max(max_classes, 0), dtype=CENSUS_CLASS_DTYPE)
        cls = np.full(max(hi - inst_lo, 0), -1, dtype=np.int32) if class_of else None
        info = np.zeros(5, dtype=np.int64)
        tail = (C.byref(spec), _p(classes) if max_classes > 0 else None, _p(cls) if class_of else None, _p(info))
        if iset is None:
            _check(self._L.cl_snapshot_census(self._h, snapshot_id, inst_lo, hi, *tail))
        else:
            _check(self._L.cl_snapshot_census_in(self._h, snapshot_id, inst_lo, hi, iset._handle(), *tail))
        instances, ok, sample, n_classes, n_returned = info.tolist()
        return SnapshotCensus(snapshot_id, instances, ok, sample, n_classes, classes[:n_returned].copy(), cls)

    def snapshot_census_in(self, snapshot_id, iset, inst_lo=0, inst_hi=None, max_classes=4096, class_of=False,
                           lds_slots=0):
        """snapshot_census over the members of the InstanceSet `iset` (cl_snapshot_census_in); class_of
        is -1 for the instances of the range outside the conditional sample.  A SnapshotCensus like
        any other (dist.gather_census takes it unchanged)."""
        return self._census(iset, snapshot_id, inst_lo, inst_hi, max_classes, class_of, lds_slots)

    def census_time(self):
        """Device ms of the latest snapshot_census kernels."""
        ms = C.c_double(0)
        _check(self._L.cl_census_time(self._h, C.byref(ms)))
        return ms.value

    def select_clauses(self, where):
        """`where` of select_instances as a SELECT_CLAUSE_DTYPE array (host only): node ids and
        (src_id, dest_id) pairs mapped to ranks and channel numbers, None bounds opened, keys as
        uint64 bit patterns."""
        return _select_clauses(where, self.node_ids(), self.channels())

    def select_instances(self, snapshot_id, where=(), inst_lo=0, inst_hi=None, max_out=None, ticks=False):
        """The OK instances of [inst_lo, inst_hi) in which snapshot `snapshot_id` completed and that
        satisfy every clause of `where`, found on the GPU (cl_select_instances): a
        SnapshotSelection with the ascending instance indices.  A clause is (field, index, lo, hi)
        or (field, index, lo, hi, "not"): field one of SELECT_FIELDS; index None, a node id or
        rank ("node"), a channel number or (src_id, dest_id) pair ("ch_msgs", "ch_tok"); lo and
        hi inclusive, None for an open end.  max_out=None counts first and fetches every match;
        else at most max_out indices are returned (the smallest).  ticks=True also returns the
        completion ticks."""
        return self._select(None, snapshot_id, where, inst_lo, inst_hi, max_out, ticks)

    def _select(self, iset, snapshot_id, where, inst_lo, inst_hi, max_out, ticks):
        hi = self.n_instances if inst_hi is None else inst_hi
        clauses = self.select_clauses(where)
        info = np.zeros(5, dtype=np.int64)

        def call(cap):
            insts = np.zeros(max(cap, 0), dtype=np.int64)
            tk = np.zeros(max(cap, 0), dtype=np.int32) if ticks else None
            tail = (_p(clauses) if clauses.size else None, clauses.size, _p(insts) if cap > 0 else None,
                    _p(tk) if ticks and cap > 0 else None, cap, _p(info))
            if iset is None:
                _check(self._L.cl_select_instances(self._h, snapshot_id, inst_lo, hi, *tail))
            else:
                _check(self._L.cl_select_instances_in(self._h, snapshot_id, inst_lo, hi, iset._handle(), *tail))
            k = int(info[4])
            return insts[:k].copy(), None if tk is None else tk[:k].copy()

        if max_out is None:
            call(0)
            insts, tk = call(int(info[3]))
        else:
            insts, tk = call(max_out)
        instances, ok, sample, n_match, _ = info.tolist()
        return SnapshotSelection(snapshot_id, instances, ok, sample, n_match, insts, tk)

    def select_instances_in(self, snapshot_id, iset, where=(), inst_lo=0, inst_hi=None, max_out=None, ticks=False):
        """select_instances over the members of the InstanceSet `iset` (cl_select_instances_in)."""
        return self._select(iset, snapshot_id, where, inst_lo, inst_hi, max_out, ticks)

    def crosstab_axis(self, axis, name="a"):
        """An axis of snapshot_crosstab, (sid, field, index, lo, width, bins), as a
        CROSSTAB_AXIS_DTYPE record (host only): index normalised as in select_clauses."""
        return _crosstab_axis(name, axis, self.node_ids(), self.channels())

    def snapshot_crosstab(self, a, b, inst_lo=0, inst_hi=None):
        """The joint distribution of two snapshot quantities over the OK instances of
        [inst_lo, inst_hi) in which the snapshots of both axes completed, reduced on the GPU
        (cl_snapshot_crosstab): a SnapshotCrosstab with the contingency table and the joint
        moments.  An axis is (sid, field, index, lo, width, bins): field one of CROSSTAB_FIELDS,
        index as in a select clause, bin(v) = 0 below lo, else min((v - lo) // width, bins - 1).
        The axes may name different snapshot ids."""
        return self._crosstab(None, a, b, inst_lo, inst_hi)

    def _crosstab(self, iset, a, b, inst_lo, inst_hi):
        hi = self.n_instances if inst_hi is None else inst_hi
        a, b = self.crosstab_axis(a, "a"), self.crosstab_axis(b, "b")
        if int(a["bins"][0]) * int(b["bins"][0]) > CROSSTAB_MAX_CELLS:
            raise ValueError(f"crosstab: bins_a * bins_b <= {CROSSTAB_MAX_CELLS}")
        raw = np.zeros(XT_CELLS + int(a["bins"][0]) * int(b["bins"][0]), dtype=np.int64)
        if iset is None:
            _check(self._L.cl_snapshot_crosstab(self._h, inst_lo, hi, _p(a), _p(b), _p(raw), raw.size))
        else:
            _check(self._L.cl_snapshot_crosstab_in(self._h, inst_lo, hi, iset._handle(), _p(a), _p(b), _p(raw),
                                                   raw.size))
        return SnapshotCrosstab((a, b), raw)

    def snapshot_crosstab_in(self, iset, a, b, inst_lo=0, inst_hi=None):
        """snapshot_crosstab over the members of the InstanceSet `iset` (cl_snapshot_crosstab_in);
        `instances` and `ok` still count the whole range."""
        return self._crosstab(iset, a, b, inst_lo, inst_hi)

    def crosstab_time(self):
        """Device ms of the latest snapshot_crosstab kernel."""
        ms = C.c_double(0)
        _check(self._L.cl_crosstab_time(self._h, C.byref(ms)))
        return ms.value

    def group_terms(self, terms):
        """`terms` of snapshot_groups, each (sid, field, index), as a GROUP_TERM_DTYPE array (host
        only): field one of SELECT_FIELDS, index normalised as in select_clauses."""
        return _group_terms(terms, self.node_ids(), self.channels())

    def snapshot_groups(self, terms, inst_lo=0, inst_hi=None, max_groups=4096, group_of=False, lds_slots=0):
        """GROUP BY over the tuple of snapshot quantities `terms` (1 to 8 of (sid, field, index), which
        may name different snapshot ids) over the OK instances of [inst_lo, inst_hi) in which the
        snapshot of every term completed, on the GPU (cl_snapshot_groups): a SnapshotGroups of at
        most `max_groups` groups, most frequent first, each with its tuple of values.
        group_of=True also returns each instance's group index.  lds_slots as in snapshot_census.
        Adjacent terms of one snapshot id share one staging of its records: keep them together."""
        return self._groups(None, terms, inst_lo, inst_hi, max_groups, group_of, lds_slots)

    def _groups(self, iset, terms, inst_lo, inst_hi, max_groups, group_of, lds_slots):
        hi = self.n_instances if inst_hi is None else inst_hi
        t = self.group_terms(terms)
        spec = _CensusSpec(max_groups, lds_slots)
        groups = np.zeros(max(max_groups, 0), dtype=CENSUS_CLASS_DTYPE)
        values = np.zeros((max(max_groups, 0), t.size), dtype=np.int64)
        gof = np.full(max(hi - inst_lo, 0), -1, dtype=np.int32) if group_of else None
        info = np.zeros(5, dtype=np.int64)
        tail = (_p(t), t.size, C.byref(spec), _p(groups) if max_groups > 0 else None,
                _p(values) if max_groups > 0 else None, _p(gof) if group_of else None, _p(info))
        if iset is None:
            _check(self._L.cl_snapshot_groups(self._h, inst_lo, hi, *tail))
        else:
            _check(self._L.cl_snapshot_groups_in(self._h, inst_lo, hi, iset._handle(), *tail))
        instances, ok, sample, n_groups, n_returned = info.tolist()
        return SnapshotGroups(t, instances, ok, sample, n_groups, groups[:n_returned].copy(),
                              values[:n_returned].copy(), gof)

    def snapshot_groups_in(self, iset, terms, inst_lo=0, inst_hi=None, max_groups=4096, group_of=False, lds_slots=0):
        """snapshot_groups over the members of the InstanceSet `iset` (cl_snapshot_groups_in);
        `instances` and `ok` still count the whole range."""
        return self._groups(iset, terms, inst_lo, inst_hi, max_groups, group_of, lds_slots)

    def groups_time(self, stages=False):
        """Device ms of the latest snapshot_groups kernels; stages=True: the tuple (table
        initialisation, key pass, gather, group_of, values) whose sum it is."""
        if stages:
            ms = (C.c_double * 5)()
            _check(self._L.cl_groups_stage_times(self._h, ms))
            return tuple(ms)
        ms = C.c_double(0)
        _check(self._L.cl_groups_time(self._h, C.byref(ms)))
        return ms.value

    def order_term(self, term):
        """The term of an ordering call, (sid, field, index), as a GROUP_TERM_DTYPE array of one
        entry (host only): resolved exactly as a term of snapshot_groups."""
        return _order_term(term, self.node_ids(), self.channels())

    def snapshot_topk(self, term, k, largest=False, lo=0, hi=None):
        """ORDER BY `term` LIMIT k over the OK instances of [lo, hi) in which the term's snapshot
        completed, on the GPU (cl_snapshot_topk): a SnapshotTopK with the first min(k, sample)
        instances of the order and their values.  `term` is (sid, field, index) as in
        snapshot_groups ("key" is refused); ascending by (value, instance), or with largest=True
        by value descending, the instance still ascending.  k == 0 only counts."""
        return self._topk(None, term, k, largest, lo, hi)

    def _topk(self, iset, term, k, largest, lo, hi):
        hi = self.n_instances if hi is None else hi
        t = self.order_term(term)
        k = int(k)
        insts, vals = np.zeros(max(k, 0), dtype=np.int64), np.zeros(max(k, 0), dtype=np.int64)
        info = np.zeros(4, dtype=np.int64)
        tail = (_p(t), ORDER_DESC if largest else 0, k, _p(insts) if k > 0 else None, _p(vals) if k > 0 else None,
                _p(info))
        if iset is None:
            _check(self._L.cl_snapshot_topk(self._h, lo, hi, *tail))
        else:
            _check(self._L.cl_snapshot_topk_in(self._h, lo, hi, iset._handle(), *tail))
        instances, ok, sample, n = info.tolist()
        return SnapshotTopK(t, largest, k, instances, ok, sample, insts[:n].copy(), vals[:n].copy())

    def snapshot_topk_in(self, iset, term, k, largest=False, lo=0, hi=None):
        """snapshot_topk over the members of the InstanceSet `iset` (cl_snapshot_topk_in);
        `instances` and `ok` still count the whole range."""
        return self._topk(iset, term, k, largest, lo, hi)

    def snapshot_quantiles(self, term, qs, lo=0, hi=None):
        """Exact quantiles of `term` over the sample of [lo, hi), on the GPU (cl_snapshot_quantiles):
        a SnapshotQuantiles.  `qs`: up to 64 of (num, den), Fraction, 0, 1 or float (through
        Fraction(q).limit_denominator(10**9)); nearest rank, r = 0 if num == 0 else
        ceil(num * sample / den) - 1 in the ascending order."""
        return self._quantiles(None, term, qs, lo, hi)

    def _quantiles(self, iset, term, qs, lo, hi):
        hi = self.n_instances if hi is None else hi
        t, q = self.order_term(term), _quantiles(qs)
        values, ranks = np.zeros(q.size, dtype=np.int64), np.zeros(q.size, dtype=np.int64)
        info = np.zeros(4, dtype=np.int64)
        tail = (_p(t), _p(q), q.size, _p(values), _p(ranks), _p(info))
        if iset is None:
            _check(self._L.cl_snapshot_quantiles(self._h, lo, hi, *tail))
        else:
            _check(self._L.cl_snapshot_quantiles_in(self._h, lo, hi, iset._handle(), *tail))
        instances, ok, sample, _ = info.tolist()
        return SnapshotQuantiles(t, q, ranks, values, sample, instances, ok)

    def snapshot_quantiles_in(self, iset, term, qs, lo=0, hi=None):
        """snapshot_quantiles over the members of the InstanceSet `iset` (cl_snapshot_quantiles_in)."""
        return self._quantiles(iset, term, qs, lo, hi)

    def snapshot_values(self, term, lo=0, hi=None):
        """(values int64[hi - lo], in_sample bool[hi - lo]): `term` (any field, "key" as its int64
        bit pattern) of every instance of [lo, hi), 0 outside the sample, evaluated on the GPU
        (cl_snapshot_values): the bulk form of snapshot_ticks for any quantity."""
        return self._values(None, term, lo, hi)

    def _values(self, iset, term, lo, hi):
        hi = self.n_instances if hi is None else hi
        t = self.order_term(term)
        values, member = np.zeros(max(hi - lo, 0), dtype=np.int64), np.zeros(max(hi - lo, 0), dtype=np.uint8)
        if iset is None:
            _check(self._L.cl_snapshot_values(self._h, lo, hi, _p(t), _p(values), _p(member)))
        else:
            _check(self._L.cl_snapshot_values_in(self._h, lo, hi, iset._handle(), _p(t), _p(values), _p(member)))
        return values, member.astype(bool)

    def snapshot_values_in(self, iset, term, lo=0, hi=None):
        """snapshot_values over the members of the InstanceSet `iset` (cl_snapshot_values_in)."""
        return self._values(iset, term, lo, hi)

    def order_time(self, stages=False):
        """Device ms of the latest snapshot_topk / snapshot_quantiles / snapshot_values kernels;
        stages=True: the tuple (value walk, select passes, compaction) whose sum it is."""
        if stages:
            ms = (C.c_double * 3)()
            _check(self._L.cl_order_stage_times(self._h, ms))
            return tuple(ms)
        ms = C.c_double(0)
        _check(self._L.cl_order_time(self._h, C.byref(ms)))
        return ms.value

    def instance_set(self, snapshot_id, where=(), inst_lo=0, inst_hi=None):
        """The InstanceSet of the instances select_instances(snapshot_id, where, inst_lo, inst_hi)
        would return, built and kept on the GPU (cl_iset_from_clauses); its ``info`` is
        (instances, ok, sample, n_match) of that selection."""
        hi = self.n_instances if inst_hi is None else inst_hi
        clauses = self.select_clauses(where)
        info = np.zeros(5, dtype=np.int64)
        h = C.c_void_p()
        _check(self._L.cl_iset_from_clauses(self._h, snapshot_id, inst_lo, hi, _p(clauses) if clauses.size else None,
                                            clauses.size, C.byref(h), _p(info)))
        return InstanceSet(self, h, tuple(info[:4].tolist()))

    def instance_set_from(self, insts):
        """The InstanceSet of the listed instances (cl_iset_from_list): any order, duplicates allowed."""
        insts = np.ascontiguousarray(insts, dtype=np.int64).ravel()
        h = C.c_void_p()
        _check(self._L.cl_iset_from_list(self._h, _p(insts) if insts.size else None, insts.size, C.byref(h)))
        return InstanceSet(self, h)

    def iset_time(self):
        """Device ms of the latest InstanceSet kernels (list scatter, combine, count, listing);
        instance_set() is timed by select_time()."""
        ms = C.c_double(0)
        _check(self._L.cl_iset_time(self._h, C.byref(ms)))
        return ms.value

    def select_time(self, stages=False):
        """Device ms of the latest select_instances kernels, both stages; stages=True: the pair
        (evaluate ms, compact ms)."""
        if stages:
            a, b = C.c_double(0), C.c_double(0)
            _check(self._L.cl_select_stage_times(self._h, C.byref(a), C.byref(b)))
            return a.value, b.value
        ms = C.c_double(0)
        _check(self._L.cl_select_time(self._h, C.byref(ms)))
        return ms.value

    def snapshot_ticks(self, snapshot_id, inst_lo=0, inst_hi=None):
        """Completion tick of snapshot `snapshot_id` in every instance of [inst_lo, inst_hi)
        (int32, -1 = not complete): the bulk form of snapshot_tick (cl_snapshot_ticks)."""
        hi = self.n_instances if inst_hi is None else inst_hi
        out = np.full(max(hi - inst_lo, 0), -1, dtype=np.int32)
        _check(self._L.cl_snapshot_ticks(self._h, snapshot_id, inst_lo, hi, _p(out)))
        return out

    def collect_snapshot_list(self, snapshot_id, insts):
        """collect_snapshot_packed over an instance list (cl_collect_snapshot_list): row r is
        instance insts[r]; any order, duplicates allowed.  Same tuple as collect_snapshot_packed."""
        insts = np.ascontiguousarray(insts, dtype=np.int64).ravel()
        k, n, ch = insts.size, self.num_nodes, self.num_channels
        tok, done = np.zeros((k, n), dtype=np.int32), np.zeros(k, dtype=np.int32)
        off, msg = np.zeros(k * ch + 1, dtype=np.int64), np.zeros(max(1024, 4 * k), dtype=np.int32)
        m = C.c_int64(0)
        for _ in range(2):
            rc = self._L.cl_collect_snapshot_list(self._h, snapshot_id, _p(insts), k, _p(tok), _p(done), _p(off),
                                                  _p(msg), msg.size, C.byref(m))
            if rc != -7 or m.value <= msg.size:
                break
            msg = np.zeros(m.value, dtype=np.int32)
        _check(rc)
        return tok, done.astype(bool), off, msg[:m.value]

    # ---- drivers (test_common.go) -------------------------------------------
    def read_topology_file(self, path):           # test_common.go:29
        _check(self._L.cl_read_topology_file(self._h, path.encode()))

    def read_topology_text(self, text):
        _check(self._L.cl_read_topology_text(self._h, text.encode()))

    def read_events_file(self, path):             # test_common.go:79 (incl. drain)
        n = C.c_int32(0)
        _check(self._L.cl_read_events_file(self._h, path.encode(), C.byref(n)))
        return n.value

    def read_events_text(self, text):
        n = C.c_int32(0)
        _check(self._L.cl_read_events_text(self._h, text.encode(), C.byref(n)))
        return n.value

    def drain(self):                               # test_common.go:123-137
        _check(self._L.cl_drain(self._h))

    # ---- engine control -----------------------------------------------------
    def set_delay_schedule(self, delays):
        d = np.ascontiguousarray(delays, dtype=np.uint8)
        if d.ndim != 2 or d.shape[0] != self.n_instances:
            raise ClSnapError(-1, "schedule must be uint8[n_instances, draws]")
        _check(self._L.cl_set_delay_schedule(self._h, _p(d), d.shape[1]))

    def set_delay_go_seeds(self, seed_base):
        _check(self._L.cl_set_delay_go_seeds(self._h, seed_base))

    def set_delay_go_seed_list(self, seeds):
        """Instance i draws from rand.Seed(seeds[i]) (cl_set_delay_go_seed_list): e.g. the instances
        a selection named, re-run as their own batch with ``seed_base + insts``."""
        s = np.ascontiguousarray(seeds, dtype=np.int64)
        if s.ndim != 1:
            raise ClSnapError(E_INVALID, "seeds must be int64[n_instances]")
        _check(self._L.cl_set_delay_go_seed_list(self._h, _p(s), s.size))

    DELAY_GENERATORS = ("host", "device")

    def set_delay_generator(self, generator):
        """"host" (default) or "device": who makes the Go streams' delay rows (cl_set_delay_generator);
        the rows are the same bytes either way."""
        if generator not in self.DELAY_GENERATORS:
            raise ClSnapError(E_INVALID, f"delay generator must be one of {self.DELAY_GENERATORS}")
        _check(self._L.cl_set_delay_generator(self._h, self.DELAY_GENERATORS.index(generator)))

    @property
    def delay_generator(self):
        """The generator that made the rows now on the device: "host", "device", or None before any
        rows exist and for an explicit schedule."""
        m = self._i32(self._L.cl_delay_generator)
        return None if m < 0 else self.DELAY_GENERATORS[m]

    def delay_gen_time(self):
        """(kernel ms, host ms, rows patched on the host) of the latest delay generation."""
        d, h, p = C.c_double(0), C.c_double(0), C.c_int64(0)
        _check(self._L.cl_delay_gen_time(self._h, C.byref(d), C.byref(h), C.byref(p)))
        return d.value, h.value, p.value

    def set_limits(self, fifo_lds_slots=0, max_drain_ticks=10000):
        _check(self._L.cl_set_limits(self._h, fifo_lds_slots, max_drain_ticks))

    def flush(self):
        _check(self._L.cl_flush(self._h))

    def rerun(self):
        _check(self._L.cl_rerun(self._h))

    def synchronize(self):
        _check(self._L.cl_synchronize(self._h))

    def poison_outputs(self):
        """Overwrite every result plane with 0xA5 bytes (cl_debug_poison_outputs): results
        read after the next rerun() can only come from that launch."""
        _check(self._L.cl_debug_poison_outputs(self._h))

    def last_kernel_ms(self):
        ms = C.c_double(0)
        _check(self._L.cl_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def replay_split(self):
        """(instances that spilled in the probe run, -1 before it; first slot of the
        spill-capable part of split replays, 0 = no split) -- cl_replay_split."""
        a, b = C.c_int64(0), C.c_int64(0)
        _check(self._L.cl_replay_split(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def spill_free_replays(self):
        """True when the next rerun() runs wholly on the spill-free kernel (cl_replay_spill_free)."""
        v = C.c_int32(0)
        _check(self._L.cl_replay_spill_free(self._h, C.byref(v)))
        return bool(v.value)

    def mapped_replays(self):
        """True when the next rerun() launches through the length-ordered slot map."""
        v = C.c_int32(0)
        _check(self._L.cl_replay_mapped(self._h, C.byref(v)))
        return bool(v.value)

    def records_blocked(self):
        """True when the device's snapshot records are block-major by replay slot: the latest
        launch from the initial state was a replay through the slot map that saved no state
        image (rerun() of a mapped plan), on either exec kernel."""
        v = C.c_int32(0)
        _check(self._L.cl_records_blocked(self._h, C.byref(v)))
        return bool(v.value)

    # exec kernel choice (include/clsnap.h CL_ENGINE_*): results are identical on either kernel
    ENGINE_AUTO, ENGINE_NODES, ENGINE_LANES = 0, 1, 2

    def set_exec_engine(self, engine):
        _check(self._L.cl_set_exec_engine(self._h, int(engine)))

    def exec_engine(self):
        """The exec kernel the most recent launch used (ENGINE_NODES / ENGINE_LANES; 0 before any)."""
        return self._i32(self._L.cl_exec_engine)

    def lanes_compile_check(self):
        """Compile the instance-per-lane kernels for this topology without a device:
        (compile ms, compiler log); raises ClSnapError when they do not fit or fail to compile."""
        ms = C.c_double()
        buf = C.create_string_buffer(16384)
        _check(self._L.cl_lanes_compile_check(self._h, C.byref(ms), buf, len(buf)))
        return ms.value, buf.value.decode(errors="replace")

    # kernels specialized on the program for replays on the instance-per-lane kernels
    # (include/clsnap.h CL_PROGRAM_*): results are identical either way
    PROGRAM_AUTO, PROGRAM_OFF, PROGRAM_ON = 0, 1, 2

    def set_program_kernels(self, mode):
        _check(self._L.cl_set_program_kernels(self._h, int(mode)))

    def exec_program_kernels(self):
        """True when the most recent launch ran program-specialized kernels."""
        return bool(self._i32(self._L.cl_exec_program_kernels))

    def exec_program_cover(self):
        """True when the program-specialized kernels of the most recent launch, or of a later
        lanes_program_compile_check(), were compiled for delay rows that hold every draw the
        program can make (no row-end test in their broadcast guard) -- cl_exec_program_cover."""
        return bool(self._i32(self._L.cl_exec_program_cover))

    def lanes_program_compile_check(self):
        """Compile the kernels specialized on the current program without a device: (compile ms,
        specialized, compiler log); specialized is False (and nothing is compiled) for a program
        over the cap, which replays on the generic kernels."""
        ms, spec = C.c_double(), C.c_int32(0)
        buf = C.create_string_buffer(16384)
        _check(self._L.cl_lanes_program_compile_check(self._h, C.byref(ms), C.byref(spec), buf, len(buf)))
        return ms.value, bool(spec.value), buf.value.decode(errors="replace")

    def kernel_time(self):
        """(total exec-kernel ms, launches) since the previous call (HIP events)."""
        ms, n = C.c_double(0), C.c_int64(0)
        _check(self._L.cl_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- queries ------------------------------------------------------------
    def _i32(self, fn, *args):
        v = C.c_int32(0)
        _check(fn(self._h, *args, C.byref(v)))
        return v.value

    def _i64(self, fn):
        v = C.c_int64(0)
        _check(fn(self._h, C.byref(v)))
        return v.value

    @property
    def num_nodes(self):
        return self._i32(self._L.cl_num_nodes)

    @property
    def num_channels(self):
        return self._i32(self._L.cl_num_channels)

    @property
    def num_snapshots(self):
        return self._i32(self._L.cl_num_snapshots)

    @property
    def draws_needed(self):
        return self._i64(self._L.cl_delay_draws_needed)

    @property
    def device_bytes(self):
        return self._i64(self._L.cl_device_bytes)

    def node_ids(self):
        out = []
        for r in range(self.num_nodes):
            s = C.c_char_p()
            _check(self._L.cl_node_id(self._h, r, C.byref(s)))
            out.append(s.value.decode())
        return out

    def channels(self):
        out = []
        for c in range(self.num_channels):
            a, b = C.c_int32(), C.c_int32()
            _check(self._L.cl_channel(self._h, c, C.byref(a), C.byref(b)))
            out.append((a.value, b.value))
        return out

    def status(self):
        out = np.zeros(self.n_instances, dtype=np.int32)
        _check(self._L.cl_get_status(self._h, _p(out)))
        return out

    def time(self):
        out = np.zeros(self.n_instances, dtype=np.int32)
        _check(self._L.cl_get_time(self._h, _p(out)))
        return out

    def node_tokens(self, instance=0):
        out = np.zeros(self.num_nodes, dtype=np.int64)
        _check(self._L.cl_node_tokens(self._h, instance, _p(out)))
        return dict(zip(self.node_ids(), out.tolist()))

    def snapshot_tick(self, snapshot_id, instance=0):
        return self._i32(self._L.cl_snapshot_tick, snapshot_id, instance)

    def counters(self, only_ok=False):
        out = np.zeros(len(COUNTER_NAMES), dtype=np.int64)
        _check(self._L.cl_get_counters(self._h, 1 if only_ok else 0, _p(out)))
        return dict(zip(COUNTER_NAMES, out.tolist()))

    def instance_hashes(self, inst_lo=0, inst_hi=None):
        """Each instance's snapshot-hash term (the oracle's per-instance hash; 0 unless OK)."""
        hi = self.n_instances if inst_hi is None else inst_hi
        out = np.zeros(max(hi - inst_lo, 0), dtype=np.uint64)
        _check(self._L.cl_instance_hashes(self._h, inst_lo, hi - inst_lo, _p(out)))
        return out

    def checksums(self):
        out = np.zeros(len(SUM_NAMES), dtype=np.int64)
        _check(self._L.cl_get_checksums(self._h, _p(out)))
        return out

    # ---- device event trace: the reference's debug Logger (logger.go:12-76) ------
    def trace_enable(self, instance_lo=0, n_instances=1, capacity=4096):
        """Record the Logger of instances [instance_lo, instance_lo + n_instances); the
        next flush replays the event program with the trace build of the kernel."""
        _check(self._L.cl_trace_enable(self._h, instance_lo, n_instances, capacity))

    def trace(self, instance=0):
        """LogEvents of one traced instance in Logger order: (epoch, kind, node rank,
        other rank | -1, data, nodeTokens); kinds LOG_* (include/clsnap.h CL_LOG_*)."""
        n = C.c_int32(0)
        _check(self._L.cl_trace_read(self._h, instance, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 6), dtype=np.int32)
        _check(self._L.cl_trace_read(self._h, instance, _p(out), n.value, C.byref(n)))
        return [tuple(int(x) for x in r) for r in out[:n.value]]

    def pretty_print(self, instance=0):
        """Logger.PrettyPrint (logger.go:55-64) of a traced instance, as text."""
        return format_log(self.node_ids(), self.trace(instance))

    @staticmethod
    def status_string(code):
        return lib().cl_status_string(code).decode()
