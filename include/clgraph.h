/*
 * clgraph.h -- C ABI of the MI355X graph engine: ONE reference Chandy-Lamport
 * simulation (sim.go ChandyLamportSim) over a large topology, state in HBM.
 *
 * Where clsnap.h batches many copies of a small scenario (one wave segment per
 * instance), cl_graph runs a single instance whose nodes and channels span the whole
 * GPU: BASELINE configs 4 (2^20-node random 8-out-regular digraph, one snapshot under
 * continuous token traffic) and 5 (100k-node power-law graph, 4,096 overlapping
 * snapshots).  It keeps the reference's semantics bit-exactly -- tick order, same-tick
 * visibility, the global delay-draw order, per-channel recording -- and runs the
 * reference's test_data scenarios too (parity-tested against the golden snapshots).
 *
 * Conventions follow clsnap.h: int return codes (CL_OK / CL_E_*), cl_last_error(),
 * caller-allocated buffers, one host thread per cl_graph, node order = getSortedKeys
 * (common.go:135-146) rank, channel c = the c-th link in (src rank, dest rank) order.
 * Per-run fatal conditions become a status (CL_INST_*) and freeze the simulation.
 *
 * Event model.  The engine executes a program of steps; step k (simulator time k) is:
 *   1. synthetic traffic sends of step k (if configured, cl_graph_set_traffic),
 *   2. host events (cl_graph_send_tokens / cl_graph_start_snapshot) in call order,
 *   3. one Tick (sim.go:71-95).
 * Host calls only append to the program; cl_graph_flush() executes what is pending
 * on the GPU, and cl_graph_rerun() replays the whole program from the initial state.
 */
#ifndef CLGRAPH_H
#define CLGRAPH_H

#include <stdint.h>

#include "clsnap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- checksums (cl_graph_get_checksums), int64, all-reducible across ranks ---- */
#define CL_GSUM_OK 0             /* 1 if the run's status is CL_INST_OK */
#define CL_GSUM_DELIVERED 1      /* delivered packets (sim.go:85 pops) */
#define CL_GSUM_COMPLETED 2      /* globally completed snapshots */
#define CL_GSUM_CUT_RESIDUAL 3   /* sum over completed snapshots |tokens + recorded - total| */
#define CL_GSUM_FINAL_RESIDUAL 4 /* |final tokens + in-flight tokens - total| (checkTokens) */
#define CL_GSUM_DIGEST 5         /* sum of per-snapshot content digests */
#define CL_GSUM_IN_FLIGHT 6      /* token payloads still queued */
#define CL_NUM_GSUMS 7

typedef struct cl_graph cl_graph;

int cl_graph_create(cl_graph** out);
int cl_graph_destroy(cl_graph* g);
int cl_graph_set_device(cl_graph* g, int32_t device_ordinal);

/* ---- topology (before the first event) ------------------------------------- */
/* AddNode / AddLink (sim.go:40-56; node.go:45-55,87-94) and readTopologyFile
 * (test_common.go:29-68): string ids, ranked by lexicographic order at freeze. */
int cl_graph_add_node(cl_graph* g, const char* id, int64_t tokens);
int cl_graph_add_link(cl_graph* g, const char* src, const char* dest);
int cl_graph_read_topology_text(cl_graph* g, const char* text);
int cl_graph_read_topology_file(cl_graph* g, const char* path);
/* Bulk topology by rank: node r is "N" + r zero-padded to id_width digits (so rank ==
 * lexicographic order; id_width = 0 picks the digits of n_nodes-1), tokens[r]; the
 * links AddLink(src[i], dst[i]) with self links ignored and duplicates collapsed. */
int cl_graph_set_topology(cl_graph* g, int32_t n_nodes, int32_t id_width, const int64_t* tokens,
                          int64_t n_edges, const int32_t* src, const int32_t* dst);
/* Synthetic graphs:
 * regular: `degree` random permutations pi_p (Fisher-Yates driven by
 *   cl_counter_hash(seed, p, i)), links v -> pi_p(v);
 * powerlaw: `targets` links per node to ranks drawn from Zipf(exponent) over rank,
 *   plus ring links v -> v+1 and v -> v-1 when ring != 0.
 * Every node starts with `tokens` tokens. */
int cl_graph_generate_regular(cl_graph* g, int32_t n_nodes, int32_t degree, int64_t tokens, uint64_t seed);
int cl_graph_generate_powerlaw(cl_graph* g, int32_t n_nodes, int32_t targets, double exponent, int32_t ring,
                               int64_t tokens, uint64_t seed);

int cl_graph_num_nodes(cl_graph* g, int32_t* n);
int cl_graph_num_channels(cl_graph* g, int64_t* n);
/* src[c], dst[c] ranks of every channel, channel order */
int cl_graph_channels(cl_graph* g, int32_t* src, int32_t* dst);
/* node id of a rank, NUL-terminated into buf[cap] (CL_E_LIMIT if cap <= its length) */
int cl_graph_node_id(cl_graph* g, int32_t rank, char* buf, int32_t cap);
/* length of a rank's node id (bytes, without the NUL): size buf for cl_graph_node_id */
int cl_graph_node_id_length(cl_graph* g, int32_t rank, int32_t* len);

/* ---- configuration (before the first flush) -------------------------------- */
/* fifo_slots: ring slots per channel (power of two, 2..32768; deeper -> FIFO_OVERFLOW
 * status); max_snapshots: snapshot ids provisioned (0 = the program's count, at least
 * 16); max_drain_ticks bounds cl_graph_drain (HANG status). */
int cl_graph_set_limits(cl_graph* g, int32_t fifo_slots, int32_t max_snapshots, int64_t max_drain_ticks);
/* Delay source replacing rand.Intn(maxDelay) at sim.go:101; draw k of the run gets
 *   hash:     (cl_counter_hash(seed, k, 0) >> 32) % 5          (default, seed 0)
 *   go seed:  the k-th rand.Intn(5) of rand.Seed(seed)          (snapshot_test.go:20)
 *   schedule: delays[k] (values in [0, 5); DELAY_EXHAUSTED beyond n). */
int cl_graph_set_delay_hash(cl_graph* g, uint64_t seed);
int cl_graph_set_delay_go_seed(cl_graph* g, int64_t seed);
int cl_graph_set_delay_schedule(cl_graph* g, const uint8_t* delays, int64_t n);
/* Synthetic traffic: at every step k < steps, each node (rank order) holding tokens
 * with out-links sends ONE token when (uint32)cl_counter_hash(seed, k, rank) <
 * threshold, on out-link ((hash >> 32) * outdeg) >> 32 (SendTokens node.go:112-131). */
int cl_graph_set_traffic(cl_graph* g, uint64_t seed, uint32_t threshold, int64_t steps);
/* Diagnostic override of the push kernel's lanes per node: 0 = automatic (4 lanes below
 * 2^18 nodes, else 1), 1 or 4 = forced.  Results are identical either way; the tests run
 * both paths on the same graphs. */
int cl_graph_set_push_lanes(cl_graph* g, int32_t lanes);

/* ---- events ------------------------------------------------------------------ */
int cl_graph_send_tokens(cl_graph* g, const char* src, const char* dest, int64_t n);  /* sim.go:58-62 */
int cl_graph_send_tokens_rank(cl_graph* g, int32_t src, int32_t dest, int64_t n);
int cl_graph_start_snapshot(cl_graph* g, const char* node, int32_t* out_sid);         /* sim.go:105 */
int cl_graph_start_snapshot_rank(cl_graph* g, int32_t node, int32_t* out_sid);
int cl_graph_tick(cl_graph* g, int32_t n);                                             /* sim.go:71 */
/* test_common.go:123-137: tick until every snapshot started before this call has
 * completed, then maxDelay+1 more ticks.  Host-driven (checks completion between
 * ticks).  If it exceeds max_drain_ticks the run gets CL_INST_HANG and freezes: later
 * program ops do not execute. */
int cl_graph_drain(cl_graph* g);
int cl_graph_read_events_text(cl_graph* g, const char* text, int32_t* n_snapshots); /* test_common.go:79-140 */
int cl_graph_read_events_file(cl_graph* g, const char* path, int32_t* n_snapshots);

/* ---- execution ---------------------------------------------------------------- */
int cl_graph_flush(cl_graph* g);
/* Reset to the initial topology state and replay the whole program, asynchronously
 * when it has no drain (the benchmark step); cl_graph_synchronize() waits. */
int cl_graph_rerun(cl_graph* g);
int cl_graph_synchronize(cl_graph* g);
/* Device time of the runs since the previous call (HIP events on the engine stream
 * around each flush / rerun), the number of runs, and the ticks they executed. */
int cl_graph_run_time(cl_graph* g, double* total_ms, int64_t* runs, int64_t* ticks);
/* Test/benchmark aid: overwrite the run's result planes (node tokens, snapshot token maps
 * and cursors, completion ticks, counters) with 0xA5 bytes on the engine's stream, so
 * results read after the next cl_graph_rerun come from that run alone. */
int cl_graph_debug_poison_outputs(cl_graph* g);
/* Phases of the latest run: ms[0] / ticks[0] from its start to its first drain (the event
 * program's ticks: the traffic window of the synthetic workloads), ms[1] / ticks[1] the
 * drains (test_common.go:123-137); ms[1] = ticks[1] = 0 without a drain.  HIP events on the
 * engine's stream. */
int cl_graph_phase_time(cl_graph* g, double* ms /* [2] */, int64_t* ticks /* [2] */);
int cl_graph_device_bytes(cl_graph* g, int64_t* bytes);

/* ---- results (flush pending events first) ----------------------------------- */
int cl_graph_get_status(cl_graph* g, int32_t* status);
int cl_graph_get_time(cl_graph* g, int64_t* time);
int cl_graph_num_snapshots(cl_graph* g, int32_t* n);
int cl_graph_node_tokens(cl_graph* g, int64_t* out /* [num_nodes] */);
int cl_graph_snapshot_tick(cl_graph* g, int32_t sid, int32_t* tick);
/* CollectSnapshot (sim.go:134-173): tokens[rank] = tokenMap; the messages recorded on
 * channel c are msg_tokens[msg_offsets[c] .. msg_offsets[c+1]) in delivery order.
 * CL_E_NOT_COMPLETE if sid has not completed; CL_E_LIMIT (offsets written) if msg_cap
 * is too small. */
int cl_graph_collect_snapshot(cl_graph* g, int32_t sid, int64_t* tokens, int64_t* msg_offsets,
                              int64_t* msg_tokens, int64_t msg_cap);
/* CL_CNT_* counters (clsnap.h) of the run; recorded copies include channels still
 * recording at the end. */
int cl_graph_get_counters(cl_graph* g, int64_t* out /* [CL_NUM_COUNTERS] */);
int cl_graph_get_checksums(cl_graph* g, int64_t* out /* [CL_NUM_GSUMS] */);

/* ---- per-snapshot summary table, reduced on the device ---------------------------
 * One row per snapshot id of [sid_lo, sid_hi): one pass over the snapshot planes, and
 * (sid_hi - sid_lo) x 128 B cross to the host -- against one cl_graph_collect_snapshot
 * (N token words, E cursors and the payload history) per snapshot.  Epochs are the
 * reference Logger's (logger.go:12-76): start_tick is the epoch of the snapshot's
 * CL_LOG_START_SNAPSHOT record, a node's creation epoch that of the first
 * CL_LOG_RECV_MARKER of the snapshot delivered to it (the initiator's: start_tick).
 * The node fields cover the local snapshots created so far; the channel fields and the
 * digest are taken from completed snapshots only.  The digests of all rows sum (mod 2^64)
 * to CL_GSUM_DIGEST.  Partitioned runs: this device's part -- its nodes, the channels
 * into them, completion over its nodes. */
typedef struct cl_graph_snap_row {   /* 16 x int64 = 128 B */
  int64_t sid;
  int64_t initiator;        /* rank of the StartSnapshot node; -1 if this device does not own it (partitioned) */
  int64_t start_tick;       /* Logger epoch of its StartSnapshot record; -1 likewise */
  int64_t complete_tick;    /* cl_graph_snapshot_tick; -1 = not complete */
  int64_t nodes_created;    /* local snapshots created so far (== N when complete, unpartitioned) */
  int64_t last_create_tick; /* largest creation epoch over created nodes; -1 if none */
  int64_t node_tokens;      /* sum of the recorded node tokens over created nodes */
  int64_t min_node_tokens;  /* INT64_MAX if no node created */
  int64_t max_node_tokens;  /* INT64_MIN if no node created */
  int64_t rec_msgs;         /* recorded messages over all channels   -- complete snapshots only, else 0 */
  int64_t rec_tokens;       /* their token payloads                   -- " */
  int64_t rec_channels;     /* channels with at least one recorded message -- " */
  int64_t max_ch_msgs;      /* most messages recorded on one channel  -- " */
  int64_t digest;           /* this snapshot's term of CL_GSUM_DIGEST -- ", else 0 */
  int64_t reserved[2];      /* 0 */
} cl_graph_snap_row;
/* CL_E_INVALID unless 0 <= sid_lo <= sid_hi <= num_snapshots, or on a null `rows` with a
 * non-empty range; an empty range returns CL_OK and launches nothing. */
int cl_graph_snapshot_table(cl_graph* g, int32_t sid_lo, int32_t sid_hi, cl_graph_snap_row* rows /* [sid_hi - sid_lo] */);
/* Device ms of the latest table call's kernels (HIP events on the engine's stream). */
int cl_graph_table_time(cl_graph* g, double* ms);

/* ---- marker-wave profile and marker tree per snapshot, on the device ---------------
 * A node's local snapshot of a sid is created by the first marker of the sid delivered to it
 * (the reference's scan order: lowest tick, then lowest sender rank), or by StartSnapshot at
 * the initiator.  The engine keeps that tick and that sender per (snapshot, node); these calls
 * read them out at scale: how the marker wave spread over time, and the spanning tree it took.
 * Only the node records are read, no channel plane.  All results are exact integers and pure
 * functions of the run.
 *
 * cl_graph_snapshot_wave: row r (snapshot sid_lo + r) = CL_WV_HEAD + lat_bins + depth_bins
 * int64 words, reduced over the owned nodes that hold a local snapshot of the sid.
 *   latency  creation tick - origin (signed); bin = latency < 0 ? 0 : min(latency / lat_width,
 *            lat_bins - 1).  origins == NULL: the origin of a sid is the creation tick of its
 *            initiator's record -- the table's start_tick -- and -1 with the row left at its
 *            identities if the run never started it.  An origins array gives the origin of
 *            every row, whatever its sign.
 *   depth    (depth_bins > 0) tree edges from the node up to the initiator along the creating
 *            senders, the initiator at 0; bin = min(depth, depth_bins - 1).  Computed by pointer
 *            doubling over an 8-byte {ancestor, hops} pair per (sid, node); the sid range is
 *            processed in chunks whose pairs fit in 256 MiB (one sid at least), counted in
 *            cl_graph_device_bytes.  Rounds run until none moves a pair, at most 32.
 *   guard    before the first round every node's creating sender must lie in [0, N), hold a
 *            local snapshot of the sid and have a strictly smaller creation tick.  A node that
 *            fails is a root that is not the initiator; it and every node whose chain ends at
 *            it are left out of the depth fields and counted in CL_WV_BROKEN.  The engine's
 *            runs always pass: the guard keeps the call inside its planes and finite on any
 *            record contents, and CL_WV_BROKEN != 0 reports an engine defect.
 * Errors, all before any device work and with `out` untouched: CL_E_INVALID on a NULL g, spec
 * or out, lat_bins outside [1, CL_GRAPH_WAVE_MAX_BINS], lat_width < 1, depth_bins outside
 * [0, CL_GRAPH_WAVE_MAX_BINS], a non-zero reserved, or a range outside 0 <= sid_lo <= sid_hi <=
 * num_snapshots; CL_E_LIMIT if out_words < rows x row words; CL_E_STATE in a partitioned run with
 * depth_bins > 0 (the parents' records live on other devices) or with origins == NULL (only the
 * initiator's owner knows the start: pass the merged table's start_tick).  An empty range
 * returns CL_OK and launches nothing.  Partitioned runs: this device's nodes; the rows of the
 * parts add up (graph.py SnapshotWave.merge). */
#define CL_GRAPH_WAVE_MAX_BINS 1024
typedef struct { int32_t lat_bins, lat_width, depth_bins, reserved; } cl_graph_wave_spec;
#define CL_WV_SID 0
#define CL_WV_ORIGIN 1      /* the tick latencies are measured from */
#define CL_WV_CREATED 2     /* owned nodes with a local snapshot */
#define CL_WV_LAT_SUM 3
#define CL_WV_LAT_SUMSQ 4   /* modulo 2^64, like the batch statistics */
#define CL_WV_LAT_MIN 5     /* INT64_MAX when CREATED == 0 */
#define CL_WV_LAT_MAX 6     /* INT64_MIN when CREATED == 0 */
#define CL_WV_DEPTH_SUM 7
#define CL_WV_DEPTH_SUMSQ 8
#define CL_WV_DEPTH_MAX 9   /* -1 when depth is off or nothing was created */
#define CL_WV_BROKEN 10     /* nodes under a root the guard made; 0 in every run */
#define CL_WV_HEAD 12       /* word 11 reserved, 0; lat_hist[lat_bins], then depth_hist[depth_bins] follow */
int cl_graph_snapshot_wave(cl_graph* g, int32_t sid_lo, int32_t sid_hi, const cl_graph_wave_spec* spec,
                           const int64_t* origins /* [sid_hi - sid_lo] or NULL */, int64_t* out, int64_t out_words);
/* Device ms of the latest wave call's kernels (HIP events on the engine's stream, the reads of
 * the round flag between them included) and, with rounds != NULL, its doubling rounds: the most
 * any chunk of sids ran, the round that moved nothing included; 0 with the depth off.
 * CL_E_STATE before any wave call. */
int cl_graph_wave_time(cl_graph* g, double* ms, int32_t* rounds /* may be NULL */);
/* Bytes of scratch one chunk of sids may take in the wave and tree calls (0 = the default,
 * 256 MiB; a chunk holds one sid at least).  The results do not depend on it. */
int cl_graph_set_wave_scratch(cl_graph* g, int64_t bytes);
/* The tree itself over the owned ranks [node_lo, node_hi) (all nodes outside the partitioned
 * mode): parent[r][v - node_lo] = the rank of the creating sender of node v's local snapshot of
 * sid_lo + r (a global rank, also in a partitioned run), -1 at the initiator, -2 where there is
 * no local snapshot; tick = the creation epoch, or -1.  A pack kernel writes the two int32 planes
 * on the device, so 8 bytes per node cross to the host, 4 with tick == NULL.  CL_E_INVALID on a
 * NULL g or parent or a range outside 0 <= sid_lo <= sid_hi <= num_snapshots, before any device
 * work; an empty range returns CL_OK and launches nothing. */
int cl_graph_snapshot_tree(cl_graph* g, int32_t sid_lo, int32_t sid_hi,
                           int32_t* parent /* [sid_hi - sid_lo][node_hi - node_lo] */,
                           int32_t* tick /* same shape, or NULL */);

/* ---- sparse packed collect of snapshot contents, compacted on the device -----------
 * The recorded channel state of the COMPLETED snapshots of [sid_lo, sid_hi), one entry per
 * channel with at least one recorded message: entry i is channel ent_channel[i] (the channel
 * index of cl_graph_channels) with ent_count[i] messages; entries are ordered by snapshot id,
 * then ascending channel; the entries of snapshot sid_lo + r are [row_offsets[r],
 * row_offsets[r + 1]).  msg_tokens holds the token payloads of all entries back to back in
 * entry order, delivery order within a channel: entry i's start at the exclusive prefix sum of
 * ent_count.  complete[r] = 1 iff snapshot sid_lo + r has completed; an incomplete snapshot has
 * no entries.  tokens (optional) is the plane [n_sids][node_hi - node_lo] of recorded node
 * tokens, a row of -1 for an incomplete snapshot.  Partitioned runs: this device's part -- its
 * nodes [node_lo, node_hi), the channels into them, completion over its nodes.
 *
 * Only info, complete, row_offsets, the entries, the payloads and the token plane cross to the
 * host: nothing sized by the number of channels -- against N token words, E cursors and the
 * whole payload history per snapshot of cl_graph_collect_snapshot.
 *
 * Sizing: info, complete and row_offsets are written whenever the device scan has run.  If
 * n_entries > ent_cap, or msg_tokens != NULL and n_msgs > msg_cap, the call returns CL_E_LIMIT
 * and leaves the entry, payload and token arrays untouched: size them from info and call
 * again (ent_cap == 0 with NULL arrays is the sizing call).  msg_tokens == NULL skips the
 * payloads.  unit_payloads = 1: the run keeps no payload history, every payload is 1.
 * CL_E_INVALID (before any device work) on a NULL info, a range outside 0 <= sid_lo <= sid_hi
 * <= num_snapshots, a negative capacity, or NULL entry arrays with ent_cap > 0.  An empty range
 * returns CL_OK with info zeroed but for node_lo / node_hi and launches nothing. */
typedef struct cl_graph_sparse_info {   /* 8 x int64 = 64 B */
  int64_t n_sids;          /* sid_hi - sid_lo */
  int64_t n_complete;      /* completed snapshots among them */
  int64_t n_entries;       /* entries of all of them */
  int64_t n_msgs;          /* recorded messages of all entries */
  int64_t unit_payloads;   /* 1: no payload history, every payload is 1 */
  int64_t node_lo, node_hi; /* the owned node ranks (the token plane's columns) */
  int64_t reserved;        /* 0 */
} cl_graph_sparse_info;
int cl_graph_collect_sparse(cl_graph* g, int32_t sid_lo, int32_t sid_hi,
                            int32_t* complete /* [ns] or NULL */, int64_t* row_offsets /* [ns+1] or NULL */,
                            int32_t* ent_channel, int32_t* ent_count, int64_t ent_cap,
                            int32_t* msg_tokens /* [msg_cap] or NULL */, int64_t msg_cap,
                            int32_t* tokens /* [ns * (node_hi - node_lo)] or NULL */,
                            cl_graph_sparse_info* info);
/* Device ms of the latest sparse collect's kernels (HIP events on the engine's stream). */
int cl_graph_sparse_time(cl_graph* g, double* ms);

/* ---- node and channel profile over a snapshot range, reduced on the device ---------
 * The table, the wave and the sparse collect give one row per snapshot id.  This call reduces
 * the other way, over the USED snapshots of [sid_lo, sid_hi): one record per channel into an
 * owned node and one row per owned node.  ns = sid_hi - sid_lo; row r (snapshot sid_lo + r) is
 * used iff (use == NULL or use[r] != 0) and the snapshot has completed on this device -- the
 * cursors of an incomplete snapshot are undefined and are never read.  used[r] = 1 / 0,
 * CL_PF_N_USED their count.
 *
 * Per owned channel c over the used rows, with k_r(c) the messages snapshot r recorded on it and
 * t_r(c) their token payloads (k_r(c) where the run keeps no payload history): msgs = sum k_r,
 * tokens = sum t_r, snaps = #{r : k_r > 0}, peak = max k_r, peak_sid = the lowest sid with
 * k_r == peak (-1 where msgs == 0).  hist[b] counts the owned channels with b == min(msgs /
 * msg_width, msg_bins - 1): channels without a message fall in bin 0, and the bins sum to
 * CL_PF_CHANNELS.  `entries` gets one record for every owned channel with msgs >= min_msgs, in
 * ascending channel index.
 *
 * Per owned node v over the used rows (a used snapshot is complete, so v holds a local snapshot
 * of it), CL_PF_NODE_WORDS int64: tok_sum, tok_sumsq (modulo 2^64), tok_min, tok_max of the
 * recorded node tokens; lat_sum, lat_max of creation tick - origin[r], signed; in_msgs,
 * in_tokens = msgs and tokens summed over the channels into v.  With no used row a node row is
 * 0, 0, INT64_MAX, INT64_MIN, 0, INT64_MIN, 0, 0.  origins == NULL: the origin of a row is the
 * creation tick of its initiator's record, the table's start_tick; an origins array gives the
 * origin of every row, whatever its sign.
 *
 * Errors, all before any device work and with every output untouched: CL_E_INVALID on a NULL g,
 * spec or head, msg_bins outside [1, CL_GRAPH_PROFILE_MAX_BINS], msg_width < 1, min_msgs < 1, a
 * non-zero reserved, a range outside 0 <= sid_lo <= sid_hi <= num_snapshots, a negative ent_cap,
 * or NULL entries with ent_cap > 0; CL_E_STATE in a partitioned run with node_rows != NULL and
 * origins == NULL (only the initiator's owner knows the start: pass the merged table's
 * start_tick).  An empty range returns CL_OK and launches nothing; the head is zeroed but for
 * CL_PF_NODE_LO / CL_PF_NODE_HI.
 *
 * Sizing: head, hist and used are written whenever the reduction has run.  If CL_PF_ENTRIES >
 * ent_cap the call returns CL_E_LIMIT and leaves entries and node_rows untouched (ent_cap == 0
 * with NULL entries is the sizing call).  Nothing is cached between calls: a sizing call costs
 * one reduction.  Everything is an exact integer and a pure function of the run, the range, the
 * mask, the origins and the spec; nothing depends on the grid or on
 * cl_graph_set_profile_slices.  Partitioned runs: this device's part -- its nodes and the
 * channels into them (graph.py SnapshotProfile.merge joins the parts).  The scratch, 32 B per
 * owned in-position and 64 B per owned node, is counted in cl_graph_device_bytes. */
#define CL_GRAPH_PROFILE_MAX_BINS 1024
typedef struct { int32_t msg_bins, msg_width, min_msgs, reserved; } cl_graph_profile_spec;   /* 16 B */
typedef struct cl_graph_profile_entry {   /* 32 B */
  int32_t channel;    /* channel index of cl_graph_channels */
  int32_t snaps;      /* used snapshots with at least one recorded message on it */
  int32_t peak;       /* most messages one used snapshot recorded on it */
  int32_t peak_sid;   /* the lowest sid that recorded `peak` */
  int64_t msgs;       /* recorded messages over the used snapshots */
  int64_t tokens;     /* their token payloads (== msgs with unit payloads) */
} cl_graph_profile_entry;
/* head words, then hist[msg_bins] */
#define CL_PF_N_SIDS 0
#define CL_PF_N_USED 1
#define CL_PF_NODE_LO 2
#define CL_PF_NODE_HI 3
#define CL_PF_CHANNELS 4      /* owned channels: those into the owned nodes */
#define CL_PF_ACTIVE 5        /* owned channels with msgs > 0 */
#define CL_PF_ENTRIES 6       /* owned channels with msgs >= min_msgs */
#define CL_PF_MSGS 7
#define CL_PF_TOKENS 8
#define CL_PF_MAX_MSGS 9      /* largest msgs of one channel; 0 if none */
#define CL_PF_MAX_PEAK 10
#define CL_PF_MAX_SNAPS 11
#define CL_PF_UNIT_PAYLOADS 12
#define CL_PF_HEAD 16         /* words 13..15 reserved, 0 */
#define CL_PF_NODE_WORDS 8    /* tok_sum, tok_sumsq, tok_min, tok_max, lat_sum, lat_max, in_msgs, in_tokens */
int cl_graph_snapshot_profile(cl_graph* g, int32_t sid_lo, int32_t sid_hi, const cl_graph_profile_spec* spec,
                              const int32_t* use /* [ns] or NULL */, const int64_t* origins /* [ns] or NULL */,
                              int64_t* head /* [CL_PF_HEAD + msg_bins] */,
                              int32_t* used /* [ns] or NULL */,
                              int64_t* node_rows /* [(node_hi - node_lo) * CL_PF_NODE_WORDS] or NULL */,
                              cl_graph_profile_entry* entries, int64_t ent_cap);
/* Device ms of the latest profile call's kernels (HIP events on the engine's stream).
 * CL_E_STATE before any profile call. */
int cl_graph_profile_time(cl_graph* g, double* ms);
/* Slices of the used list the channel and node passes run in (0 = automatic; 1 = plain stores, no
 * atomics).  The results do not depend on it. */
int cl_graph_set_profile_slices(cl_graph* g, int32_t slices);

/* ---- restore: a new run that begins in a recorded cut, seeded on the device ---------
 * g: an unpartitioned graph whose run has status CL_INST_OK; sid: one of its completed
 * snapshots, with tokenMap T[v] and recorded messages m[c][0..k_c) per channel c in delivery
 * order (what cl_graph_collect_snapshot(g, sid) returns), M = sum of k_c.  *out is a new,
 * independent graph r:
 *   - the same topology (node ids, ranks, channel order), frozen: topology calls return
 *     CL_E_STATE;
 *   - initial node tokens T[v];
 *   - at simulator time 0, before step 0's synthetic traffic and before any host event, channel
 *     c's queue holds m[c][0..k_c), head first.  Message j of channel c was pushed with delay
 *     draw index off(c) + j, off = the exclusive prefix of k_c over channel order, and has
 *     receiveTime = GetReceiveTime(that draw, time 0) under r's delay source;
 *   - the draw counter and CL_CNT_PUSH start at M (pushes == draws stays true);
 *   - no Logger record of the seed, no snapshots, no history: snapshot ids start at 0;
 *   - r owns copies of all it needs: g may be rerun, advanced or destroyed afterwards;
 *   - cl_graph_rerun(r) resets to the seeded state.
 * With no synthetic traffic on r, r is indistinguishable -- status, time, node tokens after every
 * tick, counters, checksums, completion ticks, collected snapshots, table, wave -- from a fresh
 * graph of the same topology with node tokens T[v] + (payloads recorded on v's out-channels)
 * whose first host events of step 0 are SendTokens(src(c), dest(c), m[c][j]) in (c, j) order;
 * only that graph's M SENT_TOKEN Logger records differ.  With traffic the seed still comes first.
 *
 * r inherits g's device, fifo_slots, max_snapshots, max_drain_ticks, push lanes and delay source
 * (hash seed, Go seed or a copy of the schedule); not its traffic, trace or bound stream.  Until
 * its first flush r takes cl_graph_set_limits, _set_delay_*, _set_traffic, _set_push_lanes and
 * _trace_enable like any graph; cl_graph_set_device and cl_graph_part_begin return CL_E_STATE.
 * r runs partitioned through cl_graph_part_begin_seeded (below, with the partitioned mode), on any
 * number of devices, each of which holds the whole seed and queues its own channels' share of it.
 * A seeded channel with more messages than r's fifo_slots gives r's run CL_INST_FIFO_OVERFLOW, a
 * delay schedule shorter than M gives it CL_INST_DELAY_EXHAUSTED, either from before its first
 * event (only the status is specified then); exactly fifo_slots messages are fine.
 *
 * The seed is built by kernels from g's planes (the sparse collect's scan and write for one sid,
 * a prefix scan, a reduction) and stays on the device; the topology's device arrays are copied
 * device to device.  Every run of r from its initial state seeds its queues with one kernel.
 * Errors (*out = NULL): CL_E_INVALID, before any device work, on a NULL g or out or a sid outside
 * [0, num_snapshots); CL_E_STATE on a partitioned source or one whose run status is not
 * CL_INST_OK; CL_E_NOT_COMPLETE if the snapshot has not completed.  A partitioned run is
 * restored from through its merged cut: cl_graph_collect_sparse with tokens on every part,
 * merged by channel, into cl_graph_restore_cut below. */
int cl_graph_restore(cl_graph* g, int32_t sid, cl_graph** out);
typedef struct cl_graph_seed_info {     /* 8 x int64 = 64 B */
  int64_t source_sid;      /* the sid restored from */
  int64_t channels;        /* seeded channels (k_c > 0) */
  int64_t msgs;            /* M */
  int64_t tokens;          /* sum of the seeded payloads */
  int64_t max_ch_msgs;     /* the largest k_c */
  int64_t unit_payloads;   /* 1: every seeded payload is 1 */
  int64_t node_tokens;     /* sum of T[v] */
  int64_t reserved;        /* 0 */
} cl_graph_seed_info;
/* The seed of a restored graph; CL_E_STATE for a graph not made by cl_graph_restore. */
int cl_graph_seed_info_of(cl_graph* r, cl_graph_seed_info* info);
/* Device ms (HIP events): build_ms of the kernels of the restore call that made r, seed_ms of the
 * seed kernel of r's latest run from its initial state (0 before any).  CL_E_STATE for a graph
 * not made by cl_graph_restore.  cl_graph_device_bytes(r) counts the seed's buffers. */
int cl_graph_restore_time(cl_graph* r, double* build_ms, double* seed_ms);

/* ---- restore from a cut held on the host: saved, merged from a partitioned run, or hand-made ----
 * The cut takes the place of the snapshot's contents in cl_graph_restore: T = tokens, and the
 * recorded messages as the sparse collect lays them out -- one entry (channel, count) per channel
 * with messages, in channel order, the payloads back to back in entry order and delivery order
 * within an entry.  *out is a graph exactly as cl_graph_restore specifies it, with `topo` in the
 * place of g for all that is inherited (topology, device, fifo_slots, max_snapshots,
 * max_drain_ticks, push lanes, delay source; not traffic, trace, program or bound stream), and
 * cl_graph_seed_info_of, cl_graph_restore_time (build_ms: the check, offsets and sums kernels, the
 * uploads excluded), cl_graph_rerun and cl_graph_device_bytes work on it unchanged.
 *
 * topo needs only a topology: it may never have had an event or a flush, and may equally have
 * run.  The call freezes its topology like any call that needs rank order and uploads the
 * topology's arrays if they are not resident; it allocates none of topo's run state and changes
 * nothing else of it.  topo may be destroyed afterwards and serves any number of cuts.
 *
 * The arrays are uploaded and checked by a kernel before anything uses them; a graph is made
 * only from a cut that passed:
 *   (a) tokens[v] >= 0;
 *   (b) 0 <= channel[i] < E and channel[i-1] < channel[i];
 *   (c) 1 <= count[i] <= 32768 (the largest fifo_slots);
 *   (d) 0 <= msg_tokens[j] <= 0x7fffffff (bit 31 of a queued word marks a marker);
 *   (e) sum(count) == n_msgs.
 * A breach returns CL_E_INVALID with cl_last_error() naming the element as <field>[<index>] and
 * its value ((e): n_msgs and the sum); of several, the lowest rule in this order, then the lowest
 * index.  A count above r's fifo_slots but at most 32768 is valid and gives r's run
 * CL_INST_FIFO_OVERFLOW, a short schedule CL_INST_DELAY_EXHAUSTED, as in cl_graph_restore.
 * unit_payloads is 1 when msg_tokens is NULL or every payload is 1.
 * Errors answered before any device work (*out = NULL in every case): CL_E_INVALID on a NULL topo,
 * cut or out, a negative length, a NULL array with a positive length (msg_tokens excepted),
 * n_nodes != N, n_entries > E, n_msgs < n_entries or n_msgs > n_entries * 32768; CL_E_STATE on a
 * topo with no nodes or a partitioned one. */
typedef struct cl_graph_cut {       /* 64 B */
  int64_t source_sid;               /* reported back in cl_graph_seed_info.source_sid, not interpreted */
  int64_t n_nodes;
  const int32_t* tokens;            /* [n_nodes]   the tokenMap T */
  int64_t n_entries;
  const int32_t* channel;           /* [n_entries] channel index (cl_graph_channels), strictly ascending */
  const int32_t* count;             /* [n_entries] recorded messages, >= 1 */
  int64_t n_msgs;                   /* == sum of count */
  const int32_t* msg_tokens;        /* [n_msgs] payloads in entry order, delivery order within; NULL: all 1 */
} cl_graph_cut;
int cl_graph_restore_cut(cl_graph* topo, const cl_graph_cut* cut, cl_graph** out);

/* ---- device event trace: the reference's debug Logger (logger.go:12-76) ---------- */
/* Record up to `capacity` LogEvents from the next run on (0 = off, the default); the next
 * flush replays the program with tracing.  A debugging aid: records go through one device
 * counter, so keep it to graphs and runs of modest size. */
int cl_graph_trace_enable(cl_graph* g, int32_t capacity);
/* The Logger's records (cl_log_event, clsnap.h) in its order -- per epoch (simulator time),
 * the tick's deliveries in sender rank order with the broadcasts and EndSnapshot records
 * they cause, then that step's traffic sends in node order, then the host events -- with
 * LogEvent.nodeTokens.  *n_events = total; CL_E_LIMIT if the run overflowed the capacity. */
int cl_graph_trace_read(cl_graph* g, cl_log_event* out, int32_t cap, int32_t* n_events);

/* ---- graph-partitioned mode --------------------------
 * ONE simulation whose nodes are split into contiguous rank ranges over several devices
 * (one process per GPU).  Each device holds the graph-sized arrays but owns the tokens,
 * out-channel FIFOs and local snapshots of its nodes [node_lo, node_hi).  There is no
 * reference interface for this (the reference is one process); the caller moves the rows
 * between devices (graph.py PartitionedGraphSim over torch.distributed all-to-all).  One
 * tick:
 *   part_pick     time++, every owned sender pops its first due head (sim.go:71-95);
 *                 returns the deliveries to other devices' receivers, rows (s, v, k, pay).
 *   part_receive  applies the deliveries addressed here (every device's rows for its
 *                 nodes, any order), handles the markers (node.go:149-171); returns the
 *                 broadcast triggers of other devices' senders, rows (s0, outdeg).
 *   part_tally    applies the reports addressed here, tallies triggers and next-step sends
 *                 of the owned senders; totals[0..2] = (trigger draws, send draws, this
 *                 device's run status).  A device that froze (engine limit) tallies
 *                 nothing, so the caller allgathers the status with the totals and, when
 *                 any device has one, freezes every device (part_freeze) before part_bases:
 *                 no device then draws from stale totals.
 *   part_bases    bases[4] = (trigger draws of lower devices, of all, send draws of lower
 *                 devices, of all); returns the first draw of each reported sender s0.
 *   part_push     replies (s0, draw0) for broadcasts triggered by other devices' senders;
 *                 pushes broadcasts and traffic sends of step `step` (queue.go:18-20).
 * The step-0 traffic is part_tally(0) + part_bases + part_push(0) with no rows.
 * part_snapshot(node) must be called on every device (each counts the draws).  Queries
 * (node tokens, counters, snapshot ticks, collect) return this device's part: its nodes,
 * the channels into them, completion over its nodes; the program calls (tick, send,
 * flush of a program) return CL_E_STATE once the partitioned run began. */
int cl_graph_part_begin(cl_graph* g, int32_t node_lo, int32_t node_hi);
/* The same for a restored graph r (cl_graph_restore, cl_graph_restore_cut) before its first flush:
 * the partitioned run's time-0 state is the recorded cut.  Every device restores the whole cut
 * (like every other array of the mode, the seed is graph-sized on each) and calls this with its
 * own range; the number of devices need not be that of the run that wrote the cut.  A device
 * owns the queues of its nodes' out-channels, and channels are ordered by (src rank, dest rank):
 * its channels are [out_off[node_lo], out_off[node_hi]), its entries a contiguous slice [e_lo,
 * e_hi) of the cut's ascending entries, and its messages the slice [m_lo, m_hi) = [moff(e_lo),
 * moff(e_hi)) of the draw order of cl_graph_restore (moff = the exclusive prefix of the counts).
 * The effect is cl_graph_part_begin's, except that
 *   - the node tokens are the cut's T[v];
 *   - after the reset and before anything else every owned channel holds exactly what the
 *     unpartitioned r's queue holds at time 0: message q of entry i has receiveTime
 *     GetReceiveTime(draw moff(i) + q, time 0) under r's delay source (counter hash or explicit
 *     schedule) -- the global draw index, whichever device queues it; other devices' channels
 *     get nothing;
 *   - the draw counter starts at M on every device, and CL_CNT_PUSH at m_hi - m_lo, so the
 *     devices' counters sum to the unpartitioned run's M.
 * What cannot be seeded is judged on the whole cut, the same on every device: max_ch_msgs above
 * fifo_slots sets CL_INST_FIFO_OVERFLOW, a schedule shorter than M CL_INST_DELAY_EXHAUSTED, at
 * begin and with nothing queued; the first part_tally / dev_bases (the step-0 traffic) then stops
 * every device at time 0.  The slice is found and queued by two kernels; one synchronisation.
 * cl_graph_seed_info_of(r) still describes the whole cut, cl_graph_restore_time's seed_ms is this
 * device's seed kernel.  Errors: CL_E_STATE, before any device work, for a graph that is not
 * restored; every refusal of cl_graph_part_begin otherwise (begun already, a non-empty program,
 * the trace, a Go-seed delay source: CL_E_STATE; an unaligned or out-of-bounds range:
 * CL_E_INVALID), after which r is what it was and still runs unpartitioned. */
int cl_graph_part_begin_seeded(cl_graph* r, int32_t node_lo, int32_t node_hi);
/* out = (e_lo, e_hi, m_lo, m_hi): the slice of the cut's entries and messages this device
 * queued.  CL_E_STATE before cl_graph_part_begin_seeded and for a graph that is not restored. */
int cl_graph_part_seed_share(cl_graph* r, int64_t out[4]);
int cl_graph_part_snapshot(cl_graph* g, int32_t node, int32_t* out_sid);
int cl_graph_part_pick(cl_graph* g, int32_t* rows, int64_t cap, int64_t* n_rows);
int cl_graph_part_receive(cl_graph* g, const int32_t* rows, int64_t n, int32_t* reports, int64_t cap,
                          int64_t* n_reports);
int cl_graph_part_tally(cl_graph* g, int32_t step, const int32_t* reports, int64_t n, int64_t* totals);
int cl_graph_part_bases(cl_graph* g, const int64_t* bases, const int32_t* s0, int64_t n, int64_t* draw0);
int cl_graph_part_push(cl_graph* g, int32_t step, const int64_t* replies, int64_t n);
/* Freeze this device's part of the run with `status` (no-op if it is already frozen):
 * another device froze, and the partitioned run stops everywhere at the same step. */
int cl_graph_part_freeze(cl_graph* g, int32_t status);

/* ---- partitioned mode, device-resident exchange ---------------------------------------
 * The same tick with every exchanged row kept in device memory: the caller binds four
 * device buffers it owns (torch tensors) and runs the collectives between the steps on
 * the engine's stream (cl_graph_set_stream: torch's current stream), so a tick needs no
 * host round trip (RCCL all-to-all / all-gather over xGMI with one process per GPU).
 *   send, recv  world * (cap + 1) rows of 16 B each: bucket q = a header row {rows, 0, 0, 0},
 *               then up to `cap` rows; send bucket q goes to rank q and recv bucket q came
 *               from rank q (all_to_all_single with equal splits);
 *   tot_send    4 int64 (this rank's trigger draws, send draws, status, 0);
 *   tot_recv    world * 4 int64 (all_gather of tot_send).
 * `cap` must bound every bucket: for ranks r != q, the number of r's nodes with a channel
 * into q's nodes (graph.py computes it from the topology); `span` = nodes per rank
 * (owner(v) = v / span, the block-aligned ranges of part_begin).  One tick:
 *   dev_pick      time++, pops; deliveries to other ranks' receivers -> send       [all-to-all]
 *   dev_receive   recv deliveries + own markers; broadcast reports (s0, outdeg) -> send
 *                                                                                  [all-to-all]
 *   dev_tally     recv reports, tally of triggers and next-step sends -> tot_send  [all-gather]
 *   dev_bases     draw bases from tot_recv (a frozen rank freezes every rank); replies
 *                 (s0, first draw) to the reporters -> send                       [all-to-all]
 *   dev_push      recv replies; pushes of broadcasts and the traffic of `step`.
 * The step-0 traffic: dev_seal (empty reports) [all-to-all] dev_tally(0) [all-gather]
 * dev_bases [all-to-all] dev_push(0).  The results are part_* queries as above. */
int cl_graph_part_dev_bind(cl_graph* g, int32_t world, int32_t rank, int32_t span, int64_t cap, void* send,
                           void* recv, void* tot_send, void* tot_recv);
int cl_graph_part_dev_seal(cl_graph* g);
int cl_graph_part_dev_pick(cl_graph* g);
int cl_graph_part_dev_receive(cl_graph* g);
int cl_graph_part_dev_tally(cl_graph* g, int32_t step);
int cl_graph_part_dev_bases(cl_graph* g);
int cl_graph_part_dev_push(cl_graph* g, int32_t step);
/* Run every later launch and copy of this engine on `stream` (a hipStream_t of the engine's
 * device, e.g. torch.cuda.current_stream().cuda_stream; NULL = the engine's own stream).
 * The engine waits for its own stream first. */
int cl_graph_set_stream(cl_graph* g, void* stream);

/* ---- counter hash of the synthetic workloads ------------------------------------ */
uint64_t cl_counter_hash(uint64_t seed, uint64_t a, uint64_t b);

#ifdef __cplusplus
}
#endif
#endif /* CLGRAPH_H */
