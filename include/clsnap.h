/*
 * clsnap.h -- C ABI of the MI355X Chandy-Lamport batch engine.
 *
 * One cl_sim is a batch of n_instances independent copies of the reference simulator
 * (sim.go ChandyLamportSim).  Every instance shares the topology and receives the same
 * event stream (send / snapshot / tick), but draws its own per-message delays, so each
 * instance is the reference run under its own delay stream.  Instances run as
 * tick-synchronous simulations on one gfx950 GPU; results are bit-exact per instance.
 *
 * Each entry point below names the reference interface it replaces
 * (paths relative to /root/reference/chandy_lamport).  The reference is a Go package
 * with no FFI; INTEGRATION.md shows the cgo binding that maps this ABI back onto the
 * reference's Simulator API so the .top/.events drivers and snapshot_test.go run
 * unchanged.
 *
 * Conventions
 *   - Every call returns int: CL_OK (0) or a negative CL_E_* code; cl_last_error()
 *     describes the most recent failure on the calling thread.
 *   - All buffers are caller-allocated; no pointer returned by the library is owned by
 *     the caller except where stated.
 *   - One host thread drives a cl_sim (events, ticks, flush).  Event calls only append
 *     to the sim's event program; cl_flush() (or any result query) executes pending
 *     events on the GPU.  Every call holds the sim's lock, so other threads may call
 *     cl_poll_snapshot / cl_wait_snapshot / cl_collect_snapshot* concurrently -- the
 *     reference collects each snapshot on its own goroutine while the driver ticks
 *     (test_common.go:106-108, sim.go:134-173).  Those calls execute events already
 *     issued but never add a tick.
 *   - Node order everywhere is the reference's getSortedKeys order (common.go:135-146):
 *     lexicographic byte order of the node IDs ("rank").  Channel c is the c-th link in
 *     (src rank, dest rank) order -- the order Tick scans senders and out-links
 *     (sim.go:76-78).
 *   - Where the reference calls log.Fatal* on a per-run condition, the affected
 *     instance gets a CL_INST_* status and freezes; API misuse that the reference
 *     turns into a process exit or nil dereference returns a CL_E_* code instead.
 */
#ifndef CLSNAP_H
#define CLSNAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes ------------------------------------------------------- */
#define CL_OK 0
#define CL_E_INVALID (-1)        /* bad argument or handle */
#define CL_E_UNKNOWN_NODE (-2)   /* sim.go:49-54 log.Fatalf; nil *Node at sim.go:61,106 */
#define CL_E_DUPLICATE_NODE (-3) /* sim.go:42 would silently replace a wired node */
#define CL_E_PARSE (-4)          /* test_common.go parse fatals (:45,52,58,93,119,...) */
#define CL_E_IO (-5)             /* ioutil.ReadFile failure (test_common.go:30,80) */
#define CL_E_DEVICE (-6)         /* HIP error or no gfx950 device */
#define CL_E_LIMIT (-7)          /* engine limit (nodes, snapshots, token range) */
#define CL_E_STATE (-8)          /* topology change after events started, etc. */
#define CL_E_NOT_COMPLETE (-9)   /* collect of a snapshot that has not completed */

/* ---- per-instance status (cl_get_status) -------------------------------- */
#define CL_INST_OK 0
#define CL_INST_FATAL_INSUFFICIENT_TOKENS 1 /* node.go:113-116 */
#define CL_INST_FATAL_UNKNOWN_DEST 2        /* node.go:121-124 */
#define CL_INST_FIFO_OVERFLOW 3             /* engine: channel deeper than 255 packets */
#define CL_INST_HANG 4                      /* drain exceeded max ticks (test_common.go:124-132 loops forever) */
#define CL_INST_DELAY_EXHAUSTED 5           /* replayed delay schedule too short */
#define CL_INST_HIST_OVERFLOW 6             /* graph engine: token history slots exhausted */
#define CL_INST_XCHG_OVERFLOW 7             /* partitioned graph run: a device exchange bucket overflowed */

/* ---- counters (cl_get_counters), summed over instances ------------------ */
#define CL_CNT_PUSH 0      /* Queue.Push (queue.go:18) == delay draws (sim.go:101) */
#define CL_CNT_PEEK 1      /* Queue.Peek inside Tick (sim.go:83) */
#define CL_CNT_POP_TOKEN 2 /* delivered token packets (sim.go:85) */
#define CL_CNT_POP_MARKER 3
#define CL_CNT_RECORDED 4  /* recorded message copies (node.go:179-183) */
#define CL_CNT_COMPLETED 5 /* globally completed snapshots (sim.go:126-131) */
#define CL_CNT_INSTANCES 6 /* instances counted */
#define CL_CNT_TICKS 7     /* sum of per-instance simulator time */
#define CL_NUM_COUNTERS 8

/* ---- checksums (cl_get_checksums): int64 sums, all-reducible across ranks -- */
#define CL_SUM_INSTANCES 0       /* instances in the batch */
#define CL_SUM_OK 1              /* status OK */
#define CL_SUM_FATAL 2           /* FATAL_* statuses */
#define CL_SUM_OTHER 3           /* FIFO_OVERFLOW / HANG / DELAY_EXHAUSTED */
#define CL_SUM_DELIVERED 4       /* packets delivered by OK instances */
#define CL_SUM_SNAPSHOT_HASH 5   /* sum of snapshot content hashes over OK instances */
#define CL_SUM_CUT_RESIDUAL 6    /* sum |snapshot tokens + recorded - total| (0 = consistent cuts) */
#define CL_SUM_FINAL_RESIDUAL 7  /* sum |final tokens + in-flight tokens - total| (checkTokens) */
#define CL_SUM_COMPLETED 8       /* completed snapshots over OK instances */
#define CL_SUM_IN_FLIGHT 9       /* token packets still queued at the end (OK instances) */
#define CL_NUM_SUMS 10

typedef struct cl_sim cl_sim;

/* NewSimulator (sim.go:28-37) for n_instances independent instances. No GPU work. */
int cl_sim_create(int64_t n_instances, cl_sim** out);
/* Wakes every thread blocked in cl_wait_snapshot (they return CL_E_STATE) and waits for
 * them to leave before freeing the sim; no other call may overlap it. */
int cl_sim_destroy(cl_sim* sim);

/* AddNode (sim.go:40-43; node.go:45-55). Each token count is an int32, negative allowed. The
 * positive counts of all nodes must sum to at most INT32_MAX (a node never drops below min(start, 0), so
 * none exceeds its start plus the others' positive counts: every node word stays in int32) and
 * the total must be at least INT32_MIN: CL_E_LIMIT otherwise. A refused call adds nothing. */
int cl_add_node(cl_sim* sim, const char* id, int64_t tokens);
/* AddLink (sim.go:46-56; node.go:87-94): self links ignored, duplicates replace. */
int cl_add_link(cl_sim* sim, const char* src, const char* dest);
/* readTopologyFile (test_common.go:29-68) on a file path / on text. */
int cl_read_topology_file(cl_sim* sim, const char* path);
int cl_read_topology_text(cl_sim* sim, const char* text);

/* Engine configuration (before the first flush). */
int cl_set_device(cl_sim* sim, int32_t device_ordinal);
/* fifo_lds_slots: per-channel packets kept in LDS (power of two, 2..64; deeper
 * channels spill to HBM), or 0 to size it automatically for occupancy (default).
 * max_drain_ticks bounds the drain loop (HANG status). */
int cl_set_limits(cl_sim* sim, int32_t fifo_lds_slots, int64_t max_drain_ticks);

/* Delay source replacing rand.Intn(maxDelay) at sim.go:101.
 * Go stream: instance i draws from rand.Seed(seed_base + i) -- the reference's own
 * generator (snapshot_test.go:20), restated bit-exactly and precomputed on the host. */
int cl_set_delay_go_seeds(cl_sim* sim, int64_t seed_base);
/* Explicit schedule: delays[i * draws_per_instance + k] in [0, 5) is the k-th draw
 * of instance i.  Copied; the caller may free it after the call. */
int cl_set_delay_schedule(cl_sim* sim, const uint8_t* delays, int64_t draws_per_instance);
/* Go stream with one seed per instance: instance i draws from rand.Seed(seeds[i]); any int64 is a
 * seed (rng.go reduces it mod 2^31 - 1).  E.g. the instances cl_select_instances named, re-run as
 * a batch of their own with seeds[k] = seed_base + insts[k].  n must be the instance count
 * (CL_E_INVALID otherwise, and for NULL); the list is copied.  Works with both generators below;
 * replaces, and is replaced by, cl_set_delay_go_seeds and cl_set_delay_schedule. */
int cl_set_delay_go_seed_list(cl_sim* sim, const int64_t* seeds, int64_t n);
/* Which generator makes the Go streams' delay rows:
 *   CL_DELAYGEN_HOST    (default) sequential generators on up to 16 host threads, then one copy
 *                       of the n_instances x row plane to the device
 *   CL_DELAYGEN_DEVICE  a gfx950 kernel writes the plane in device memory from the generator's
 *                       closed form; no host plane, no copy.  A row in which Go's
 *                       Intn(5) rejects an output and draws again (about one row in 6 million at
 *                       100 draws) is regenerated sequentially on the host and patched in.  The
 *                       seed list, if any, then lives in device memory only.
 * The rows are the same bytes either way.  Rows longer than CL_DELAYGEN_MAX_DRAWS (one wave
 * keeps a row's 8-byte outputs in LDS), planes of 2^31 dwords or more, and batches in which more
 * than 4,096 rows met a rejection silently take the host generator; cl_delay_generator tells.
 * CL_E_INVALID for another mode.  Like cl_set_delay_go_seeds it may be called at any time: a
 * change makes the next flush generate the rows again and replay the program from the start. */
#define CL_DELAYGEN_HOST 0
#define CL_DELAYGEN_DEVICE 1
#define CL_DELAYGEN_MAX_DRAWS 4096
int cl_set_delay_generator(cl_sim* sim, int32_t mode);
/* The generator that made the rows now on the device (CL_DELAYGEN_*); -1 before any rows exist
 * and for an explicit schedule. */
int cl_delay_generator(cl_sim* sim, int32_t* mode);
/* The latest generation of Go-stream rows (CL_E_STATE before any): device_ms = the generator
 * kernel, from HIP events around it (0 for the host generator); host_ms = wall time of the host
 * generator and its copy, or of patching the rejected rows; patched_rows = rows regenerated on
 * the host after the kernel.  Any of the three pointers may be NULL. */
int cl_delay_gen_time(cl_sim* sim, double* device_ms, double* host_ms, int64_t* patched_rows);

/* ProcessEvent(PassTokenEvent) -> SendTokens (sim.go:58-62; node.go:112-131). */
int cl_send_tokens(cl_sim* sim, const char* src, const char* dest, int64_t n);
/* ProcessEvent(SnapshotEvent) -> StartSnapshot (sim.go:63-64,105-123). */
int cl_start_snapshot(cl_sim* sim, const char* node, int32_t* out_sid);
/* Tick (sim.go:71-95), n times. */
int cl_tick(cl_sim* sim, int32_t n);
/* The drain of readEventsFile (test_common.go:123-137): tick until every started
 * snapshot has completed in an instance, then maxDelay+1 more ticks (per instance). */
int cl_drain(cl_sim* sim);
/* readEventsFile (test_common.go:79-140) incl. the drain; n_snapshots may be NULL. */
int cl_read_events_file(cl_sim* sim, const char* path, int32_t* n_snapshots);
int cl_read_events_text(cl_sim* sim, const char* text, int32_t* n_snapshots);

/* Execute pending events on the GPU and wait. */
int cl_flush(cl_sim* sim);
/* Re-run the whole event program from the initial topology state (asynchronous on
 * the sim's stream; inputs stay resident in HBM).  cl_synchronize() waits.  A replay split
 * over two streams (cl_replay_split) leaves its spill-capable half running when the call
 * returns: back-to-back cl_rerun calls overlap that half with the next replay's spill-free
 * half (they touch disjoint instances); every other call waits for it first. */
int cl_rerun(cl_sim* sim);
int cl_synchronize(cl_sim* sim);
/* Device time of the most recent cl_flush/cl_rerun kernel, from HIP events recorded by the
 * kernel dispatches themselves; a split replay's time is the longer of its two concurrent
 * halves, each timed by its own dispatch's events. */
int cl_last_kernel_ms(cl_sim* sim, double* ms);
/* Sum of exec-kernel device times (as cl_last_kernel_ms, every launch) since the previous
 * call, and the number of launches; resets the accumulator. */
int cl_kernel_time(cl_sim* sim, double* total_ms, int64_t* launches);
/* 1 in *on when the next cl_rerun runs wholly on the spill-free kernel: the layout has no HBM
 * spill rings, or the first full run of the same program with the same delays and layout
 * spilled nothing (engine-internal specialization; results are the same either way). */
int cl_replay_spill_free(cl_sim* sim, int32_t* on);
/* The replay plan of the current program (from its first full run): instances whose queues
 * outgrew the LDS rings (-1: no plan yet), and the slot from which replays run on the
 * spill-capable kernel while the slots before it run spill-free, concurrently (0: no split).
 * Engine-internal; results are the same either way. */
int cl_replay_split(cl_sim* sim, int64_t* spill_instances, int64_t* split_slot);
/* 1 in *on when the next cl_rerun launches through the replay plan's slot map (instances
 * grouped by the final tick of an earlier full run of the same program and delays, so the
 * instances sharing a wave finish together, and those that spilled last; engine-internal,
 * results unchanged). */
int cl_replay_mapped(cl_sim* sim, int32_t* on);
/* The planning policy behind the three calls above, on the host alone (no sim, no device): from
 * every instance's final tick and spill flag (spilled NULL: none spilled), the layout's instances
 * per wave and whether the kernels can split a replay, the slot order (order[n]: slot ->
 * instance), whether replays launch through it, the split slot and the spilled instances.
 * CL_E_INVALID for NULL final_ticks, n <= 0 or insts_per_wave <= 0; any output may be NULL.
 * Engine-internal: it exists so the policy can be tested without a GPU. */
int cl_replay_plan_of(const int32_t* final_ticks, const uint8_t* spilled, int64_t n, int32_t insts_per_wave,
                      int32_t can_split, int32_t* order, int32_t* mapped, int64_t* split_slot, int64_t* n_spilled);

/* 1 when the snapshot records in device memory are block-major by replay slot: the latest launch
 * from the initial state was a replay through the slot map that saved no state image (cl_rerun
 * of a mapped plan), on either exec kernel.  Engine-internal: every reader (CollectSnapshot,
 * checksums, counters, packed collects, instance hashes, statistics) handles both layouts. */
int cl_records_blocked(cl_sim* sim, int32_t* on);

/* Which exec kernel runs the program (engine-internal; results are identical):
 *   CL_ENGINE_AUTO   the instance-per-lane kernel, compiled at run time for this topology
 *                    (hipRTC), wherever the topology fits it (<= 16 nodes, every degree <= 4,
 *                    <= 16 snapshot ids); else -- or when run-time compilation fails -- the
 *                    node-parallel kernel
 *   CL_ENGINE_NODES  the node-parallel kernel (one lane per node)
 *   CL_ENGINE_LANES  the instance-per-lane kernel; CL_E_LIMIT where the topology does not fit
 * cl_exec_engine reports the kernel the most recent launch used (0 before any). */
#define CL_ENGINE_AUTO 0
#define CL_ENGINE_NODES 1
#define CL_ENGINE_LANES 2
int cl_set_exec_engine(cl_sim* sim, int32_t engine);
int cl_exec_engine(cl_sim* sim, int32_t* engine);
/* Replays (cl_rerun) of a planned program on the instance-per-lane kernels can run kernels
 * compiled for the topology and the program: the sends and snapshot starts as straight-line code
 * on their nodes' registers (engine-internal; results are identical).  Such a compile takes
 * seconds, once per program and process:
 *   CL_PROGRAM_AUTO  only for batches AUTO itself would put on the instance-per-lane kernels
 *                    (cl_engine.h kLanesAutoMinInstances, a topology degree of at least 2)
 *   CL_PROGRAM_OFF   never
 *   CL_PROGRAM_ON    for every replay of a planned program on those kernels
 * Programs over 128 sends and snapshot starts or 32 tick ops, first launches, flushes and resumed
 * launches always run the generic kernels; so does a program whose compile fails.
 * cl_exec_program_kernels: 1 when the most recent launch ran program-specialized kernels. */
#define CL_PROGRAM_AUTO 0
#define CL_PROGRAM_OFF 1
#define CL_PROGRAM_ON 2
int cl_set_program_kernels(cl_sim* sim, int32_t mode);
int cl_exec_program_kernels(cl_sim* sim, int32_t* on);
/* Run-time kernel compilations of this process so far and their total wall time. */
int cl_jit_stats(double* compile_ms, int64_t* compiles);
/* Compile the instance-per-lane kernels for this sim's topology and layout without loading
 * them (no device needed): CL_OK, or CL_E_LIMIT (the topology does not fit them) / CL_E_DEVICE
 * (compilation failed); the compiler log goes to log (log_cap bytes, may be NULL). */
int cl_lanes_compile_check(cl_sim* sim, double* compile_ms, char* log, int64_t log_cap);
/* The same for the kernels specialized on the sim's current program (every event issued so far,
 * as a replay would run it): *specialized = 1 and they are compiled, or 0 and nothing is -- the
 * program is over the cap and replays on the generic kernels. */
int cl_lanes_program_compile_check(cl_sim* sim, double* compile_ms, int32_t* specialized, char* log, int64_t log_cap);
/* *on = 1 when the program-specialized kernels of the latest launch -- or of the latest
 * cl_lanes_program_compile_check, if that came later -- were compiled for delay rows that hold
 * every draw the program can make (cl_delay_draws_needed): their broadcast guard has no row-end
 * test.  0 with shorter rows (a caller's schedule), and when no such kernels were used. */
int cl_exec_program_cover(cl_sim* sim, int32_t* on);

/* Test/benchmark aid (no reference counterpart): overwrite every result plane the exec
 * kernel writes -- node snapshot records, completion ticks, per-instance result rows,
 * final node tokens -- with the byte 0xA5 on the sim's stream, so that results read after
 * the next cl_rerun can only come from that launch.  No-op before the first execution. */
int cl_debug_poison_outputs(cl_sim* sim);

/* ---- topology queries (host only) ---------------------------------------- */
int cl_num_nodes(const cl_sim* sim, int32_t* n);
int cl_node_id(const cl_sim* sim, int32_t rank, const char** id); /* owned by sim */
int cl_num_channels(const cl_sim* sim, int32_t* n);
int cl_channel(const cl_sim* sim, int32_t ch, int32_t* src_rank, int32_t* dest_rank);
int cl_num_snapshots(const cl_sim* sim, int32_t* n);
int cl_num_instances(const cl_sim* sim, int64_t* n);
/* Delay draws per instance the current event program can consume (upper bound). */
int cl_delay_draws_needed(const cl_sim* sim, int64_t* draws);
/* Bytes of GPU memory the batch holds (after flush). */
int cl_device_bytes(const cl_sim* sim, int64_t* bytes);

/* ---- results (flush pending events first) -------------------------------- */
int cl_get_status(cl_sim* sim, int32_t* out /* [n_instances] */);
int cl_get_time(cl_sim* sim, int32_t* out /* [n_instances] */);
/* Final node tokens (checkTokens, test_common.go:298-302), rank order. */
int cl_node_tokens(cl_sim* sim, int64_t inst, int64_t* out /* [num_nodes] */);
/* Completion tick of snapshot sid in instance inst, -1 if not complete. */
int cl_snapshot_tick(cl_sim* sim, int32_t sid, int64_t inst, int32_t* tick);
/* CollectSnapshot (sim.go:134-173) of one instance: tokens[rank] = tokenMap, and the
 * recorded messages as a CSR over channels: messages of channel c are
 * msg_tokens[msg_offsets[c] .. msg_offsets[c+1]) in delivery order.  Returns
 * CL_E_NOT_COMPLETE if the snapshot has not completed in that instance; if msg_cap is
 * too small, offsets are still written and CL_E_LIMIT is returned. */
int cl_collect_snapshot(cl_sim* sim, int32_t sid, int64_t inst, int64_t* tokens,
                        int64_t* msg_offsets /* [num_channels + 1] */, int64_t* msg_tokens,
                        int64_t msg_cap);
/* Completion of snapshot sid over instances [inst_lo, inst_hi) -- the global
 * WaitGroup of sim.go:116-117,126-131 per instance: *n_complete = instances whose
 * snapshot has completed after every event issued so far (pending events are executed,
 * no tick is added).  Non-blocking apart from that execution. */
int cl_poll_snapshot(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, int64_t* n_complete);
/* The blocking side of CollectSnapshot (sim.go:137-140): wait until snapshot sid has
 * completed in every instance of [inst_lo, inst_hi).  The caller is a collector thread;
 * it is woken after each execution of the driver's events (cl_flush, queries) and after
 * every cl_tick / cl_drain, and re-checks (executing the pending events itself, so a
 * driver that only calls Tick() -- the reference's pattern -- completes the wait).  timeout_ms < 0 waits forever; on timeout returns CL_E_NOT_COMPLETE with
 * *n_complete (may be NULL) set.  It also returns CL_E_NOT_COMPLETE at once when every
 * instance of the range has either completed or stopped with a non-OK status (the
 * reference process would have exited at that log.Fatal; such an instance never
 * completes).  Never ticks. */
int cl_wait_snapshot(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, int64_t timeout_ms,
                     int64_t* n_complete);
/* CollectSnapshot (sim.go:134-173) of instances [inst_lo, inst_hi) at once:
 * tokens[(i - inst_lo) * N + rank] (-1 for an instance whose snapshot has not
 * completed, with complete[i - inst_lo] = 0; complete may be NULL); the recorded
 * messages as ONE CSR over (instance, channel): the messages of instance i on channel c
 * are msg_tokens[msg_offsets[r * C + c] .. msg_offsets[r * C + c + 1]), r = i - inst_lo,
 * msg_offsets has (inst_hi - inst_lo) * C + 1 entries.  CL_E_LIMIT (offsets still
 * written) if msg_cap is too small. */
int cl_collect_snapshot_range(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, int64_t* tokens,
                              int32_t* complete, int64_t* msg_offsets, int64_t* msg_tokens, int64_t msg_cap);
/* CollectSnapshot (sim.go:134-173; finalizeSnapshot node.go:188-195) of instances
 * [inst_lo, inst_hi), packed on the GPU: only the packed arrays cross PCIe.
 *   tokens[(i - inst_lo) * N + rank]    tokenMap (int32), -1 where not complete
 *   complete[i - inst_lo]                1 when the snapshot completed in instance i
 *   msg_offsets[r * C + c]               start of instance r's channel c (int64, (hi-lo)*C+1
 *                                        entries; channels in (src rank, dest rank) order)
 *   msg_tokens[...]                      recorded token counts (int32), delivery order
 * Any output pointer may be NULL; *n_msgs (may be NULL) = messages; CL_E_LIMIT (everything
 * else still written) when msg_cap is too small.  cl_collect_snapshot_range is the same
 * collect with int64 tokens and messages (widened on the host). */
int cl_collect_snapshot_packed(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, int32_t* tokens,
                               int32_t* complete, int64_t* msg_offsets, int32_t* msg_tokens, int64_t msg_cap,
                               int64_t* n_msgs);
/* cl_collect_snapshot_packed over an instance list: row r is instance insts[r], r < n, in any
 * order, duplicates allowed (msg_offsets has n * C + 1 entries).  An index outside
 * [0, n_instances) gives CL_E_INVALID before any device work; otherwise the same outputs, NULL-able
 * pointers and CL_E_LIMIT behaviour.  E.g. the representatives of cl_snapshot_census's classes. */
int cl_collect_snapshot_list(cl_sim* sim, int32_t sid, const int64_t* insts, int64_t n, int32_t* tokens,
                             int32_t* complete, int64_t* msg_offsets, int32_t* msg_tokens, int64_t msg_cap,
                             int64_t* n_msgs);
/* Device time of the latest packed collect's kernels (HIP events). */
int cl_collect_time(cl_sim* sim, double* device_ms);
/* Counters over instances (only_ok: restrict to CL_INST_OK instances). */
int cl_get_counters(cl_sim* sim, int32_t only_ok, int64_t* out /* [CL_NUM_COUNTERS] */);
/* Batch checksums computed on the GPU (see CL_SUM_*); all-reduce them across ranks. */
int cl_get_checksums(cl_sim* sim, int64_t* out /* [CL_NUM_SUMS] */);
/* Per-instance snapshot hashes of instances [lo, lo + n): the CL_SUM_SNAPSHOT_HASH term of each
 * instance (the sum over its completed snapshots of the content hash; 0 unless the instance is
 * CL_INST_OK), for instance-by-instance parity checks of a whole batch. */
int cl_instance_hashes(cl_sim* sim, int64_t lo, int64_t n, uint64_t* out);

/* ---- per-snapshot batch statistics (no reference counterpart: the batch is a Monte-Carlo
 * experiment over the delay streams, this is its distribution) ------------------------------
 * The sample of cl_snapshot_stats(sid, [inst_lo, inst_hi)) is every instance of the range with
 * status CL_INST_OK in which snapshot sid has completed (the instances CL_SUM_COMPLETED counts).
 * One reduction kernel reads the status, completion-tick and snapshot-record planes on the
 * device; only the result crosses PCIe.  `out` is one flat int64 array of three contiguous
 * sections, so ranks and sub-ranges merge with one SUM, one MIN and one MAX over three slices:
 *   SUM  instances (all of the range), ok, sample;
 *        tick_sum, tick_sumsq, tick_hist[tick_bins]   bin clamp(tick - tick_lo, 0, tick_bins - 1)
 *        msgs_sum, msgs_sumsq          recorded messages of an instance, over all channels
 *        inflight_sum, inflight_sumsq  recorded tokens of an instance (the in-flight part of the cut)
 *        node_sum[N], node_sumsq[N]    tokenMap entry per node, rank order
 *        ch_msgs_sum[C], ch_msgs_sumsq[C], ch_tok_sum[C], ch_tok_sumsq[C]   per channel (cl_channel order)
 *        ch_msg_hist[C][msg_bins]      bin min(recorded messages, msg_bins - 1)
 *   MIN  tick, msgs, inflight, node[N], ch_msgs[C], ch_tok[C]   (INT64_MAX on an empty sample)
 *   MAX  the same fields                                          (INT64_MIN on an empty sample)
 * Total words: 15 + tick_bins + 4 N + 8 C + C * msg_bins.  Everything is exact integer arithmetic
 * and independent of the grid, the record layout and the exec kernel; the sums of squares
 * accumulate modulo 2^64 (two's complement wrap-around; merge them with wrapping adds). */
#define CL_STATS_MAX_TICK_BINS 4096
#define CL_STATS_MAX_MSG_BINS 64
typedef struct {
  int32_t tick_lo;   /* completion tick of histogram bin 0 */
  int32_t tick_bins; /* 1 .. CL_STATS_MAX_TICK_BINS */
  int32_t msg_bins;  /* 1 .. CL_STATS_MAX_MSG_BINS */
} cl_stats_spec;
/* Offsets, in int64 words, of every field of `out` (array fields: their first word), the three
 * section bounds and the total; the first five fields restate the shape the layout is for. */
typedef struct {
  int64_t n_nodes, n_channels, tick_lo, tick_bins, msg_bins;
  int64_t total_words, sum_begin, sum_end, min_begin, min_end, max_begin, max_end;
  int64_t instances, ok, sample, tick_sum, tick_sumsq, tick_hist, msgs_sum, msgs_sumsq, inflight_sum,
      inflight_sumsq, node_sum, node_sumsq, ch_msgs_sum, ch_msgs_sumsq, ch_tok_sum, ch_tok_sumsq, ch_msg_hist;
  int64_t min_tick, min_msgs, min_inflight, min_node, min_ch_msgs, min_ch_tok;
  int64_t max_tick, max_msgs, max_inflight, max_node, max_ch_msgs, max_ch_tok;
} cl_stats_layout;
#define CL_STATS_LAYOUT_FIELDS 41
/* The layout for this sim's topology and a spec.  Host only, no device. */
int cl_stats_layout_of(const cl_sim* sim, const cl_stats_spec* spec, cl_stats_layout* out);
/* The statistics of snapshot sid over instances [inst_lo, inst_hi) into out[out_words].  Like
 * the other result queries it executes pending events and never adds a tick, holds the sim's
 * lock and waits for a split replay's second half.  Arguments are checked before any device
 * work: CL_E_INVALID (bad spec, sid or range out of bounds, NULL pointer), CL_E_STATE (no event
 * was ever issued: nothing has run), CL_E_LIMIT (out_words below the layout's total_words).
 * inst_lo == inst_hi is valid: the empty sample. */
int cl_snapshot_stats(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, const cl_stats_spec* spec,
                      int64_t* out, int64_t out_words);
/* Device time of the latest cl_snapshot_stats kernel(s) (HIP events), like cl_collect_time. */
int cl_stats_time(cl_sim* sim, double* device_ms);

/* ---- snapshot outcome census: the distinct global snapshots of a batch -----------------------
 * cl_snapshot_stats gives the marginal distributions; this is the joint one.  Over the same
 * sample (instances of [inst_lo, inst_hi) with status CL_INST_OK in which snapshot sid has
 * completed) the GPU groups the instances by the 64-bit snapshot content hash -- the value of
 * orc_snapshot_hash, the per-snapshot term of CL_SUM_SNAPSHOT_HASH -- and returns one
 * cl_census_class per distinct value.  Equality of snapshots here MEANS equality of that hash:
 * contents are not compared (the engine's parity checks rest on the same hash).  Every key value,
 * 0 and UINT64_MAX included, is a class.
 *   classes    ordered by count descending, then key ascending (unsigned); the first
 *              n_returned = min(n_classes, max_classes) are written
 *   class_of   (may be NULL) class_of[i - inst_lo] = index of instance i's class in that full
 *              order (not clamped to n_returned), -1 for instances outside the sample
 *   info       instances, ok, sample as in cl_snapshot_stats; n_classes = distinct keys
 * The result is a pure function of the records: it does not depend on the grid, on lds_slots, on
 * the record layout or on the exec kernel.  Only n_classes * 32 bytes cross PCIe (plus class_of
 * when asked for).  Like the other result queries the call executes pending events and never
 * adds a tick, holds the sim's lock and waits for a split replay's second half.  Arguments are
 * checked before any device work: CL_E_INVALID (bad spec, NULL info, NULL classes with
 * max_classes > 0, sid or range out of bounds), CL_E_STATE (no event was ever issued).
 * inst_lo == inst_hi is valid and gives an all-zero info. */
typedef struct {
  int64_t max_classes; /* entries of `classes` the caller provides, >= 0 */
  int32_t lds_slots;   /* per-workgroup LDS table: 0 = engine's choice; -1 = none (every sample instance
                          inserts into the global table); else a power of two in [16, 4096] */
} cl_census_spec;
typedef struct {       /* 32 bytes */
  uint64_t key;        /* the snapshot content hash: orc_snapshot_hash, the per-snapshot term of
                          CL_SUM_SNAPSHOT_HASH */
  int64_t count;       /* sample instances with this content */
  int64_t first_inst;  /* smallest instance index of the class (its representative) */
  int32_t min_tick, max_tick; /* completion ticks over the class */
} cl_census_class;
typedef struct { int64_t instances, ok, sample, n_classes, n_returned; } cl_census_info;
int cl_snapshot_census(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, const cl_census_spec* spec,
                       cl_census_class* classes /* [max_classes], NULL iff max_classes == 0 */,
                       int32_t* class_of /* [inst_hi - inst_lo] or NULL */, cl_census_info* info);
/* Device time of the latest cl_snapshot_census kernels (HIP events), like cl_stats_time. */
int cl_census_time(cl_sim* sim, double* device_ms);

/* ---- instance selection by snapshot predicate: which instances are those? --------------------
 * cl_snapshot_stats and cl_snapshot_census describe a batch; this call names the instances behind
 * a histogram bin, a tail or a class.  The query is a conjunction of at most CL_SELECT_MAX_CLAUSES
 * range clauses over the per-instance quantities the statistics reduce, evaluated on the GPU over
 * the record planes.  The universe is the sample of those two calls: the instances of
 * [inst_lo, inst_hi) with status CL_INST_OK in which snapshot sid has completed; instances, ok and
 * sample in `info` mean what they mean there.  An instance matches when every clause holds
 * (n_clauses == 0: the whole sample).  A clause holds when its field's value lies in [lo, hi], both
 * inclusive -- with CL_SEL_NOT, when it lies outside; lo > hi is the empty interval (with
 * CL_SEL_NOT it then matches everything).
 *   insts   the matches in ascending instance order, as absolute indices (not relative to
 *           inst_lo); with n_match > cap the first cap of them.  n_returned = min(n_match, cap);
 *           truncation is reported, not an error.  cap == 0 with insts == NULL only counts.
 *   ticks   (may be NULL) ticks[k] = completion tick of insts[k]
 * The result is a pure function of the records: it does not depend on the grid, the record layout
 * or the exec kernel.  Only info and n_returned * 8 bytes (12 with ticks) cross PCIe; the result
 * feeds cl_collect_snapshot_list.  Like the other result queries the call executes pending events
 * and never adds a tick, holds the sim's lock and waits for a split replay's second half.
 * Arguments are checked before any device work: CL_E_INVALID (NULL info; NULL clauses with
 * n_clauses > 0; n_clauses outside [0, CL_SELECT_MAX_CLAUSES]; an unknown field or flag bits;
 * non-zero reserved; index outside [0, N) for CL_SEL_NODE, outside [0, C) for CL_SEL_CH_*,
 * non-zero for the other fields; sid or the range out of bounds; cap < 0; NULL insts with
 * cap > 0), CL_E_STATE (no event was ever issued).  inst_lo == inst_hi is valid and gives an
 * all-zero info. */
#define CL_SEL_TICK      0  /* completion tick of sid */
#define CL_SEL_MSGS      1  /* recorded messages of the instance over all channels (stats "msgs") */
#define CL_SEL_INFLIGHT  2  /* recorded tokens of the instance over all channels (stats "inflight") */
#define CL_SEL_NODE      3  /* tokenMap entry of node rank `index` */
#define CL_SEL_CH_MSGS   4  /* recorded messages on channel `index` (cl_channel order) */
#define CL_SEL_CH_TOK    5  /* recorded tokens on channel `index` */
#define CL_SEL_KEY       6  /* snapshot content hash (the census key); lo/hi are uint64 bit patterns, compared unsigned */
#define CL_SEL_NOT       1  /* clause flag: the clause holds when the value is OUTSIDE [lo, hi] */
#define CL_SELECT_MAX_CLAUSES 8
typedef struct { int32_t field, index, flags, reserved; int64_t lo, hi; } cl_select_clause; /* 32 B */
typedef struct { int64_t instances, ok, sample, n_match, n_returned; } cl_select_info;
int cl_select_instances(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi,
                        const cl_select_clause* clauses, int32_t n_clauses,
                        int64_t* insts /* [cap] or NULL iff cap == 0 */, int32_t* ticks /* [cap] or NULL */,
                        int64_t cap, cl_select_info* info);
/* Device time of the latest cl_select_instances kernels, both stages (HIP events), like
 * cl_census_time.  cl_select_stage_times splits it: the evaluation of the clauses into the
 * verdict bitmap, and the bitmap's compaction (either pointer may be NULL). */
int cl_select_time(cl_sim* sim, double* device_ms);
int cl_select_stage_times(cl_sim* sim, double* evaluate_ms, double* compact_ms);
/* The bulk form of cl_snapshot_tick: out[i - inst_lo] = completion tick of snapshot sid in
 * instance i of [inst_lo, inst_hi), -1 = not complete.  One strided device-to-host copy; the same
 * flush and lock behaviour and argument checks as the result queries above. */
int cl_snapshot_ticks(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, int32_t* out /* [hi-lo], -1 = not complete */);

/* ---- instance sets: statistics, census and selection over a set of instances ------------------
 * The three calls above describe one snapshot id over an index range.  A cl_iset is a subset of
 * [0, n_instances) kept on the device as a bitmap (ceil(n_instances / 64) 64-bit words, bit
 * inst % 64 of word inst / 64; the bits at and above n_instances are always 0), so the answer of
 * one call can condition the next: the statistics of a census class, the completion ticks of the
 * instances in which a channel recorded a message, the outcomes of snapshot 4 among the runs in
 * which snapshot 0 finished late.  A set is made from select clauses or from an index list, sets
 * combine with each other, and the cl_*_in calls take one as a fourth condition of their sample.
 *
 * A set belongs to the sim it was made from and is only a set of indices: it stays valid across
 * cl_rerun, engine switches and both record layouts, and says nothing about a snapshot id -- a set
 * made from clauses on one sid may condition the analysis of another.  Its bitmap is allocated by
 * the first call that needs it on the device (a set made from a list before anything has run keeps
 * the list until then).  cl_iset_destroy frees a set; cl_sim_destroy frees the sets still alive,
 * whose handles are dead from then on.  Every call holds the lock of the set's sim, like the other
 * result queries.
 *
 * cl_iset_from_clauses  the arguments, argument checks and `info` of cl_select_instances without
 *     its output arrays: the set holds every match (there is no cap), info->n_returned is 0.
 * cl_iset_from_list     the listed instances; any order, duplicates allowed, n == 0 gives the empty
 *     set.  CL_E_INVALID, before any device work, for an index outside [0, n_instances), n < 0 or a
 *     NULL list with n > 0.
 * cl_iset_combine       dst = a AND b, a OR b, or a AND NOT b (CL_ISET_*); dst may be a or b.
 *     CL_E_INVALID for a NULL set, an unknown op, or sets of different sims.
 * cl_iset_count         *n = members in [inst_lo, inst_hi).
 * cl_iset_read          the members in [inst_lo, inst_hi) as ascending absolute indices, the first
 *     `cap` of them; *n_match counts them all, so truncation shows as n_match > cap, as in
 *     cl_select_instances.  cap == 0 with insts == NULL only counts.
 * cl_iset_time          device time of the kernels of the latest cl_iset_from_list (when it ran its
 *     scatter), cl_iset_combine, cl_iset_count or cl_iset_read (HIP events); cl_iset_from_clauses is
 *     timed by cl_select_time. */
#define CL_ISET_AND    0
#define CL_ISET_OR     1
#define CL_ISET_ANDNOT 2
typedef struct cl_iset cl_iset;
int cl_iset_from_clauses(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi,
                         const cl_select_clause* clauses, int32_t n_clauses, cl_iset** out, cl_select_info* info);
int cl_iset_from_list(cl_sim* sim, const int64_t* insts, int64_t n, cl_iset** out);
int cl_iset_combine(cl_iset* dst, const cl_iset* a, const cl_iset* b, int32_t op);
int cl_iset_count(cl_iset* set, int64_t inst_lo, int64_t inst_hi, int64_t* n);
int cl_iset_read(cl_iset* set, int64_t inst_lo, int64_t inst_hi, int64_t* insts /* [cap] or NULL iff cap == 0 */,
                 int64_t cap, int64_t* n_match);
int cl_iset_destroy(cl_iset* set);
int cl_iset_time(cl_sim* sim, double* device_ms);
/* The conditional forms of cl_snapshot_stats, cl_snapshot_census and cl_select_instances.  The
 * sample is the intersection of four conditions: member of `in`, in [inst_lo, inst_hi), status
 * CL_INST_OK, snapshot sid completed.  `instances` and `ok` still count the whole range, exactly as
 * the unconditional calls report them; `sample` and everything reduced from it -- sums, minima,
 * maxima, histograms, classes, class_of (-1 outside the sample), matches -- is conditional.  The
 * results have the shapes of the unconditional calls and merge like them.  With a set that holds
 * the whole batch a call returns byte for byte what the unconditional call returns.  CL_E_INVALID
 * for a NULL set or a set of another sim; every other check, the CL_E_STATE and CL_E_LIMIT
 * behaviour, the flush that adds no tick, the lock and the wait for a split replay's second half
 * are those of the unconditional call.  Their device times are read with cl_stats_time,
 * cl_census_time and cl_select_time. */
int cl_snapshot_stats_in(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, const cl_iset* in,
                         const cl_stats_spec* spec, int64_t* out, int64_t out_words);
int cl_snapshot_census_in(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, const cl_iset* in,
                          const cl_census_spec* spec, cl_census_class* classes, int32_t* class_of,
                          cl_census_info* info);
int cl_select_instances_in(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, const cl_iset* in,
                           const cl_select_clause* clauses, int32_t n_clauses, int64_t* insts, int32_t* ticks,
                           int64_t cap, cl_select_info* info);

/* ---- joint distribution of two snapshot quantities: how do they move together? ----------------
 * cl_snapshot_stats gives the marginal distribution of every quantity; this call gives the joint
 * distribution of two of them: a two-axis contingency table and the five joint moments, reduced on
 * the GPU in one sample walk (cl_crosstab.hip); only the 12 + bins_a * bins_b result words cross PCIe.
 *
 * Axis.  `field` is one of CL_SEL_TICK, CL_SEL_MSGS, CL_SEL_INFLIGHT, CL_SEL_NODE, CL_SEL_CH_MSGS,
 * CL_SEL_CH_TOK, with the meaning and the `index` rule it has in cl_select_clause (node rank,
 * channel number, 0 for the others), of snapshot `sid`; CL_SEL_KEY is refused (a hash is not
 * binnable).  The two axes may name different snapshot ids, the same one, or be identical.
 * Bin rule per axis:  bin(v) = v < lo ? 0 : min((uint64)(v - lo) / width, bins - 1)  -- the first and
 * the last bin take everything below and above; the subtraction happens only when v >= lo, so it
 * is exact for every int64 lo.  width >= 1, 1 <= bins <= CL_CROSSTAB_MAX_BINS,
 * bins_a * bins_b <= CL_CROSSTAB_MAX_CELLS.
 *
 * Sample.  The instances of [inst_lo, inst_hi) with status CL_INST_OK in which both a->sid and
 * b->sid completed (cl_snapshot_crosstab_in: that are also members of `in`).
 *
 * out[] (int64 words, out_words >= CL_XT_CELLS + bins_a * bins_b):
 *   CL_XT_INSTANCES  hi - lo                      CL_XT_OK      instances of the range with status OK
 *   CL_XT_SAMPLE     instances in the sample      (the first two count the range, as in every other call)
 *   CL_XT_SUM_A, CL_XT_SUM_B                      sums of the two values over the sample, exact int64
 *   CL_XT_SUM_AA, CL_XT_SUM_AB, CL_XT_SUM_BB      sums of a*a, a*b, b*b, accumulated modulo 2^64 (the
 *                                                 convention of cl_snapshot_stats' sums of squares)
 *   CL_XT_MIN_A, CL_XT_MIN_B                      minima (INT64_MAX on an empty sample)
 *   CL_XT_MAX_A, CL_XT_MAX_B                      maxima (INT64_MIN on an empty sample)
 *   CL_XT_CELLS + ia * bins_b + ib                instances of the sample with bin(a) == ia, bin(b) == ib
 * Ranks and sub-ranges merge with a wrapping SUM over words [0, 8) and [12, end), a MIN over
 * [8, 10) and a MAX over [10, 12).  All integer: the result does not depend on the grid, the
 * record layout or the exec kernel.
 *
 * Errors, all found before any device work, `out` untouched:
 *   CL_E_INVALID  a NULL sim, axis or out; a field outside CL_SEL_TICK .. CL_SEL_CH_TOK; an index out
 *                 of range for its field; bins outside [1, CL_CROSSTAB_MAX_BINS]; width < 1;
 *                 bins_a * bins_b > CL_CROSSTAB_MAX_CELLS; the instance range or either sid out of
 *                 bounds; (_in) a NULL set or a set of another sim
 *   CL_E_STATE    no event was ever issued
 *   CL_E_LIMIT    out_words < CL_XT_CELLS + bins_a * bins_b
 * inst_lo == inst_hi is the empty sample: zero counts, empty MIN / MAX, zero cells.  The flush that
 * adds no tick, the lock and the wait for a split replay's second half are those of
 * cl_snapshot_stats.  The scratch (the result words) is allocated on first use and counted by
 * cl_device_bytes.  cl_crosstab_time: device ms (HIP events) of the latest call's kernel;
 * CL_E_STATE before any call. */
#define CL_CROSSTAB_MAX_BINS  4096   /* per axis */
#define CL_CROSSTAB_MAX_CELLS 4096   /* bins_a * bins_b */
typedef struct { int32_t sid, field, index, bins; int64_t lo, width; } cl_crosstab_axis;   /* 32 B */
#define CL_XT_INSTANCES 0
#define CL_XT_OK        1
#define CL_XT_SAMPLE    2
#define CL_XT_SUM_A     3
#define CL_XT_SUM_B     4
#define CL_XT_SUM_AA    5
#define CL_XT_SUM_AB    6
#define CL_XT_SUM_BB    7
#define CL_XT_MIN_A     8
#define CL_XT_MIN_B     9
#define CL_XT_MAX_A     10
#define CL_XT_MAX_B     11
#define CL_XT_CELLS     12   /* cells[ia * bins_b + ib] follow */
int cl_snapshot_crosstab(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_crosstab_axis* a,
                         const cl_crosstab_axis* b, int64_t* out, int64_t out_words);
int cl_snapshot_crosstab_in(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_iset* in,
                            const cl_crosstab_axis* a, const cl_crosstab_axis* b, int64_t* out, int64_t out_words);
int cl_crosstab_time(cl_sim* sim, double* device_ms);

/* ---- group-by over a tuple of snapshot quantities: which outcomes occur, and together? --------
 * The census groups by the hash of one whole snapshot, the crosstab is joint over two binned
 * quantities; this call is GROUP BY (q1, ..., qk) over the quantities a select clause names, possibly
 * of different snapshot ids: exact, without bin edges, and sparse -- one row per tuple that occurs.
 *
 * Term.  (sid, field, index): `field` is one of CL_SEL_TICK .. CL_SEL_KEY with the meaning and the
 * `index` rule it has in cl_select_clause; the value of a CL_SEL_KEY term is the snapshot content
 * hash of `sid` (the census key), a uint64 bit pattern carried in an int64.  A call takes 1 to
 * CL_GROUPS_MAX_TERMS terms, in the caller's order; they may name different snapshot ids.
 *
 * Sample.  The instances of [inst_lo, inst_hi) with status CL_INST_OK in which the snapshot of every
 * term completed (cl_snapshot_groups_in: that are also members of `in`).  info->instances and
 * info->ok count the range, as everywhere else.
 *
 * Group.  The sample instances with the same tuple of values, keyed by a 64-bit hash:
 *   group_key(v[0 .. n)) = h, where h = 0x9E3779B97F4A7C15 ^ (uint64)n, then
 *                          h = mix64(h ^ (uint64)v[k]) for k = 0 .. n - 1   (cl_group_key; mix64 is
 *                          the finaliser of the snapshot content hash)
 * Equality of groups here MEANS equality of that key: tuples are not compared, as the census does
 * not compare snapshot contents.  Every key value, 0 and UINT64_MAX included, is a group.
 *   groups     one cl_census_class per group: key, count, first_inst (smallest instance), and the min
 *              and max completion tick OF terms[0].sid; ordered by count descending, then key
 *              ascending (unsigned); the first n_returned = min(n_classes, max_classes) are written
 *              (truncation is not an error; info->n_classes counts all groups)
 *   values     values[g * n_terms + k] = term k evaluated on the device for group g's first_inst
 *   group_of   (may be NULL) group_of[i - inst_lo] = index of instance i's group in the full order
 *              (not clamped to n_returned), -1 outside the sample
 *   spec       a cl_census_spec: max_classes = entries of `groups` and rows of `values`; lds_slots
 *              as in the census
 * The result does not depend on the grid, on lds_slots, on the record layout or on the exec kernel.
 * Staging: adjacent terms of one snapshot id share one staged tile of its records; a term list that
 * alternates between snapshot ids restages at every change, so keep the terms of one id together
 * where the order is free.  A list of CL_SEL_TICK terms reads no records.
 *
 * Errors, all found before any device work, nothing written:
 *   CL_E_INVALID  a NULL sim, term array, spec or info; n_terms outside [1, CL_GROUPS_MAX_TERMS]; a
 *                 field outside CL_SEL_TICK .. CL_SEL_KEY, a non-zero reserved, an index out of range
 *                 for its field; a bad spec (the census's rules); NULL groups or values with
 *                 max_classes > 0; the instance range or any term's sid out of bounds; (_in) a NULL
 *                 set or a set of another sim
 *   CL_E_LIMIT    more than 2^29 instances in the range
 *   CL_E_STATE    no event was ever issued
 * Like the other result queries the call executes pending events and never adds a tick, holds the
 * sim's lock and waits for a split replay's second half.  It shares the census's table scratch; the
 * buffers it adds (representatives, values) are counted by cl_device_bytes.  cl_groups_time: device
 * ms (HIP events) of the latest call's kernels, CL_E_STATE before any call or after an empty range.
 * cl_group_key: the key of a tuple, host only (no sim). */
#define CL_GROUPS_MAX_TERMS 8
typedef struct { int32_t sid, field, index, reserved; } cl_group_term;   /* 16 B */
int cl_snapshot_groups(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_group_term* terms, int32_t n_terms,
                       const cl_census_spec* spec, cl_census_class* groups /* [max_classes] */,
                       int64_t* values /* [max_classes][n_terms] */, int32_t* group_of /* [inst_hi - inst_lo] or NULL */,
                       cl_census_info* info);
int cl_snapshot_groups_in(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_iset* in, const cl_group_term* terms,
                          int32_t n_terms, const cl_census_spec* spec, cl_census_class* groups, int64_t* values,
                          int32_t* group_of, cl_census_info* info);
int cl_groups_time(cl_sim* sim, double* device_ms);
/* cl_groups_time split: stage_ms[5] = table initialisation, key pass, gather, group_of, values (0 for a
 * stage the latest call did not run); their sum is cl_groups_time. */
int cl_groups_stage_times(cl_sim* sim, double* stage_ms);
uint64_t cl_group_key(const int64_t* values, int32_t n);

/* ---- ordering a batch: top-k instances and exact quantiles of a snapshot quantity -------------
 * ORDER BY q LIMIT k, and the exact percentile of q, over the sample of one snapshot: "which 16
 * runs finished snapshot 0 last", "the median and p99 of the tokens in flight".  The list feeds
 * cl_collect_snapshot_list and cl_iset_from_list; cl_set_delay_go_seed_list(seed_base + insts)
 * re-runs exactly those instances.
 *
 * Term.  (sid, field, index) as a cl_group_term: the meaning and the `index` rule of
 * cl_select_clause.  The ordering calls (top-k, quantiles) take CL_SEL_TICK .. CL_SEL_CH_TOK and
 * refuse CL_SEL_KEY: a hash has no order worth asking for.  cl_snapshot_values takes CL_SEL_KEY
 * too, as the int64 bit pattern of the hash.
 *
 * Sample.  As everywhere: the instances of [inst_lo, inst_hi) with status CL_INST_OK in which
 * snapshot `sid` completed (the _in forms: that are also members of `in`).  info->instances and
 * info->ok count the range.
 *
 * Order.  Total and deterministic: ascending by (value, instance); with CL_ORDER_DESC by value
 * descending, instance still ascending.  Ties always go to the smaller instance index, whatever
 * the record layout, the slot map, the grid or the exec kernel.
 *
 * cl_snapshot_topk       the first n_returned = min(k, sample) instances of that order: insts[]
 *     absolute instance indices, values[] their values.  0 <= k <= CL_ORDER_MAX_K; k == 0 with NULL
 *     arrays only counts.
 * cl_snapshot_quantiles  n_q quantiles q[j] = num / den (den >= 1, 0 <= num <= den), 1 <= n_q <=
 *     CL_ORDER_MAX_QUANTILES, by the nearest-rank rule
 *         r = num == 0 ? 0 : ceil(num * sample / den) - 1      (the product exact, in 128 bits)
 *     values[j] = the value at position r of the ascending order, ranks[j] = r.  On an empty sample
 *     ranks[j] = -1, values is untouched and n_returned = 0; else n_returned = n_q.
 * cl_snapshot_values     the bulk form of cl_snapshot_ticks for any quantity: values[i - inst_lo] =
 *     the value for a sample instance and 0 for the others, in_sample[i - inst_lo] (may be NULL) 1 or 0.
 * The _in forms take the sample from the members of `in`; with a set holding the whole batch each
 * returns byte for byte what the unconditional call returns.
 *
 * Errors, all found before any device work, nothing written:
 *   CL_E_INVALID  a NULL sim, term or info; a field outside the call's range, an index out of range
 *                 for its field, a non-zero reserved; unknown flag bits; k outside [0, CL_ORDER_MAX_K];
 *                 NULL arrays with k > 0; a quantile with den < 1 or num outside [0, den], n_q outside
 *                 [1, CL_ORDER_MAX_QUANTILES], NULL q, values or ranks; the instance range or sid out
 *                 of bounds; (_in) a NULL set or a set of another sim
 *   CL_E_STATE    no event was ever issued
 *   CL_E_LIMIT    more than 2^29 instances in the range
 * inst_lo == inst_hi is the empty sample.  Like the other result queries the calls execute pending
 * events and never add a tick, hold the sim's lock and wait for a split replay's second half.  Their
 * scratch (the value plane, bitmaps, lists) is counted by cl_device_bytes.  Only the info, 16 *
 * n_returned bytes and a few words per digit pass cross to the host; cl_snapshot_values copies the
 * plane.  cl_order_time: device ms (HIP events) of the latest call's kernels; cl_order_stage_times:
 * ms[3] = the value walk, the select passes, the compaction (0 for a stage the call did not run);
 * CL_E_STATE before any call. */
#define CL_ORDER_DESC 1           /* flag: value descending (instance still ascending) */
#define CL_ORDER_MAX_K 65536
#define CL_ORDER_MAX_QUANTILES 64
typedef struct { int64_t instances, ok, sample, n_returned; } cl_order_info;
typedef struct { int64_t num, den; } cl_quantile;   /* 16 B */
int cl_snapshot_topk(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_group_term* term, int32_t flags,
                     int64_t k, int64_t* insts /* [k] or NULL iff k == 0 */, int64_t* values /* [k] likewise */,
                     cl_order_info* info);
int cl_snapshot_topk_in(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_iset* in, const cl_group_term* term,
                        int32_t flags, int64_t k, int64_t* insts, int64_t* values, cl_order_info* info);
int cl_snapshot_quantiles(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_group_term* term,
                          const cl_quantile* q, int32_t n_q, int64_t* values /* [n_q] */, int64_t* ranks /* [n_q] */,
                          cl_order_info* info);
int cl_snapshot_quantiles_in(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_iset* in,
                             const cl_group_term* term, const cl_quantile* q, int32_t n_q, int64_t* values,
                             int64_t* ranks, cl_order_info* info);
int cl_snapshot_values(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_group_term* term,
                       int64_t* values /* [hi-lo] */, uint8_t* in_sample /* [hi-lo] or NULL */);
int cl_snapshot_values_in(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_iset* in,
                          const cl_group_term* term, int64_t* values, uint8_t* in_sample);
int cl_order_time(cl_sim* sim, double* device_ms);
int cl_order_stage_times(cl_sim* sim, double* stage_ms /* [3] */);
/* Engine-internal test aid (needs a gfx950 device, CL_E_DEVICE otherwise), like
 * cl_go_delay_schedule_device: uploads a plane of n int64 values (in_sample[i] != 0: element i is in
 * the sample; NULL: all are) and runs exactly the select and compaction kernels of the calls above
 * on it, element index = instance.  Snapshot quantities are non-negative and below 2^31; this is the
 * only way to pin the kernels over the whole int64 range.  k, insts, vals as in cl_snapshot_topk
 * (*n_returned = min(k, sample)); q, n_q, q_values, q_ranks as in cl_snapshot_quantiles (n_q == 0: no
 * quantiles).  *device_ms (may be NULL): the kernels' time. */
int cl_order_plane_device(int32_t device, const int64_t* values, const uint8_t* in_sample, int64_t n, int32_t flags,
                          int64_t k, int64_t* insts, int64_t* vals, int64_t* n_returned, const cl_quantile* q,
                          int32_t n_q, int64_t* q_values, int64_t* q_ranks, double* device_ms);

/* ---- device event trace: the reference's debug Logger (logger.go:12-76) ---- */
/* One LogEvent (logger.go:18-23) per record, in the Logger's order.  Node ranks refer
 * to cl_node_id; `other` is the peer of a Sent/Received record (-1 for Start/End and
 * for a SendTokens to a dest without a link, node.go:121-124); tokens = nodeTokens. */
#define CL_LOG_SENT_TOKEN 0     /* SentMsgRecord, token (node.go:118) */
#define CL_LOG_SENT_MARKER 1    /* SentMsgRecord, marker (node.go:100) */
#define CL_LOG_RECV_TOKEN 2     /* ReceivedMsgRecord, token (sim.go:86) */
#define CL_LOG_RECV_MARKER 3    /* ReceivedMsgRecord, marker (sim.go:86) */
#define CL_LOG_START_SNAPSHOT 4 /* StartSnapshotRecord (sim.go:109) */
#define CL_LOG_END_SNAPSHOT 5   /* EndSnapshotRecord (sim.go:127) */
typedef struct {
  int32_t epoch;  /* Logger.events index = simulator time (sim.go:73, test_common.go:35) */
  int32_t kind;   /* CL_LOG_* */
  int32_t node;   /* LogEvent.nodeId (rank) */
  int32_t other;  /* dest of a Sent record, src of a Received record (rank), else -1 */
  int32_t data;   /* Message.data / snapshot id */
  int32_t tokens; /* LogEvent.nodeTokens */
} cl_log_event;
/* Record the Logger of instances [inst_lo, inst_lo + n_inst) with room for cap events
 * each (n_inst = 0: off, the default).  The next flush replays the program with the
 * trace build of the kernel. */
int cl_trace_enable(cl_sim* sim, int64_t inst_lo, int32_t n_inst, int32_t cap);
/* The Logger of one traced instance: *n_events records, the first min(cap, *n_events)
 * copied to out.  CL_E_LIMIT if the instance emitted more than the enabled capacity. */
int cl_trace_read(cl_sim* sim, int64_t inst, cl_log_event* out, int32_t cap, int32_t* n_events);

/* ---- delay-stream utility (host only, but for cl_go_delay_schedule_device) -- */
/* out[i*draws + k] = k-th rand.Intn(5) of rand.Seed(seed_base + i), i in [0, n). */
int cl_go_delay_schedule(int64_t seed_base, int64_t n, int64_t draws, uint8_t* out);
/* The same schedule from the closed form the device generator evaluates (csrc/cl_gorand.h), on
 * the host, no device needed: row i from seeds[i], or from seed_base + i when seeds is NULL.  A
 * row in which Intn(5) rejects an output is regenerated sequentially; *rejected_rows (may be
 * NULL) counts them. */
int cl_go_delay_schedule_jump(int64_t seed_base, const int64_t* seeds /* [n] or NULL */, int64_t n, int64_t draws,
                              uint8_t* out, int64_t* rejected_rows);
/* The device form (needs a gfx950 device, CL_E_DEVICE otherwise): the generator kernel writes
 * the plane in device memory with the engine's row padding, the host patches the rows that met
 * a rejection, and the plane is copied back to out[n * draws].  *patched_rows and *device_ms
 * (either may be NULL) as in cl_delay_gen_time.  Where the engine would take the host generator
 * (see cl_set_delay_generator: a shape the kernel does not take, or more than 4,096 rows that met
 * a rejection) the schedule comes from the host generator, and *patched_rows and *device_ms are 0. */
int cl_go_delay_schedule_device(int32_t device, int64_t seed_base, const int64_t* seeds /* [n] or NULL */, int64_t n,
                                int64_t draws, uint8_t* out, int64_t* patched_rows, double* device_ms);
/* Go math/rand Int63 / Intn restatement, for known-answer tests. */
int cl_go_int63(int64_t seed, int64_t n, int64_t* out);
int cl_go_intn(int64_t seed, int32_t bound, int64_t n, int32_t* out);

const char* cl_status_string(int32_t code);
const char* cl_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* CLSNAP_H */
