// cg_engine.h -- data layout shared by the graph engine's host runtime (cg_host.cpp)
// and its gfx950 kernels (cg_kernels.hip, cg_table.hip, cg_sparse.hip, cg_wave.hip, cg_profile.hip, cg_restore.hip).  DESIGN.md §10 draws the same layout.
//
// The graph engine runs ONE reference simulation over a large topology (BASELINE
// configs 4 and 5: 2^20-node regular digraph, 100k-node power-law graph with 4,096
// overlapping snapshots).  State lives in HBM, one entry per node / channel /
// (snapshot, node) / (snapshot, channel); each tick is a short sequence of grid-wide
// phases (pick, marker, expand, tally, scan, push) launched on one HIP stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cl_engine.h"  // mix64, status codes

namespace clsnap {

// Counter hash of the synthetic workloads: the same definition is restated in
// oracle/cl_oracle.c (orc_counter_hash) and tests/graphgen.py.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint64_t cg_hash(uint64_t seed, uint64_t a, uint64_t b) {
  const uint64_t h = mix64(seed ^ (a * 0x9E3779B97F4A7C15ULL));
  return mix64(h ^ (b * 0xD6E8FEB86659FD93ULL));
}

#if defined(__HIPCC__)
// Exclusive prefix of v over the threads of a workgroup of WAVES waves (thread order), and the
// workgroup's total.  lds: WAVES words, free again when the call returns.
template <int WAVES>
__device__ __forceinline__ uint64_t cg_block_prefix(uint64_t v, uint64_t* lds, uint64_t& total) {
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t inc = v;
#pragma unroll
  for (int32_t o = 1; o < 64; o <<= 1) {
    const uint64_t u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  uint64_t base = 0;
  total = 0;
#pragma unroll
  for (int32_t w = 0; w < WAVES; ++w) {
    const uint64_t x = lds[w];
    base += w < wave ? x : 0;
    total += x;
  }
  __syncthreads();
  return base + inc - v;
}
#endif

// FIFO entry (u64): lo32 = payload | kGMarker (token count or snapshot id, common.go:28-31),
// hi32 = receiveTime (sim.go:101).
constexpr uint32_t kGMarker = 0x80000000u;
constexpr uint32_t kGPayload = 0x7fffffffu;
// Recording cursor pair (u64) of (snapshot, in-channel): lo32 = begin, hi32 = end.
constexpr uint32_t kOpen = 0xffffffffu;
// Pending-count accumulator per (snapshot, node): creation adds kBig + links recorded,
// every later marker adds -1; the operation whose result is exactly kBig completes it.
constexpr int32_t kBig = 1 << 30;
constexpr int32_t kGMaxOutDegree = 64;  // non-empty out-channel bitmask per node (u64)
constexpr int32_t kGThreads = 256;      // threads (= nodes) per pick / marker / push block
constexpr int32_t kPushLanes = 4;       // k_push threads per node on small graphs
constexpr int32_t kGStatusHistOverflow = 6;
// A local snapshot created at a node of in-degree above this is expanded over its
// in-links by the whole k_push grid instead of by the creating lane.
constexpr int32_t kSmallIndeg = 64;
// Counters are kept as per-shard partial sums, cpart[shard * kNumCnt + counter]: every
// block adds its block-reduced totals to shard blockIdx % kParts, so no address sees
// more than a few atomics per kernel (a device-scope atomic on one word serializes at
// ~11 ns, MI355X_MICROARCH.md 'fanin').
constexpr int32_t kParts = 512;
enum GCnt : int32_t { GC_PEEK = 0, GC_POP_TOK, GC_POP_MK, GC_PUSH, GC_RECORDED, GC_COMPLETED, kNumCnt = 8 };

// A local snapshot created this tick at a node of in-degree > kSmallIndeg.
struct BigX {
  int32_t lo, hi;  // the node's in-CSR range
  int32_t s0;      // creating sender
  int32_t sid;
  int32_t karr;    // in-position of the arriving channel
  int32_t v;
  int32_t pad[2];
};

// A marker delivered this tick (k_pick -> k_marker).
struct MDel {
  int32_t s0, v, k, sid;  // sender, receiver, in-position of the channel, snapshot id
};

// A delivery that crosses devices in the partitioned mode: sender, receiver, in-position,
// payload word (kGMarker | sid, or token count).
struct PDel {
  int32_t s, v, k;
  uint32_t pay;
};

// Receiver-side channel state is one word per in-channel, tokcnt[k]: the tokens delivered on
// it so far (the recording cursor).  A local snapshot created this tick learns whether its
// in-channel k also delivered this tick, and what, from the SENDER's delivery word: sender
// s = in_src[k] popped on out-link in_oj[k] this tick iff pp[s].x == (t << 6) | in_oj[k],
// with payload pp[s].y (each sender delivers at most once per tick, sim.go:90).

constexpr uint32_t kEmpty = 0xffffffffu;  // head receiveTime word of an empty channel

// Per-(snapshot, node) state, one 16-byte record at sid * n + v: every marker handling
// (k_pick's creation bid, k_marker's creation or close, completion) touches one line instead
// of three arrays' (DESIGN.md §10).
struct alignas(16) SNode {
  unsigned long long W;  // creation key: (tick << 32) | creating sender (initiator: | 0xffffffff); ~0 = none
  int32_t cnt;           // pending accumulator (kBig + links recorded, -1 per later marker)
  int32_t stok;          // recorded node tokens (CreateLocalSnapshot, node.go:77)
};

// Device event trace of the graph engine (the reference's debug Logger, logger.go:12-76).
// One record per LogEvent, appended unordered; the host sorts them into the Logger's order
// by (epoch, order, sub) and restores LogEvent.nodeTokens by replaying the token changes the
// records themselves carry (cg_host.cpp cl_graph_trace_read).  Within an epoch (= simulator
// time, Logger.NewEpoch per Tick, sim.go:73) the Logger holds the tick's deliveries in
// sender rank order (sim.go:76-90), then the traffic sends of that step in node order, then
// the host events in program order.
enum : uint32_t { kTrTick = 0u, kTrSend = 1u, kTrHost = 2u };
constexpr uint32_t kTrSubEnd = 0xffffffffu;  // EndSnapshotRecord after the delivery's records
struct GTraceRec {
  int32_t epoch;
  uint32_t order;  // part (bits 31..30) | key: sender rank (tick), node rank (send), op index (host)
  uint32_t sub;    // 0 the delivery / send / start record, 1 + j the broadcast on out-link j, kTrSubEnd
  int32_t kind;    // TK_* (cl_engine.h) == CL_LOG_* (clsnap.h)
  int32_t node, other, data, pad;
};

enum GOpKind : int32_t { GOP_SEND = 1, GOP_SNAP = 2 };
struct GOp {
  int32_t kind, a, b;  // SEND: a = src rank, b = dest rank; SNAP: a = node rank, b = snapshot id
  int32_t n;           // SEND: tokens
};

// Device scalars of one run.
struct GScal {
  unsigned long long draw;  // next delay draw index (sim.go:101 call count)
  unsigned long long base_trig, base_send;  // this tick's draw bases (scan kernel)
  int32_t status;
  int32_t big_n;    // creations at high in-degree nodes this tick
  int32_t time;     // simulator time of the last tick that ran (sim.go:13)
  int32_t skip;     // the drain is over (or hung): launched drain ticks do nothing
  // device-side drain (test_common.go:123-137), evaluated by k_drain_ctl before each tick
  int32_t dphase;   // 0 waiting for completions, 1 the maxDelay+1 extra ticks, 2 done, 3 hang
  int32_t dleft;    // extra ticks left in phase 1
  int32_t dticks;   // ticks spent waiting
  int32_t dcur;     // first snapshot (< the drain's count) not yet complete
  // drain tick i runs with slot i & 1: its time and whether it runs were decided by the
  // previous tick's k_scan (k_drain_begin for the first), so no control kernel per tick
  int32_t dnow;      // time of the last drain tick decided to run
  int32_t dtime[2];
  int32_t dskip[2];
  // parallel send group (k_sg_check -> k_sg_apply)
  int32_t sg_first;              // position of the group's first failing send (INT32_MAX: none)
  int32_t sg_frozen;             // status at the group's start (k_sg_begin): the run was already frozen
  unsigned long long sg_draw0;   // the group's first draw index
  // partitioned mode: this device's tick totals (k_scan), global bases set by the host
  unsigned long long tot_trig, tot_send;
  // draws of the last tick whose k_push scanned its own bases (small graphs, no k_scan):
  // folded into `draw` by the next kernel that reads it (fold_draw), since every k_push block
  // reads `draw` while the tick runs
  unsigned long long draw_pend;
};
enum : int32_t { kDrainWait = 0, kDrainExtra = 1, kDrainDone = 2, kDrainHang = 3 };
constexpr int32_t kTimeFromDevice = -1;  // tick argument -1 - k: drain slot k (time, skip in GScal)
constexpr int32_t kDrainExtraTicks = 6;  // maxDelay + 1 (test_common.go:135-137)  // tick argument: read the tick's time from GScal.time

struct GParams {
  int32_t n, e;
  int32_t cap_log2;  // FIFO slots per channel = 1 << cap_log2
  int32_t s_cap;     // snapshot ids provisioned
  int32_t hist;      // token payload history slots per channel (0: unit payloads)
  int32_t delay_mode;  // 0 counter hash, 1 schedule
  uint64_t delay_seed;
  const uint8_t* sched;
  int64_t sched_len;
  uint64_t traffic_seed;
  uint32_t traffic_thresh;
  int64_t traffic_steps;
  int32_t n_pblocks;  // node blocks = ceil(n / kGThreads)
  int32_t blk_max_out;  // most out-channels of any node block (k_pick's LDS stage size)
  int32_t push_lanes;  // k_push threads per node: 0 = automatic, else forced (1 or kPushLanes)
  // topology (out-CSR channel order = (src rank, dest rank); in-CSR by (dest, src))
  const int32_t* out_off;   // [n+1]
  const int2* route;        // [e] channel c: (dest rank, in-CSR position)
  const int32_t* in_off;    // [n+1]
  const int32_t* in_src;    // [e] src rank at in-position k
  const uint8_t* in_oj;     // [e] out-link index at the sender of in-position k
  // node state
  int32_t* tokens;     // [n]
  // [n] the sender's delivery word: x = (tick << 6) | out-index popped in that tick, y = the
  // payload word of that pop (kGMarker | sid, or token count) -- one 8-byte entry, so a
  // creation's expansion reads one line per in-link's sender, not two
  int2* pp;
  int32_t* ltrig;      // [n] block-local exclusive prefix of triggered broadcasts (draws)
  int32_t* lsend;      // [n] block-local exclusive prefix of traffic sends
  long long* bsum;     // [2 * n_pblocks] block sums (trig, send) -> exclusive block offsets
  int32_t* crn;        // [n] snapshots created at the node this tick
  uint64_t* cre;       // [e] by in-CSR range of the node: (s0 << 32) | sid
  MDel* mlist;         // [n_pblocks * kGThreads] markers delivered, per pick block
  int32_t* mcnt;       // [n_pblocks]
  BigX* big;           // [n] creations at nodes of in-degree > kSmallIndeg this tick
  unsigned long long* cpart;  // [kParts * kNumCnt]
  // channel state
  // [e] lo32: receiveTime of the head packet (kEmpty if the queue is empty),
  //     hi32: ring head (lo16) | packets queued (hi16)
  uint64_t* hq;
  uint64_t* fifo;      // [e << cap_log2]
  uint32_t* tokcnt;    // [e] by in-position: tokens delivered on the channel so far
  uint32_t* histv;     // [e * hist] by in-position
  // snapshot state
  SNode* sn;           // [s_cap * n] per-(snapshot, node) record: creation key, pending accumulator, node tokens
  uint64_t* rec;       // [s_cap * e] by in-position: recording cursors
  int32_t* done;       // [s_cap] node groups complete (p.done[s_cap..] = gdone)
  int32_t* gdone;      // [s_cap * n_pblocks] nodes complete per group of kGThreads ranks
  int32_t* ctick;      // [s_cap] completion tick (-1)
  GScal* sc;
  const GOp* ops;
  // event trace (nullptr: off)
  GTraceRec* trace;
  uint32_t* trace_cnt;
  int32_t trace_cap;
  // Graph-partitioned mode: this device owns node ranks [part_lo, part_hi)
  // = pick blocks [blk_lo, blk_hi) (part_lo a multiple of kGThreads); whole-graph runs own
  // everything (part 0, [0, n)).  Arrays stay graph-sized; a device touches its own rows.
  int32_t part;
  int32_t part_lo, part_hi, blk_lo, blk_hi;
  int32_t pad1;
  PDel* outbox;          // [n] deliveries by owned senders to other devices' receivers
  uint32_t* out_n;       // [4] 0 outbox rows, 1 remote markers, 2 reports
  MDel* rmlist;          // [n] markers delivered to owned receivers by other devices' senders
  int2* reports;         // [n] (s0, outdeg) broadcasts triggered by other devices' senders
  int32_t* trigv;        // [n] broadcasts triggered by owned senders this tick (draws)
  unsigned long long* rdraw;  // [n] first draw of broadcasts triggered by other devices' senders
  // Device-resident exchange (cl_graph_part_dev_*): every exchange step moves
  // fixed-capacity buckets of 16-B rows between device buffers (one bucket per peer rank:
  // a header row {rows, 0, 0, 0} then bk_cap rows), so a tick needs no host round trip.
  // bk_cap bounds every bucket exactly (from the topology: the senders of one rank with a
  // channel into another's nodes).  Null bk_send: the host-staged exchange.
  int32_t bk_world, bk_rank;
  int32_t bk_span;     // node ranks per rank (owner(v) = v / bk_span)
  int32_t bk_cap;      // rows per bucket after its header
  int4* bk_send;       // [bk_world * (bk_cap + 1)] this rank's outgoing buckets
  const int4* bk_recv; // [bk_world * (bk_cap + 1)] bucket q: what rank q sent here
  uint32_t* bk_cnt;    // [bk_world] rows appended to each outgoing bucket
  long long* tot_send;        // [4] this rank's tick totals: triggers, sends, status
  const long long* tot_recv;  // [bk_world * 4] every rank's totals (all-gathered)
};
// Engine status of a device exchange bucket that overflowed its capacity (cannot happen with
// the topology bound; a guard, never a wrong answer).
constexpr int32_t kGStatusXchgOverflow = 7;

// Launchers (cg_kernels.hip); return hipError_t as int.
int cg_launch_reset(const GParams& p, const int32_t* init_tok, void* stream);
int cg_launch_tick(const GParams& p, int32_t t, void* stream);
// Drain (test_common.go:123-137) on the device: reset the drain state for the snapshots
// [0, n_before), then `ticks` x (k_drain_ctl + one tick whose time comes from GScal):
// k_drain_ctl decides on the device whether the tick runs (waiting, then maxDelay+1 extra
// ticks) or is skipped (drain over / hung), so the host checks only once per batch.
int cg_launch_drain_begin(const GParams& p, int32_t time, int32_t n_before, int64_t max_drain, void* stream);
int cg_launch_drain_ticks(const GParams& p, int32_t n_before, int64_t max_drain, int64_t first, int32_t ticks,
                          void* stream);
int cg_launch_drain_end(const GParams& p, void* stream);  // normal ticks run again
int cg_launch_sends(const GParams& p, int32_t t, void* stream);  // step-0 traffic
int cg_launch_hostops(const GParams& p, int32_t time, int32_t op_begin, int32_t op_count, void* stream);
// A run of host sends from pairwise distinct senders, in parallel: no send of the run
// changes another's sender balance or channel, so every send up to the first failing one
// (program order) executes at once with draw index d + position.
int cg_launch_sendgroup(const GParams& p, int32_t time, int32_t op_begin, int32_t op_count, void* stream);
// Partitioned mode, one tick = pick -> [exchange deliveries] -> receive -> [exchange
// reports] -> tally -> [allgather totals] -> bases -> [exchange replies] -> push.
int cg_launch_part_pick(const GParams& p, int32_t t, void* stream);
int cg_launch_part_receive(const GParams& p, int32_t t, const PDel* in, int32_t n_in, void* stream);
int cg_launch_part_tally(const GParams& p, int32_t step, const int2* rep, int32_t n_rep, void* stream);
int cg_launch_part_bases(const GParams& p, int64_t trig_before, int64_t trig_all, int64_t send_before,
                         int64_t send_all, const int32_t* s0, int32_t n, unsigned long long* draw0, void* stream);
int cg_launch_part_push(const GParams& p, int32_t t, int32_t step, const long long* replies, int32_t n, void* stream);
// The same tick with the device-resident exchange (GParams bk_*): pick -> seal deliveries ->
// [all-to-all] -> receive -> seal reports -> [all-to-all] -> tally -> [all-gather totals] ->
// bases + replies -> [all-to-all] -> push.  No host round trip.
int cg_launch_part_dev_seal(const GParams& p, void* stream);
int cg_launch_part_dev_pick(const GParams& p, int32_t t, void* stream);
int cg_launch_part_dev_receive(const GParams& p, int32_t t, void* stream);
int cg_launch_part_dev_tally(const GParams& p, int32_t step, void* stream);
int cg_launch_part_dev_bases(const GParams& p, void* stream);
int cg_launch_part_dev_push(const GParams& p, int32_t t, int32_t step, void* stream);
// Recorded copies on channels still recording at the end (out[0] += ...).
int cg_launch_finish(const GParams& p, int32_t n_sids, unsigned long long* out, void* stream);
// Batch checks (out zeroed by the caller, 3 + n_sids entries): out[0] final node tokens,
// out[1] in-flight token payloads, out[2] digest over completed snapshots,
// out[3 + sid] = snapshot tokens + recorded token payloads of completed snapshot sid.
int cg_launch_checks(const GParams& p, int32_t n_sids, unsigned long long* out, void* stream);
// Per-snapshot summary table (cg_table.hip): rows[i] = the 16 int64 of cl_graph_snap_row
// (clgraph.h) of snapshot sid_lo + i, i < n_sids, reduced over the owned nodes and the
// in-positions [k_lo, k_hi) of the channels into them; in_ch[k] = channel of in-position k.
// An init kernel and one grid-stride pass sized to n_cus compute units.
int cg_launch_table(const GParams& p, const int32_t* in_ch, int32_t k_lo, int32_t k_hi, int32_t sid_lo,
                    int32_t n_sids, long long* rows, int32_t n_cus, void* stream);
// Sparse packed collect (cg_sparse.hip) of the snapshots sid_lo + [0, n_sids): one entry per
// channel into an owned node with at least one recorded message of a completed snapshot, in
// (sid, channel) order.  cg_sparse_tiles(e) = channel tiles of a graph of e channels; the scan
// leaves in tb[n_sids * tiles] every tile's (entry, message) offset within its sid's row, in
// rtot[n_sids] the rows' totals, in row_off / row_moff[n_sids + 1] the rows' entry and message
// offsets (the last: the totals) and in complete[n_sids] whether each sid completed.  The write
// recomputes the tiles and stores channel and count of every entry, and, with msg != nullptr,
// the payloads from the history p.histv (p.hist > 0).  The token plane is out[n_sids][part_hi -
// part_lo]: recorded node tokens, a row of -1 for an incomplete sid.
int32_t cg_sparse_tiles(int64_t e);
int cg_launch_sparse_scan(const GParams& p, int32_t sid_lo, int32_t n_sids, ulonglong2* tb, ulonglong2* rtot,
                          long long* row_off, long long* row_moff, int32_t* complete, void* stream);
int cg_launch_sparse_write(const GParams& p, int32_t sid_lo, int32_t n_sids, const ulonglong2* tb,
                           const ulonglong2* rtot, const long long* row_off, const long long* row_moff,
                           int32_t* ent_channel, int32_t* ent_count, int32_t* msg, void* stream);
int cg_launch_sparse_tokens(const GParams& p, int32_t sid_lo, int32_t n_sids, int32_t* out, void* stream);
// Restore (cg_restore.hip).  The seed of a restored graph is the sparse collect of one sid kept
// on the device: one entry per channel with recorded messages, in channel order -- channel,
// count and moff, the exclusive prefix of the counts (= the draw index of the entry's first
// message) -- and the n_msgs payloads back to back (msgs == nullptr: every payload is 1).
struct GSeed {
  const int32_t* channel;  // [n_ent]
  const int32_t* count;    // [n_ent]
  const long long* moff;   // [n_ent]
  const int32_t* msgs;     // [n_msgs] or nullptr
  int64_t n_ent, n_msgs;
  int64_t max_count;       // the largest count
};
// cg_restore_tiles(n_ent) = words of scan scratch `tiles` the offsets need.  restore_offsets:
// moff = exclusive prefix of count (three passes: tile sums, one workgroup over the tiles, tile
// prefixes).  restore_reduce adds into out[4] (zeroed by the caller): [0] max count, [1] the
// payload sum, [2] payloads that differ from 1 (both stay 0 with msgs == nullptr), [3] the sum of tok[n].
int64_t cg_restore_tiles(int64_t n_ent);
int cg_launch_restore_offsets(const int32_t* count, int64_t n_ent, long long* moff, unsigned long long* tiles,
                              void* stream);
int cg_launch_restore_reduce(const int32_t* count, int64_t n_ent, const int32_t* msgs, int64_t n_msgs,
                             const int32_t* tok, int64_t n, unsigned long long* out, void* stream);
// The seed of a run, after cg_launch_reset and before anything else: message j of the seed
// (entry i, position q = j - moff[i]) goes to ring slot q of its channel with receiveTime
// receive_time(draw j, time 0); the entry's hq word gets head 0, its count and the receiveTime
// of position 0; the draw counter and GC_PUSH start at n_msgs.  A count above the ring's slots
// or (schedule mode) n_msgs above the schedule's length sets the status and queues nothing.
// No Logger record.  Any grid gives the same result.
int cg_launch_seed(const GParams& p, const GSeed& s, void* stream);
// The same for one device of a partitioned run (p.part_lo, p.part_hi), in the place of cg_launch_seed.
// seed_share writes share[4] = e_lo, e_hi, m_lo, m_hi: the entries whose channel is one of the owned
// nodes' out-channels [out_off[part_lo], out_off[part_hi]) -- a contiguous slice, the channels being
// ascending -- and their messages [moff[e_lo], moff[e_hi]) (moff[n_ent] = n_msgs).  seed_range reads
// the share from the device and queues those messages alone, each with its draw index among all
// n_msgs, so an owned channel gets the words cg_launch_seed writes for it; the draw counter starts
// at n_msgs on every device, GC_PUSH at m_hi - m_lo.  What cannot be seeded is judged on the whole
// seed as above, the same on every device.
int cg_launch_seed_share(const GParams& p, const GSeed& s, long long* share, void* stream);
int cg_launch_seed_range(const GParams& p, const GSeed& s, const long long* share, void* stream);
// The check of a seed's arrays that came from the host (cg_cut.hip; cl_graph_restore_cut), all on
// the device: tokens[n], channel / count[n_ent] and msgs[n_msgs] (nullptr: every payload is 1) of
// a graph of e channels.  *verdict (set to kCutClean by the caller) becomes the least
// (rule << 56) | index over the elements that break a rule, under any grid:
constexpr uint32_t kCutRuleTokens = 1;   // tokens[v] >= 0
constexpr uint32_t kCutRuleChannel = 2;  // 0 <= channel[i] < e, strictly ascending
constexpr uint32_t kCutRuleCount = 3;    // 1 <= count[i] <= kCutMaxCount
constexpr uint32_t kCutRulePayload = 4;  // msgs[j] <= kGPayload as unsigned (bit 31 is the marker's)
constexpr int32_t kCutMaxCount = 32768;  // the largest fifo_slots
constexpr uint64_t kCutClean = ~0ull;
int cg_launch_cut_check(const int32_t* tokens, int64_t n, const int32_t* channel, const int32_t* count, int64_t n_ent,
                        const int32_t* msgs, int64_t n_msgs, int32_t e, unsigned long long* verdict, int32_t n_cus,
                        void* stream);
// Marker-wave profile and marker tree (cg_wave.hip).  A row is rw = CL_WV_HEAD + lat_bins +
// depth_bins int64 words (clgraph.h).  wave_init leaves rows[n_rows] of the snapshots sid_lo + r at
// their identities with the origin set: org[r] is the origin itself (user != 0) or the rank of
// the initiator, whose record's creation tick is then the origin (-1: not an owned node).  wave
// reduces the owned nodes' records into the rows; with pairs != nullptr also the resolved
// {ancestor, hops} pairs [n_rows][n] (lo32 ancestor, hi32 hops) into the depth fields.  wave_link
// writes the guarded first link of every pair, wave_jump runs one pointer-doubling round in place
// and stores 1 to *changed if a pair moved.  wave_pack turns the records of the owned ranks into
// the int32 planes parent / tick [n_rows][part_hi - part_lo] (tick may be null).
int cg_launch_wave_init(const GParams& p, const long long* org, int32_t user, int32_t sid_lo, int32_t n_rows, int32_t rw,
                        long long* rows, void* stream);
int cg_launch_wave(const GParams& p, int32_t sid_lo, int32_t n_rows, int32_t rw, int32_t lat_bins, int32_t lat_width,
                   int32_t depth_bins, int32_t user, const unsigned long long* pairs, long long* rows, int32_t n_cus,
                   void* stream);
int cg_launch_wave_link(const GParams& p, int32_t sid_lo, int32_t n_rows, unsigned long long* pairs, void* stream);
int cg_launch_wave_jump(const GParams& p, int32_t n_rows, unsigned long long* pairs, int32_t* changed, void* stream);
int cg_launch_wave_pack(const GParams& p, int32_t sid_lo, int32_t n_rows, int32_t* parent, int32_t* tick, void* stream);
// Node and channel profile over the used snapshots of sid_lo + [0, ns) (cg_profile.hip; clgraph.h
// cl_graph_snapshot_profile draws the head, the node rows and the entries).  The scratch of a call:
struct GProfile {
  int32_t* list;            // [ns] the used rows, ascending; head[CL_PF_N_USED] of them
  int32_t* used;            // [ns] 1 / 0 per row
  long long* org;           // [ns] the origin of every row
  long long* head;          // [CL_PF_HEAD + msg_bins]
  unsigned long long* acc;  // [4][k_hi - k_lo] per owned in-position: msgs, tokens, (peak << 32 | ~row), snaps
  long long* rows;          // [(part_hi - part_lo) * kProfileNodeWords] the node rows (the node pass only)
  unsigned long long* tiles;  // [cg_profile_tiles(e)] entries of the channel tiles before each tile
};
constexpr int32_t kProfileNodeWords = 8;   // CL_PF_NODE_WORDS
constexpr int32_t kProfileMaxBins = 1024;  // CL_GRAPH_PROFILE_MAX_BINS
constexpr int32_t kProfileEntryBytes = 32;
// The segmented sum of a node's in-channels (k_profile_in) by in-degree: up to kProfileLaneDeg the
// node's own lane walks the range, up to kProfileWaveDeg a wave does, above it the workgroup.
constexpr int32_t kProfileLaneDeg = 8;
constexpr int32_t kProfileWaveDeg = 256;
// profile_reduce: the used list (use[ns] or nullptr; org_in[ns] the origins with user != 0, else the
// initiators' ranks), the channel pass over the in-positions [k_lo, k_hi) in `slices` slices of the
// used list (0: automatic), then the head's sums, maxima and histogram and the tiles' entry
// offsets with head[CL_PF_ENTRIES] their total.  profile_nodes: the node pass and the in-channel
// sums into s.rows.  profile_fill: the entries (32 bytes each) in ascending channel order.  The
// host fills the head words that need no device.  Any grid and any slice count give the same result.
int32_t cg_profile_tiles(int64_t e);
int cg_launch_profile_reduce(const GParams& p, int32_t k_lo, int32_t k_hi, int32_t sid_lo, int32_t ns,
                             const int32_t* use, const long long* org_in, int32_t user, int32_t slices, int32_t min_msgs,
                             int32_t bins, int32_t width, const GProfile& s, int32_t n_cus, void* stream);
int cg_launch_profile_nodes(const GParams& p, int32_t k_lo, int32_t k_hi, int32_t sid_lo, int32_t ns, int32_t slices,
                            const GProfile& s, int32_t n_cus, void* stream);
int cg_launch_profile_fill(const GParams& p, int32_t k_lo, int32_t k_hi, int32_t sid_lo, int32_t min_msgs,
                           const GProfile& s, void* entries, void* stream);

}  // namespace clsnap
