// cl_analytics.h -- the batch analytics of the batch engine: what their kernels (cl_stats.hip, cl_order.hip,
// cl_census.hip, cl_select.hip, cl_iset.hip, cl_crosstab.hip, cl_groups.hip) and their host layer
// (cl_analytics.cpp) share.  Declarations and host-and-device inline functions only; the device
// code of the sample walk is cl_sample.h, of a snapshot quantity cl_quantity.h.  No exec kernel
// uses any of it, so it is not part of cl_engine.h, which travels inside the library and is
// compiled into the run-time lanes kernel of every topology.
#pragma once
#include "cl_engine.h"

#if defined(__HIPCC__)
#define ANALYTICS_HD __host__ __device__
#else
#define ANALYTICS_HD
#endif

namespace clsnap {

// ---- per-snapshot batch statistics (cl_stats.hip; include/clsnap.h cl_snapshot_stats) ----------
// Offsets, in int64 words, of every field of the flat result: mirrors cl_stats_layout field by
// field (cl_analytics.cpp asserts the sizes agree).
struct StatsLayout {
  int64_t n_nodes, n_channels, tick_lo, tick_bins, msg_bins;
  int64_t total_words, sum_begin, sum_end, min_begin, min_end, max_begin, max_end;
  int64_t instances, ok, sample, tick_sum, tick_sumsq, tick_hist, msgs_sum, msgs_sumsq, inflight_sum,
      inflight_sumsq, node_sum, node_sumsq, ch_msgs_sum, ch_msgs_sumsq, ch_tok_sum, ch_tok_sumsq, ch_msg_hist;
  int64_t min_tick, min_msgs, min_inflight, min_node, min_ch_msgs, min_ch_tok;
  int64_t max_tick, max_msgs, max_inflight, max_node, max_ch_msgs, max_ch_tok;
};
inline StatsLayout stats_layout(int64_t N, int64_t C, int64_t tick_lo, int64_t T, int64_t M) {
  StatsLayout L{};
  L.n_nodes = N, L.n_channels = C, L.tick_lo = tick_lo, L.tick_bins = T, L.msg_bins = M;
  int64_t o = 0;
  auto take = [&o](int64_t n) { const int64_t at = o; o += n; return at; };
  L.sum_begin = o;
  L.instances = take(1), L.ok = take(1), L.sample = take(1);
  L.tick_sum = take(1), L.tick_sumsq = take(1), L.tick_hist = take(T);
  L.msgs_sum = take(1), L.msgs_sumsq = take(1), L.inflight_sum = take(1), L.inflight_sumsq = take(1);
  L.node_sum = take(N), L.node_sumsq = take(N);
  L.ch_msgs_sum = take(C), L.ch_msgs_sumsq = take(C), L.ch_tok_sum = take(C), L.ch_tok_sumsq = take(C);
  L.ch_msg_hist = take(C * M);
  L.sum_end = L.min_begin = o;
  L.min_tick = take(1), L.min_msgs = take(1), L.min_inflight = take(1);
  L.min_node = take(N), L.min_ch_msgs = take(C), L.min_ch_tok = take(C);
  L.min_end = L.max_begin = o;
  L.max_tick = take(1), L.max_msgs = take(1), L.max_inflight = take(1);
  L.max_node = take(N), L.max_ch_msgs = take(C), L.max_ch_tok = take(C);
  L.max_end = L.total_words = o;
  return L;
}

// The statistics kernel walks the records in tiles of 64 record slots x one chunk of record
// words, staged in LDS.  A chunk is at most kStatsChunkWords words of every instance: whole node
// records (rw <= kStatsChunkWords) or a piece of one node's record.  Chunk i covers the words
// [word0, word0 + nv * kw) of an instance's N * rw record words.
constexpr int32_t kStatsChunkWords = 32;
constexpr int32_t kStatsThreads = 256;
// LDS budget of one statistics workgroup (dynamic LDS, no opt-in needed; at least two workgroups
// share a CU's 160 KB, more when the pass needs less): the staging tiles of its 4 waves, the tick histogram, and per record word of
// the pass 8 int64 accumulators and msg_bins histogram counters.  Topologies whose N * rw
// words do not fit run as several passes over chunk ranges (cl_analytics.cpp stats()).
constexpr int32_t kStatsLdsBytes = 64 * 1024;
constexpr int32_t kStatsStageWords = kWave * (kStatsChunkWords + 1);  // per wave, rows padded odd
constexpr int32_t kStatsScalars = 16;                                  // int64 words (15 used)
struct StatsChunk {
  int32_t v0, nv, k0, kw;
};
ANALYTICS_HD inline int32_t stats_chunks(int32_t n_nodes, int32_t rw) {
  if (rw <= kStatsChunkWords) {
    const int32_t g = kStatsChunkWords / rw;
    return (n_nodes + g - 1) / g;
  }
  return n_nodes * ((rw + kStatsChunkWords - 1) / kStatsChunkWords);
}
ANALYTICS_HD inline StatsChunk stats_chunk(int32_t n_nodes, int32_t rw, int32_t i) {
  StatsChunk c;
  if (rw <= kStatsChunkWords) {
    const int32_t g = kStatsChunkWords / rw;
    c.v0 = i * g;
    c.nv = n_nodes - c.v0 < g ? n_nodes - c.v0 : g;
    c.k0 = 0;
    c.kw = rw;
  } else {
    const int32_t pieces = (rw + kStatsChunkWords - 1) / kStatsChunkWords;
    c.v0 = i / pieces;
    c.nv = 1;
    c.k0 = (i % pieces) * kStatsChunkWords;
    c.kw = rw - c.k0 < kStatsChunkWords ? rw - c.k0 : kStatsChunkWords;
  }
  return c;
}
// Record words a pass may accumulate within the LDS budget (>= kStatsChunkWords for every legal
// spec: 4096 tick bins, 64 message bins leave 47).
inline int32_t stats_pass_words(int32_t tick_bins, int32_t msg_bins) {
  const int32_t fixed = kWavesPerBlock * kStatsStageWords * 4 + tick_bins * 4 + kStatsScalars * 8;
  return (kStatsLdsBytes - fixed) / (8 * 8 + msg_bins * 4);
}
// LDS bytes of a workgroup whose pass accumulates acc_words record words.
inline int32_t stats_lds_bytes(int32_t acc_words, int32_t tick_bins, int32_t msg_bins) {
  return kWavesPerBlock * kStatsStageWords * 4 + tick_bins * 4 + kStatsScalars * 8 + acc_words * (8 * 8 + msg_bins * 4);
}
// Workgroups per CU the grid is sized for: what the CU's LDS holds of them, at most 8 (32 waves).
inline int32_t stats_blocks_per_cu(int32_t lds_bytes) {
  const int32_t b = kMaxLdsBytes / (lds_bytes > 0 ? lds_bytes : 1);
  return b < 1 ? 1 : b > 8 ? 8 : b;
}

// The sample of the analytics calls (statistics, census, select) and the planes their kernels walk
// for it: the instances of [lo, hi) with status OK in which snapshot `sid` completed -- and, for the
// conditional calls (cl_*_in), that are members of the instance set `where`.  The walk itself is
// cl_sample.h's.
struct SampleParams {
  int32_t n_nodes, n_ch, s_cap, rw, sid;
  int64_t n_inst, stride;
  int64_t lo, hi;            // the sample's instance range
  int64_t tile_lo, tile_hi;  // 64-slot tiles to walk (instance-major: those overlapping [lo, hi))
  const int32_t* regs;
  const int32_t* snap_tick;
  const uint32_t* snap_nod;
  int32_t blocked;           // records block-major by slot (rec_word)
  const int32_t* inst_map;   // slot -> instance of a block-major replay (nullptr: identity)
  // An instance set's bitmap (cl_iset: bit inst & 63 of word inst >> 6, stride / 64 words): only its
  // members are in the sample; the instances / OK counters still count the range.  nullptr: no filter.
  const unsigned long long* where;
};
// The tables next to the records: what a record's channel words mean.
struct RecordTables {
  const int32_t* ch_slot;     // [C] record word of channel c
  const int32_t* hist_off;    // [C + 1]
  const int32_t* hist_val;    // the channels' token histories, channel c from hist_off[c]
  const long long* hist_pre;  // their int64 prefix sums: channel c at hist_off[c] + c
};
// Census, select, crosstab and group-by stage records of at most this many words per instance in
// LDS tile by tile, as one chunk (address-ordered loads, cl_sample.h stage_tile); longer ones are
// read word by word by the instance's lane.  The host sets a call's `staged` from sample_staged;
// its launcher refuses one that staged_ok does not admit (the tile has no room for the record).
constexpr int32_t kCensusStageWords = kStatsChunkWords;
inline int32_t sample_staged(const SampleParams& s) { return s.n_nodes * s.rw <= kCensusStageWords ? 1 : 0; }
inline bool staged_ok(const SampleParams& s, int32_t staged) { return !staged || sample_staged(s); }

struct StatsParams {
  SampleParams s;
  RecordTables tab;
  const int32_t* word_ch;    // [N * rw] record word -> channel, -2 token word, -1 padding
  int32_t chunk_lo, chunk_hi;  // chunks whose words this pass accumulates
  int32_t totals;              // this pass also takes the counts, tick, msgs and inflight
  int32_t acc_words;           // record words of the pass (LDS accumulator rows)
  StatsLayout lay;
  long long* out;  // [lay.total_words], initialised by the host (0 / INT64_MAX / INT64_MIN)
};
int launch_stats(const StatsParams& p, int32_t blocks, void* stream);

// ---- snapshot outcome census (cl_census.hip; include/clsnap.h cl_snapshot_census) --------------
// A group-by of the snapshot content hash over the sample of cl_snapshot_stats.  One entry of the
// global open-addressing table, and of the compacted class array (the layout of cl_census_class).
struct CensusEntry {
  unsigned long long key;
  unsigned long long count;  // (the class's rank, once the host has sorted: cl_census_rank)
  long long first;           // smallest instance of the class
  int32_t min_tick, max_tick;
};
// The table's "empty" marker.  A snapshot whose key has this value is a class like any other: it
// bypasses the hashed slots and lives in the extra entry table[slots] (CensusParams::empty_key).
constexpr unsigned long long kCensusEmptyKey = ~0ULL;
constexpr int32_t kCensusThreads = 256;
constexpr int32_t kCensusMinLdsSlots = 16, kCensusMaxLdsSlots = 4096;
// The engine's choice of workgroup table: with the staging tiles it stays below 64 KB of LDS, so
// two workgroups and more share a CU (the scenarios measured have 2 .. 413 classes).
constexpr int32_t kCensusAutoLdsSlots = 1024;
// Probes before an LDS insert gives up and goes to the global table (a full or crowded table).
constexpr int32_t kCensusLdsProbes = 16;
constexpr int32_t kCensusLdsEntryBytes = 8 + 8 + 4 + 4 + 4;  // key, first, count, min tick, max tick
inline int32_t census_lds_bytes(int32_t lds_slots, bool staged) {
  return lds_slots * kCensusLdsEntryBytes + 4 * 8 + (staged ? kWavesPerBlock * kStatsStageWords * 4 : 0);
}
struct CensusParams {
  SampleParams s;
  RecordTables tab;
  int32_t lds_slots;         // workgroup table entries (a power of two), 0: none
  int32_t staged;            // sample_staged(s): records staged in LDS
  unsigned long long empty_key;
  CensusEntry* table;        // [slots + 1], initialised by launch_census_init
  int64_t slots;             // a power of two >= 2 * (hi - lo)
  uint32_t* list;            // [hi - lo] table slots in the order they were claimed
  unsigned long long* info;  // instances, ok, sample, n_classes
  unsigned long long* keys;  // [hi - lo] each sample instance's key, or nullptr
  int32_t* class_of;         // [hi - lo] 0 for sample instances, -1 for the others (with keys)
};
int launch_census_init(const CensusParams& p, void* stream);
int launch_census_keys(const CensusParams& p, int32_t blocks, void* stream);
// out[j] = table[list[j]], j < n
int launch_census_gather(const CensusParams& p, int64_t n, CensusEntry* out, void* stream);
// table[list[j]].count = rank[j], j < n; then class_of[i] = rank of keys[i]'s class
int launch_census_class_of(const CensusParams& p, int64_t n, const int32_t* rank, void* stream);

// ---- a quantity of a snapshot (cl_quantity.h; include/clsnap.h CL_SEL_*) ------------------------
// What a select clause, a crosstab axis and a group term name as (sid, field, index): of snapshot
// `sid` of an instance, its completion tick, its totals of recorded messages and tokens, the
// tokenMap entry of node `index`, the recorded messages or tokens of channel `index`, or the
// census key.  The value is an int64 (the key: its bit pattern); cl_quantity.h evaluates it.
enum : int32_t {
  SEL_TICK = 0, SEL_MSGS = 1, SEL_INFLIGHT = 2, SEL_NODE = 3, SEL_CH_MSGS = 4, SEL_CH_TOK = 5, SEL_KEY = 6,
  SEL_NUM_FIELDS = 7,
};
// Whether (field, index) names a quantity of a topology of n_nodes nodes and n_ch channels, of the
// fields up to max_field (SEL_KEY; SEL_CH_TOK where a hash is no use: it is not binnable).
ANALYTICS_HD inline bool quantity_ok(int32_t field, int32_t index, int32_t max_field, int64_t n_nodes, int64_t n_ch) {
  if (field < 0 || field > max_field) return false;
  const int64_t bound = field == SEL_NODE ? n_nodes : field == SEL_CH_MSGS || field == SEL_CH_TOK ? n_ch : 1;
  return index >= 0 && index < bound;
}

// ---- instance selection by snapshot predicate (cl_select.hip; include/clsnap.h cl_select_instances) ----
// A conjunction of range clauses over snapshot quantities, evaluated over the sample of
// cl_snapshot_stats; the matches come back as ascending instance indices.
constexpr int32_t kSelNot = 1;
constexpr int32_t kSelMaxClauses = 8;
constexpr int32_t kSelThreads = 256;
// Words (64 verdict bits each) one workgroup of the compaction counts and fills: one per thread.
constexpr int32_t kSelBlockWords = kSelThreads;
struct SelectClause {  // the layout of cl_select_clause
  int32_t field, index, flags, reserved;
  int64_t lo, hi;
};
struct SelectParams {
  SampleParams s;
  RecordTables tab;
  int32_t staged;            // sample_staged(s): records staged in LDS
  int32_t n_clauses;
  int32_t need_records;      // a clause reads the records (any field but SEL_TICK)
  int32_t need_totals;       // a clause names SEL_MSGS or SEL_INFLIGHT
  int32_t need_key;          // a clause names SEL_KEY
  SelectClause clause[kSelMaxClauses];
  // Verdict bitmap: bit (inst - base) & 63 of word (inst - base) >> 6, base = lo rounded down to a
  // multiple of 64 (so an instance-major tile is one word).  Block-major: zeroed before the pass.
  int64_t base, words;
  unsigned long long* bitmap;  // [words]
  unsigned long long* info;    // instances, ok, sample, n_match
  // compaction: block b counts / fills words [b * kSelBlockWords, ...)
  long long* bsum;             // [ceil(words / kSelBlockWords)] block totals -> exclusive prefix
  int64_t cap;                 // entries of out (and ticks) the fill may write
  long long* out;              // [cap] matching instances, ascending
  int32_t* ticks;              // [cap] their completion ticks, or nullptr
};
inline int32_t select_lds_bytes(bool staged) {
  return 4 * 8 + (staged ? kWavesPerBlock * kStatsStageWords * 4 : 0);
}
int launch_select_eval(const SelectParams& p, int32_t blocks, void* stream);
// count + scan (n_match left in p.info[3]), then the fill of the first p.cap matches
int launch_select_compact(const SelectParams& p, void* stream);

// ---- device-resident instance sets (cl_iset.hip; include/clsnap.h cl_iset) ----------------------
// A subset of [0, n_instances) as a bitmap: bit inst & 63 of word inst >> 6, stride / 64 words, the
// bits at and above n_instances 0.  The analytics kernels filter on it (SampleParams::where).
enum : int32_t { ISET_AND = 0, ISET_OR = 1, ISET_ANDNOT = 2, ISET_NUM_OPS = 3 };
constexpr int32_t kIsetThreads = 256;
// bits[list[r] >> 6] |= 1 << (list[r] & 63), r < n, into a zeroed bitmap (entries outside
// [0, n_inst) are skipped: the host has refused them before)
int launch_iset_scatter(const long long* list, int64_t n, int64_t n_inst, unsigned long long* bits, void* stream);
// dst[w] = a[w] op b[w], w < words (dst may be a or b)
int launch_iset_combine(unsigned long long* dst, const unsigned long long* a, const unsigned long long* b,
                        int32_t op, int64_t words, void* stream);
// The words that overlap [lo, hi), lo < hi, the first and the last masked to the range:
// dst[j] = src[lo / 64 + j] & mask, j < ceil(hi / 64) - lo / 64 -- what the selection's compaction
// (launch_select_compact, base = lo rounded down to 64) reads; the count adds their set bits to
// *count (zeroed by the host), one atomic per workgroup.
int launch_iset_clip(unsigned long long* dst, const unsigned long long* src, int64_t lo, int64_t hi, void* stream);
int launch_iset_count(const unsigned long long* src, int64_t lo, int64_t hi, unsigned long long* count, void* stream);

// ---- joint distribution of two snapshot quantities (cl_crosstab.hip; include/clsnap.h cl_snapshot_crosstab) ----
// A two-axis contingency table with the five joint moments over the instances of [lo, hi) with
// status OK in which the snapshots of both axes completed.  An axis is one of the quantities a
// select clause names (SEL_TICK .. SEL_CH_TOK) of one snapshot id, binned:
//   bin(v) = v < lo ? 0 : min((uint64)(v - lo) / width, bins - 1).
struct CrosstabAxis {  // the layout of cl_crosstab_axis
  int32_t sid, field, index, bins;
  int64_t lo, width;
};
constexpr int32_t kXtMaxBins = 4096;   // per axis
constexpr int32_t kXtMaxCells = 4096;  // bins_a * bins_b: 16 KB of 32-bit workgroup counters
constexpr int32_t kXtThreads = 256;
// Words of the flat int64 result (CL_XT_*): wrapping sums, then minima, maxima and the cells.
enum : int32_t {
  XT_INSTANCES = 0, XT_OK = 1, XT_SAMPLE = 2, XT_SUM_A = 3, XT_SUM_B = 4, XT_SUM_AA = 5, XT_SUM_AB = 6, XT_SUM_BB = 7,
  XT_MIN_A = 8, XT_MIN_B = 9, XT_MAX_A = 10, XT_MAX_B = 11, XT_CELLS = 12,
};
struct CrosstabParams {
  SampleParams s;            // the walk, and the planes of axis a's snapshot (s.sid == a.sid)
  CrosstabAxis a, b;
  RecordTables tab;
  int32_t staged;            // sample_staged(s): the planes an axis reads are staged in LDS
  long long* out;            // [XT_CELLS + a.bins * b.bins], initialised by the host (0 / INT64_MAX / INT64_MIN)
};
inline int32_t crosstab_lds_bytes(int32_t cells, bool staged) {
  return 16 * 8 + cells * 4 + (staged ? kWavesPerBlock * kStatsStageWords * 4 : 0);
}
int launch_crosstab(const CrosstabParams& p, int32_t blocks, void* stream);

// ---- group-by over a tuple of snapshot quantities (cl_groups.hip; include/clsnap.h cl_snapshot_groups) ----
// A term names a quantity (SEL_TICK .. SEL_KEY) of one snapshot id.  The sample is the instances of
// [lo, hi) with status OK in which the snapshot of every term completed; a group is the set of
// sample instances with the same tuple of term values, keyed by group_key().  Equality of groups
// MEANS equality of that 64-bit key: tuples are not compared.
constexpr int32_t kGroupsMaxTerms = 8;
struct GroupTerm {  // the layout of cl_group_term
  int32_t sid, field, index, reserved;
};

// group_key(v[0 .. n)): h = 0x9E3779B97F4A7C15 ^ n, then h = mix64(h ^ v[k]) in term order.
ANALYTICS_HD inline uint64_t group_key_seed(int32_t n) { return 0x9E3779B97F4A7C15ULL ^ (uint64_t)n; }
ANALYTICS_HD inline uint64_t group_key_fold(uint64_t h, int64_t v) { return mix64(h ^ (uint64_t)v); }

struct GroupsParams {
  // The walk, the planes of terms[0]'s snapshot (c.s.sid == term[0].sid), the record tables and the
  // census's table: the init / gather / rank / lookup kernels of cl_census.hip run on `c` as they are.
  CensusParams c;
  int32_t n_terms;
  GroupTerm term[kGroupsMaxTerms];
  // the distinct snapshot ids of term[1 ..] other than term[0].sid: a sample lane leaves the sample
  // when one of them did not complete
  int32_t n_other;
  int32_t other_sid[kGroupsMaxTerms];
  int32_t reads_records;  // a term reads the records (any field but SEL_TICK)
};
// The key pass: c.table / c.list / c.info filled as launch_census_keys fills them.
int launch_groups_keys(const GroupsParams& p, int32_t blocks, void* stream);
// values[g * n_terms + k] = term k of instance first[g], g < n.  rec_slot: instance -> record slot
// of block-major records (SimTables::rec_slot), nullptr when they are instance-major.
int launch_groups_values(const GroupsParams& p, const int32_t* rec_slot, const long long* first, int64_t n,
                         long long* values, void* stream);

// ---- ordering a batch: top-k and exact quantiles (cl_order.hip; include/clsnap.h cl_snapshot_topk) ----
// One quantity (SEL_TICK .. SEL_KEY) of one snapshot id over the sample of cl_snapshot_stats, as an
// int64 value plane [hi - lo] and a membership bitmap in the select bitmap's convention; a radix
// select on the plane finds the key at given order positions; the top-k is compacted with the
// select's compaction.  The order is ascending by (key, instance), key = order_key(value).
constexpr int32_t kOrderDesc = 1;
constexpr int64_t kOrderMaxK = 65536;
constexpr int32_t kOrderMaxPos = 64;     // order positions one select resolves (the quantiles of a call)
constexpr int32_t kOrderDigitBits = 8, kOrderBins = 1 << kOrderDigitBits;
constexpr int32_t kOrderThreads = 256;
// The value with its sign bit flipped, complemented for descending: unsigned order of the keys is
// the order asked for.  order_value is its inverse.
ANALYTICS_HD inline uint64_t order_key(int64_t v, int32_t desc) {
  const uint64_t k = (uint64_t)v ^ 0x8000000000000000ULL;
  return desc ? ~k : k;
}
ANALYTICS_HD inline int64_t order_value(uint64_t k, int32_t desc) {
  return (int64_t)((desc ? ~k : k) ^ 0x8000000000000000ULL);
}
// Words of the walk's info: the three counters, then the sample's min and max value (the host
// initialises them to INT64_MAX / INT64_MIN).
enum : int32_t { ORD_INSTANCES = 0, ORD_OK = 1, ORD_SAMPLE = 2, ORD_MIN = 3, ORD_MAX = 4, ORD_INFO_WORDS = 8 };
struct OrderWalkParams {
  SampleParams s;            // the walk of the term's snapshot (s.sid == term.sid)
  RecordTables tab;
  GroupTerm term;
  int32_t staged;            // sample_staged(s) and the term reads the records
  long long* plane;          // [hi - lo] value of instance lo + i (0 outside the sample)
  // Membership bitmap: bit (inst - base) & 63 of word (inst - base) >> 6, base = lo rounded down to a
  // multiple of 64.  Block-major: zeroed before the pass.
  int64_t base;
  unsigned long long* bitmap;
  long long* info;           // [ORD_INFO_WORDS]
};
inline int32_t order_walk_lds_bytes(bool staged) {
  return 8 * 8 + (staged ? kWavesPerBlock * kStatsStageWords * 4 : 0);
}
int launch_order_walk(const OrderWalkParams& p, int32_t blocks, void* stream);

// An order position the select resolves: after a digit pass, `prefix` is the bits of its key from the
// pass's digit up, `rank` its position among the candidates that share that prefix, `group` the index
// of its prefix among the distinct prefixes of the positions (which are kept by ascending rank, so
// the distinct prefixes ascend with the group index).
struct OrderPos {
  unsigned long long prefix;
  long long rank;
  int32_t group, bad;        // bad: no bucket held the rank (the histogram and the rank disagree)
};
struct OrderSelectParams {
  const long long* plane;            // [n]
  const unsigned long long* bitmap;  // element i is bit i + off (off = lo - base, < 64)
  int64_t n, off;
  int32_t desc, n_pos;
  OrderPos* pos;                     // [n_pos]
  uint32_t* hist;                    // [n_pos][kOrderBins], zero before the first pass
};
inline int32_t order_hist_lds_bytes(int32_t n_pos) { return n_pos * (kOrderBins * 4 + 8); }
// One digit pass at bit `shift`: the histogram kernel (blocks workgroups), then the one-workgroup
// choice, which also regroups the positions and zeroes the histogram for the next pass.
int launch_order_pass(const OrderSelectParams& p, int32_t shift, int32_t blocks, void* stream);
// Top-k compaction.  less[w] / equal[w]: the members with key < T / key == T, T = pos[0].prefix after
// the last pass, as bitmaps of `words` words in the membership bitmap's convention.
int launch_order_mark(const OrderSelectParams& p, int64_t words, unsigned long long* less, unsigned long long* equal,
                      void* stream);
// out_inst[j], out_val[j], j < k: all of list_a (n_a = info_a[3] entries) then the first k - n_a of
// list_b; the values gathered from the plane (instance lo + i at plane[i]); -1 / 0 where a list is
// short or an instance lies outside [lo, lo + n).
int launch_order_gather(const OrderSelectParams& p, int64_t lo, int64_t k, const long long* list_a,
                        const unsigned long long* info_a, const long long* list_b, const unsigned long long* info_b,
                        long long* out_inst, long long* out_val, void* stream);

}  // namespace clsnap
