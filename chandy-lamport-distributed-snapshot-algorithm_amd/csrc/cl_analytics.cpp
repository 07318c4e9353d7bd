// cl_analytics.cpp -- the host layer of the batch analytics behind include/clsnap.h: statistics
// (cl_stats.hip), census (cl_census.hip), selection (cl_select.hip), crosstab (cl_crosstab.hip) and
// the device-resident instance sets (cl_iset.hip), the tuple group-by (cl_groups.hip) and the ordering
// calls -- top-k, quantiles, values (cl_order.hip).
//
// It owns its scratch, its timers and the sets, and reads a sim through cl_host.h only: the facts
// its argument checks need, the device and stream, and the record planes and tables of a sample.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cl_host.h"

using namespace clsnap;

// ---------------------------------------------------------------------------
// cl_iset: a device-resident set of instances of one sim (cl_iset.hip)
// ---------------------------------------------------------------------------
// Only a set of indices: nothing in it refers to a run, an engine or a record layout.  The bitmap
// (stride / 64 words, the bits from n_instances on 0) is allocated on the first call that needs it
// on the device; until then a set made from a list keeps the list (`pending`; empty: the empty set).
struct cl_iset {
  cl_sim* sim = nullptr;
  DevBuf<unsigned long long> bits;
  bool resident = false;          // bits holds the set
  std::vector<int64_t> pending;   // the list to scatter when the bitmap is made
};

namespace clsnap {

// The radix select and the top-k compaction of cl_order.hip over a value plane and its membership
// bitmap on the device, with their scratch and their timer: what cl_snapshot_topk and
// cl_snapshot_quantiles run after the value walk, and cl_order_plane_device on an uploaded plane.
struct OrderEngine {
  struct Plane {
    const long long* values;           // [n]: element i is instance lo + i
    const unsigned long long* bitmap;  // bit (lo + i - base) of it: element i is in the sample
    int64_t n, lo, base;
    long long vmin, vmax;              // of the sample (any values on an empty one)
    int32_t desc;
  };
  DevBuf<OrderPos> d_pos;
  DevBuf<uint32_t> d_hist;
  DevBuf<unsigned long long> d_less, d_equal, d_cinfo;
  DevBuf<long long> d_bsum, d_list_a, d_list_b, d_out_inst, d_out_val;
  std::vector<OrderPos> h_pos;  // the positions' initial state, uploaded by select()
  DevTimer<4> tm;    // select passes: 0 .. 1, compaction: 2 .. 3
  int ran = 0;       // bit 0: the latest operation ran select passes, bit 1: a compaction

  int64_t bytes() const {
    return (int64_t)(d_pos.bytes() + d_hist.bytes() + d_less.bytes() + d_equal.bytes() + d_cinfo.bytes() +
                     d_bsum.bytes() + d_list_a.bytes() + d_list_b.bytes() + d_out_inst.bytes() + d_out_val.bytes());
  }

  OrderSelectParams params(const Plane& pl, int32_t n_pos) const {
    OrderSelectParams p{};
    p.plane = pl.values, p.bitmap = pl.bitmap, p.n = pl.n, p.off = pl.lo - pl.base;
    p.desc = pl.desc, p.n_pos = n_pos, p.pos = d_pos.p, p.hist = d_hist.p;
    return p;
  }

  // Enqueues the digit passes that resolve the order positions `ranks` (ascending, each below the
  // sample's size) and leaves their state in d_pos.  The keys of the sample lie in [kmin, kmax]: the
  // bits above the highest one in which those differ are common, so only the digits below are passed.
  int select(const Plane& pl, const std::vector<int64_t>& ranks, hipStream_t stream, int32_t n_cus) {
    const int32_t n_pos = (int32_t)ranks.size();
    int rc;
    if ((rc = d_pos.ensure((size_t)n_pos)) || (rc = d_hist.ensure((size_t)n_pos * kOrderBins))) return rc;
    const uint64_t kmin = order_key(pl.desc ? pl.vmax : pl.vmin, pl.desc);
    const uint64_t kmax = order_key(pl.desc ? pl.vmin : pl.vmax, pl.desc);
    const int32_t bits = kmin == kmax ? 0 : 64 - __builtin_clzll(kmin ^ kmax);
    const int32_t passes = (bits + kOrderDigitBits - 1) / kOrderDigitBits;
    h_pos.resize((size_t)n_pos);  // (a member: the host's until its copy is done)
    for (int32_t j = 0; j < n_pos; ++j)
      h_pos[(size_t)j] =
          OrderPos{passes * kOrderDigitBits >= 64 ? 0 : kmin >> (passes * kOrderDigitBits), ranks[(size_t)j], 0, 0};
    HIP_TRY(hipMemcpyAsync(d_pos.p, h_pos.data(), h_pos.size() * sizeof(OrderPos), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(d_hist.p, 0, (size_t)n_pos * kOrderBins * sizeof(uint32_t), stream));
    const OrderSelectParams p = params(pl, n_pos);
    const int32_t blocks = (int32_t)std::max<int64_t>(
        1, std::min<int64_t>((pl.n + 8 * kOrderThreads - 1) / (8 * kOrderThreads), 4 * (int64_t)std::max(n_cus, 1)));
    if ((rc = tm.mark(0, stream))) return rc;
    for (int32_t q = 0; q < passes; ++q) {
      const int e = launch_order_pass(p, (passes - 1 - q) * kOrderDigitBits, blocks, stream);
      if (e) return set_err(CL_E_DEVICE, "order kernels: %s", hipGetErrorString((hipError_t)e));
    }
    if ((rc = tm.mark(1, stream))) return rc;
    ran |= 1;
    return CL_OK;
  }

  // The final state of the positions: *out[j] for ranks[j] of the latest select.
  int read_positions(int32_t n_pos, std::vector<OrderPos>* out, hipStream_t stream) {
    out->resize((size_t)n_pos);
    HIP_TRY(hipMemcpyAsync(out->data(), d_pos.p, (size_t)n_pos * sizeof(OrderPos), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (const OrderPos& z : *out)
      if (z.bad) return set_err(CL_E_DEVICE, "order select: a digit histogram does not hold its rank");
    return CL_OK;
  }

  // The first k (1 <= k <= the sample's size) elements of the order into insts[k], values[k].
  int topk(const Plane& pl, int64_t k, int64_t* insts, int64_t* values, hipStream_t stream, int32_t n_cus) {
    ran = 0;
    int rc = select(pl, std::vector<int64_t>{k - 1}, stream, n_cus);
    if (rc) return rc;
    const OrderSelectParams p = params(pl, 1);
    SelectParams c{};  // the select's compaction, over the two bitmaps in turn
    c.base = pl.base;
    c.words = (pl.lo + pl.n - pl.base + kWave - 1) / kWave;
    c.cap = k;
    const int64_t n_blocks = (c.words + kSelBlockWords - 1) / kSelBlockWords;
    if ((rc = d_less.ensure((size_t)c.words)) || (rc = d_equal.ensure((size_t)c.words)) || (rc = d_cinfo.ensure(8)) ||
        (rc = d_bsum.ensure((size_t)n_blocks)) || (rc = d_list_a.ensure((size_t)k)) ||
        (rc = d_list_b.ensure((size_t)k)) || (rc = d_out_inst.ensure((size_t)k)) || (rc = d_out_val.ensure((size_t)k)))
      return rc;
    c.bsum = d_bsum.p;
    HIP_TRY(hipMemsetAsync(d_cinfo.p, 0, 8 * sizeof(unsigned long long), stream));
    if ((rc = tm.mark(2, stream))) return rc;
    int e = launch_order_mark(p, c.words, d_less.p, d_equal.p, stream);
    c.bitmap = d_less.p, c.info = d_cinfo.p, c.out = d_list_a.p;
    if (!e) e = launch_select_compact(c, stream);
    c.bitmap = d_equal.p, c.info = d_cinfo.p + 4, c.out = d_list_b.p;
    if (!e) e = launch_select_compact(c, stream);
    if (!e)
      e = launch_order_gather(p, pl.lo, k, d_list_a.p, d_cinfo.p, d_list_b.p, d_cinfo.p + 4, d_out_inst.p, d_out_val.p,
                              stream);
    if (e) return set_err(CL_E_DEVICE, "order kernels: %s", hipGetErrorString((hipError_t)e));
    if ((rc = tm.mark(3, stream))) return rc;
    ran |= 2;
    std::vector<long long> gi((size_t)k), gv((size_t)k);
    HIP_TRY(hipMemcpyAsync(gi.data(), d_out_inst.p, (size_t)k * sizeof(long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(gv.data(), d_out_val.p, (size_t)k * sizeof(long long), hipMemcpyDeviceToHost, stream));
    std::vector<OrderPos> pos;
    if ((rc = read_positions(1, &pos, stream))) return rc;
    // ---- the rows are those of the answer, each list in instance order: sorted here by (key, instance)
    std::vector<int64_t> order((size_t)k);
    for (int64_t j = 0; j < k; ++j) {
      if (gi[(size_t)j] < 0) return set_err(CL_E_DEVICE, "order top-k: the lists hold fewer than %lld rows", (long long)k);
      order[(size_t)j] = j;
    }
    const int32_t desc = pl.desc;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
      const uint64_t ka = order_key(gv[(size_t)a], desc), kb = order_key(gv[(size_t)b], desc);
      return ka != kb ? ka < kb : gi[(size_t)a] < gi[(size_t)b];
    });
    for (int64_t j = 0; j < k; ++j) {
      insts[j] = gi[(size_t)order[(size_t)j]];
      values[j] = gv[(size_t)order[(size_t)j]];
    }
    return CL_OK;
  }

  // values[j] = the value at position ranks[j] (any order, each below the sample's size), j < n_q.
  int at_ranks(const Plane& pl, const int64_t* ranks, int32_t n_q, int64_t* values, hipStream_t stream, int32_t n_cus) {
    ran = 0;
    std::vector<int32_t> by((size_t)n_q);
    for (int32_t j = 0; j < n_q; ++j) by[(size_t)j] = j;
    std::sort(by.begin(), by.end(), [&](int32_t a, int32_t b) { return ranks[a] < ranks[b]; });
    std::vector<int64_t> sorted((size_t)n_q);
    for (int32_t j = 0; j < n_q; ++j) sorted[(size_t)j] = ranks[by[(size_t)j]];
    int rc = select(pl, sorted, stream, n_cus);
    if (rc) return rc;
    std::vector<OrderPos> pos;
    if ((rc = read_positions(n_q, &pos, stream))) return rc;
    for (int32_t j = 0; j < n_q; ++j) values[by[(size_t)j]] = order_value(pos[(size_t)j].prefix, pl.desc);
    return CL_OK;
  }

  // Device ms of the latest operation's stages (the stream is idle): select passes, compaction.
  int stage_ms(double* select_ms, double* compact_ms) const {
    *select_ms = *compact_ms = 0;
    int rc;
    if ((ran & 1) && (rc = tm.ms(0, 1, select_ms))) return rc;
    if ((ran & 2) && (rc = tm.ms(2, 3, compact_ms))) return rc;
    return CL_OK;
  }
};

// The nearest-rank position of quantile num / den in a sample of `sample` > 0 values.
static int64_t quantile_rank(const cl_quantile& q, int64_t sample) {
  if (q.num == 0) return 0;
  const unsigned __int128 prod = (unsigned __int128)(uint64_t)q.num * (uint64_t)sample;
  return (int64_t)((prod + (uint64_t)q.den - 1) / (uint64_t)q.den) - 1;
}

struct Analytics {
  cl_sim* const sim;
  SimDevice dev{};  // as of the latest device use (the stream the timers' marks lie on)
  // per-snapshot batch statistics (cl_snapshot_stats, cl_stats.hip)
  DevBuf<long long> d_stats;
  DevTimer<2> st;
  // snapshot outcome census (cl_snapshot_census, cl_census.hip); cs.done: the event pairs of the
  // latest census (key pass, gather, class_of)
  DevBuf<CensusEntry> d_cs_table, d_cs_out;
  DevBuf<uint32_t> d_cs_list;
  DevBuf<unsigned long long> d_cs_info, d_cs_keys;
  DevBuf<int32_t> d_cs_class, d_cs_rank;
  DevTimer<6> cs;
  // group-by over a tuple of snapshot quantities (cl_snapshot_groups, cl_groups.hip): the census's
  // table scratch above, plus the returned groups' smallest instances and their tuples; gr: the
  // event pairs of the latest call as cs (mark 6: between the table's initialisation and the key
  // pass), grv: the values kernel
  DevBuf<long long> d_gr_first, d_gr_vals;
  DevTimer<7> gr;
  DevTimer<2> grv;
  // instance selection (cl_select_instances, cl_select.hip): verdict bitmap, block sums, output
  DevBuf<unsigned long long> d_sel_bits, d_sel_info;
  DevBuf<long long> d_sel_bsum, d_sel_out;
  DevBuf<int32_t> d_sel_ticks;
  DevTimer<3> sel;  // start, evaluated, compacted
  // instance sets (cl_iset, cl_iset.hip): the sets alive (freed with the sim), the list upload and
  // the count's scalar; the listing borrows the selection's compaction scratch
  std::vector<cl_iset*> isets;
  DevBuf<long long> d_is_list;
  DevBuf<unsigned long long> d_is_count;
  DevTimer<2> is;
  // joint distribution of two snapshot quantities (cl_snapshot_crosstab, cl_crosstab.hip): the result words
  DevBuf<long long> d_xt;
  DevTimer<2> xt;
  // ordering (cl_snapshot_topk, cl_snapshot_quantiles, cl_snapshot_values; cl_order.hip): the value
  // plane, its membership bitmap and the walk's info; the select and the compaction are the engine's.
  // ord: the walk's event pair; ord.done: the latest call ran a walk.
  DevBuf<long long> d_ord_plane, d_ord_info;
  DevBuf<unsigned long long> d_ord_bits;
  OrderEngine order;
  DevTimer<2> ord;

  explicit Analytics(cl_sim* s) : sim(s) {}
  ~Analytics() {
    for (cl_iset* s : isets) delete s;  // (the sets still alive go with their sim)
  }

  // The opening of the analytics calls (stats, census, select): executes what is pending, makes the
  // token histories resident, and describes the sample of snapshot sid over [lo, hi) and the planes
  // its kernels walk (cl_sample.h).  `in` (the conditional calls): the instance set whose members
  // the sample is taken from, made resident here.
  int sample_begin(int32_t sid, int64_t lo, int64_t hi, SampleParams* s, SimTables* t, cl_iset* in) {
    *s = SampleParams{};
    int rc = sim_records(sim, &dev, s, t);
    if (rc) return rc;
    if (in && (rc = iset_resident(in))) return rc;
    s->sid = sid;
    s->lo = lo;
    s->hi = hi;
    // block-major records are in slot order: a sub-range's instances may sit in any tile
    s->tile_lo = s->blocked ? 0 : lo / kWave;
    s->tile_hi = hi <= lo ? s->tile_lo : s->blocked ? s->stride / kWave : (hi + kWave - 1) / kWave;
    s->where = in ? in->bits.p : nullptr;  // (the conditional calls: only the set's members)
    return CL_OK;
  }

  // Workgroups of a sample walk over `tiles` tiles whose workgroups need lds_bytes of LDS: a
  // grid-stride grid sized to the chip, as many workgroups per CU as its LDS holds (up to 8).
  // (one tile per wave where the batch is small: at 2^17 instances of C3, 4 tiles per wave --
  // a quarter of the workgroups and of their closing atomics -- measured 0.117 against 0.069 ms)
  int32_t sample_grid(int64_t tiles, int32_t lds_bytes) const {
    return (int32_t)std::min<int64_t>((tiles + kWavesPerBlock - 1) / kWavesPerBlock,
                                      (int64_t)stats_blocks_per_cu(lds_bytes) * std::max(dev.n_cus, 1));
  }

  // The four info words of a call that counted over n instances -- instances, OK, sample, and its
  // matches or classes -- read back once the stream is idle; *done = 1 then (the call's first
  // event pair is complete).  More matches or classes than instances are refused.
  int read_info(const unsigned long long* d_info, int64_t n, const char* what, int* done, unsigned long long (&h)[4]) {
    HIP_TRY(hipMemcpyAsync(h, d_info, sizeof h, hipMemcpyDeviceToHost, dev.stream));
    HIP_TRY(hipStreamSynchronize(dev.stream));
    if (done) *done = 1;
    if ((int64_t)h[3] > n)
      return set_err(CL_E_DEVICE, "%s: %lld matches or classes of %lld instances", what, (long long)h[3], (long long)n);
    return CL_OK;
  }

  // cl_snapshot_stats: the statistics of snapshot sid over [lo, hi) into out[L.total_words]
  // (arguments checked by the caller).  One kernel pass when the topology's N * rw record
  // words fit the LDS accumulator budget (stats_pass_words), else one pass per range of chunks;
  // the first pass also takes the per-instance totals.
  int stats(int32_t sid, int64_t lo, int64_t hi, const StatsLayout& L, int64_t* out, cl_iset* in) {
    StatsParams p{};
    SimTables t{};
    int rc = sample_begin(sid, lo, hi, &p.s, &t, in);
    if (rc) return rc;
    const hipStream_t stream = dev.stream;
    std::vector<long long> h((size_t)L.total_words, 0);
    std::fill(h.begin() + L.min_begin, h.begin() + L.min_end, INT64_MAX);
    std::fill(h.begin() + L.max_begin, h.begin() + L.max_end, INT64_MIN);
    if ((rc = d_stats.ensure(h.size()))) return rc;
    HIP_TRY(hipMemcpyAsync(d_stats.p, h.data(), h.size() * sizeof(long long), hipMemcpyHostToDevice, stream));
    p.tab = t;
    p.word_ch = t.word_ch;
    p.lay = L;
    p.out = d_stats.p;
    const int64_t tiles = p.s.tile_hi - p.s.tile_lo;
    const int32_t budget = stats_pass_words((int32_t)L.tick_bins, (int32_t)L.msg_bins);
    const int32_t n_chunks = stats_chunks(p.s.n_nodes, p.s.rw);
    // the grid for the LDS of the largest pass (two workgroups per CU at the full budget)
    const int32_t pass_words = std::min(budget, p.s.n_nodes * p.s.rw);
    const int32_t blocks =
        sample_grid(tiles, stats_lds_bytes(pass_words, (int32_t)L.tick_bins, (int32_t)L.msg_bins));
    if ((rc = st.mark(0, stream))) return rc;
    for (int32_t c0 = 0; c0 < n_chunks && tiles > 0;) {
      int32_t c1 = c0, words = 0;
      while (c1 < n_chunks) {
        const StatsChunk ch = stats_chunk(p.s.n_nodes, p.s.rw, c1);
        if (words + ch.nv * ch.kw > budget) break;
        words += ch.nv * ch.kw;
        ++c1;
      }
      if (c1 == c0) return set_err(CL_E_LIMIT, "statistics accumulators of one chunk exceed the LDS budget");
      p.chunk_lo = c0;
      p.chunk_hi = c1;
      p.totals = c0 == 0 ? 1 : 0;
      p.acc_words = words;
      const int e = launch_stats(p, blocks, stream);
      if (e) return set_err(CL_E_DEVICE, "statistics kernel: %s", hipGetErrorString((hipError_t)e));
      c0 = c1;
    }
    if ((rc = st.mark(1, stream))) return rc;
    st.done = 1;
    HIP_TRY(hipMemcpyAsync(out, d_stats.p, h.size() * sizeof(long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return CL_OK;
  }

  // The census's table scratch for a range of n instances (shared by the census and the tuple
  // group-by), and the fields of *p that name it and the tables next to the records.
  int table_begin(CensusParams* p, const SimTables& t, int64_t n, int32_t lds_slots, bool class_of) {
    int rc;
    p->slots = 16;
    while (p->slots < 2 * n) p->slots <<= 1;
    if ((rc = d_cs_table.ensure((size_t)p->slots + 1)) || (rc = d_cs_list.ensure((size_t)n)) ||
        (rc = d_cs_info.ensure(4)))
      return rc;
    if (class_of && ((rc = d_cs_keys.ensure((size_t)n)) || (rc = d_cs_class.ensure((size_t)n)))) return rc;
    p->tab = t;
    p->lds_slots = lds_slots;
    p->staged = sample_staged(p->s);
    p->empty_key = kCensusEmptyKey;
    // (tests move the marker onto a key that occurs, to run the extra entry's path)
    if (const char* v = std::getenv("CLSNAP_CENSUS_EMPTY_KEY")) p->empty_key = std::strtoull(v, nullptr, 0);
    p->table = d_cs_table.p;
    p->list = d_cs_list.p;
    p->info = d_cs_info.p;
    p->keys = class_of ? d_cs_keys.p : nullptr;
    p->class_of = class_of ? d_cs_class.p : nullptr;
    return CL_OK;
  }

  // After a key pass (marks 0 and 1 of `tm` around it): the counters into *info, the k classes
  // compacted on the device and sorted here (count descending, key ascending) into *out, and
  // class_of[n] when asked for.  tm.done counts the event pairs completed (key pass, gather, class_of).
  template <int N>
  int table_finish(const CensusParams& p, int64_t n, DevTimer<N>& tm, const char* what,
                   std::vector<CensusEntry>* out, int32_t* class_of, cl_census_info* info) {
    const hipStream_t stream = dev.stream;
    int rc, e;
    unsigned long long h[4] = {0, 0, 0, 0};
    if ((rc = read_info(d_cs_info.p, n, what, &tm.done, h))) return rc;
    const int64_t k = (int64_t)h[3];
    info->instances = (int64_t)h[0], info->ok = (int64_t)h[1], info->sample = (int64_t)h[2], info->n_classes = k;
    // ---- the k classes: compacted on the device, sorted here
    std::vector<CensusEntry> got((size_t)k);
    if (k > 0) {
      if ((rc = d_cs_out.ensure((size_t)k))) return rc;
      if ((rc = tm.mark(2, stream))) return rc;
      if ((e = launch_census_gather(p, k, d_cs_out.p, stream)))
        return set_err(CL_E_DEVICE, "%s kernels: %s", what, hipGetErrorString((hipError_t)e));
      if ((rc = tm.mark(3, stream))) return rc;
      HIP_TRY(hipMemcpyAsync(got.data(), d_cs_out.p, (size_t)k * sizeof(CensusEntry), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      tm.done = 2;
    } else if (class_of) {
      // (no gather: an empty pair, so that tm.done below counts recorded pairs only)
      if ((rc = tm.mark(2, stream)) || (rc = tm.mark(3, stream))) return rc;
    }
    std::vector<int32_t> order((size_t)k);
    for (int64_t j = 0; j < k; ++j) order[(size_t)j] = (int32_t)j;
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
      const CensusEntry &x = got[(size_t)a], &y = got[(size_t)b];
      return x.count != y.count ? x.count > y.count : x.key < y.key;
    });
    out->resize((size_t)k);
    for (int64_t j = 0; j < k; ++j) (*out)[(size_t)j] = got[(size_t)order[(size_t)j]];
    if (!class_of) return CL_OK;
    // ---- class_of: the ranks go back into the table, a lookup maps key -> rank per instance
    std::vector<int32_t> rank((size_t)std::max<int64_t>(k, 1));
    for (int64_t j = 0; j < k; ++j) rank[(size_t)order[(size_t)j]] = (int32_t)j;
    if ((rc = d_cs_rank.ensure(rank.size()))) return rc;
    HIP_TRY(hipMemcpyAsync(d_cs_rank.p, rank.data(), rank.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    if ((rc = tm.mark(4, stream))) return rc;
    if ((e = launch_census_class_of(p, k, d_cs_rank.p, stream)))
      return set_err(CL_E_DEVICE, "%s kernels: %s", what, hipGetErrorString((hipError_t)e));
    if ((rc = tm.mark(5, stream))) return rc;
    HIP_TRY(hipMemcpyAsync(class_of, d_cs_class.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    tm.done = 3;
    return CL_OK;
  }

  // cl_snapshot_census (arguments checked by the caller): the classes of snapshot sid over
  // [lo, hi), sorted, into *out; class_of[hi - lo] when asked for.  lds_slots: the workgroup
  // table's entries, 0 for none.
  int census(int32_t sid, int64_t lo, int64_t hi, int32_t lds_slots, std::vector<CensusEntry>* out,
             int32_t* class_of, cl_census_info* info, cl_iset* in) {
    CensusParams p{};
    SimTables t{};
    int rc = sample_begin(sid, lo, hi, &p.s, &t, in);
    if (rc) return rc;
    const hipStream_t stream = dev.stream;
    const int64_t n = hi - lo;
    out->clear();
    *info = cl_census_info{};
    if (n == 0) {
      cs.done = 0;
      return CL_OK;
    }
    if (n > ((int64_t)1 << 29)) return set_err(CL_E_LIMIT, "census of more than 2^29 instances");
    if ((rc = table_begin(&p, t, n, lds_slots, class_of != nullptr))) return rc;
    const int32_t blocks = sample_grid(p.s.tile_hi - p.s.tile_lo, census_lds_bytes(lds_slots, p.staged != 0));
    if ((rc = cs.mark(0, stream))) return rc;
    HIP_TRY(hipMemsetAsync(d_cs_info.p, 0, 4 * sizeof(unsigned long long), stream));
    int e = launch_census_init(p, stream);
    if (!e) e = launch_census_keys(p, blocks, stream);
    if (e) return set_err(CL_E_DEVICE, "census kernels: %s", hipGetErrorString((hipError_t)e));
    if ((rc = cs.mark(1, stream))) return rc;
    return table_finish(p, n, cs, "census", out, class_of, info);
  }

  // cl_snapshot_groups (arguments checked by the caller): the groups of the term tuples over
  // [lo, hi), sorted, into *out; group_of[hi - lo] when asked for; the tuples of the first
  // min(n_groups, max_groups) groups, evaluated on the device for each group's smallest instance,
  // into values[][n_terms].  The table, its scratch and the order are the census's.
  int groups(int64_t lo, int64_t hi, const cl_group_term* terms, int32_t n_terms, int32_t lds_slots,
             int64_t max_groups, std::vector<CensusEntry>* out, int64_t* values, int32_t* group_of,
             cl_census_info* info, cl_iset* in) {
    GroupsParams p{};
    SimTables t{};
    int rc = sample_begin(terms[0].sid, lo, hi, &p.c.s, &t, in);
    if (rc) return rc;
    const hipStream_t stream = dev.stream;
    const int64_t n = hi - lo;
    out->clear();
    *info = cl_census_info{};
    gr.done = grv.done = 0;
    if (n == 0) return CL_OK;
    if ((rc = table_begin(&p.c, t, n, lds_slots, group_of != nullptr))) return rc;
    p.n_terms = n_terms;
    for (int32_t k = 0; k < n_terms; ++k) {
      std::memcpy(&p.term[k], &terms[k], sizeof(GroupTerm));
      p.reads_records |= terms[k].field != SEL_TICK;
      const int32_t sid = terms[k].sid;
      if (sid != terms[0].sid && std::find(p.other_sid, p.other_sid + p.n_other, sid) == p.other_sid + p.n_other)
        p.other_sid[p.n_other++] = sid;
    }
    const bool staged = p.c.staged && p.reads_records;
    int32_t blocks = sample_grid(p.c.s.tile_hi - p.c.s.tile_lo, census_lds_bytes(lds_slots, staged));
    // A list of completion ticks reads two words per instance and has hundreds of groups and more:
    // what counts is the closing flush, one global insert per occupied table entry and workgroup,
    // so one workgroup per CU (C3 at 2^20, tick(0), tick(4): key pass 0.171 ms with the 5 per CU
    // the LDS admits, 0.108 with 2, 0.090 with 1; the five ticks 0.590 -> 0.443).  Record lists
    // keep the census's grid: with 1 per CU the 8 node words take 0.133 against 0.112 ms.
    if (!p.reads_records) blocks = std::min(blocks, std::max(dev.n_cus, 1));
    if ((rc = gr.mark(0, stream))) return rc;
    HIP_TRY(hipMemsetAsync(d_cs_info.p, 0, 4 * sizeof(unsigned long long), stream));
    int e = launch_census_init(p.c, stream);
    if ((rc = gr.mark(6, stream))) return rc;
    if (!e) e = launch_groups_keys(p, blocks, stream);
    if (e) return set_err(CL_E_DEVICE, "groups kernels: %s", hipGetErrorString((hipError_t)e));
    if ((rc = gr.mark(1, stream))) return rc;
    if ((rc = table_finish(p.c, n, gr, "groups", out, group_of, info))) return rc;
    // ---- the tuples of the returned groups, from each group's smallest instance
    const int64_t k = std::min<int64_t>(info->n_classes, max_groups);
    if (k == 0) return CL_OK;
    std::vector<long long> first((size_t)k);
    for (int64_t g = 0; g < k; ++g) first[(size_t)g] = (*out)[(size_t)g].first;
    if ((rc = d_gr_first.ensure((size_t)k)) || (rc = d_gr_vals.ensure((size_t)k * (size_t)n_terms))) return rc;
    HIP_TRY(hipMemcpyAsync(d_gr_first.p, first.data(), (size_t)k * sizeof(long long), hipMemcpyHostToDevice, stream));
    if ((rc = grv.mark(0, stream))) return rc;
    if ((e = launch_groups_values(p, t.rec_slot, d_gr_first.p, k, d_gr_vals.p, stream)))
      return set_err(CL_E_DEVICE, "groups kernels: %s", hipGetErrorString((hipError_t)e));
    if ((rc = grv.mark(1, stream))) return rc;
    HIP_TRY(hipMemcpyAsync(values, d_gr_vals.p, (size_t)k * (size_t)n_terms * sizeof(long long), hipMemcpyDeviceToHost,
                           stream));
    HIP_TRY(hipStreamSynchronize(stream));  // (also: `first` is the host's until its copy is done)
    grv.done = 1;
    return CL_OK;
  }

  // The scratch of the bitmap compaction (launch_select_compact) for p.words words and p.cap
  // entries, shared by the selection and the listing of an instance set.
  int compact_scratch(SelectParams* p, bool want_ticks) {
    const int64_t n_blocks = (p->words + kSelBlockWords - 1) / kSelBlockWords;
    int rc;
    if ((rc = d_sel_bsum.ensure((size_t)n_blocks)) || (rc = d_sel_info.ensure(4)) ||
        (rc = d_sel_out.ensure((size_t)std::max<int64_t>(p->cap, 1))))
      return rc;
    if (want_ticks && (rc = d_sel_ticks.ensure((size_t)std::max<int64_t>(p->cap, 1)))) return rc;
    p->info = d_sel_info.p;
    p->bsum = d_sel_bsum.p;
    p->out = d_sel_out.p;
    p->ticks = want_ticks ? d_sel_ticks.p : nullptr;
    return CL_OK;
  }

  // cl_select_instances (arguments checked by the caller): the instances of the sample of
  // snapshot sid over [lo, hi) that satisfy every clause, ascending, the first `cap` of them into
  // insts (and their completion ticks into ticks).  Both stages are enqueued back to back; the
  // host waits once, for the info, then copies the n_returned entries.
  // `in` (cl_select_instances_in): the sample is that of the set's members.  `into`
  // (cl_iset_from_clauses): the verdicts are written into that set's bitmap and stay there; nothing
  // is listed (cap 0), the compaction only counts.  The verdict bitmap is never the one filtered on.
  int select(int32_t sid, int64_t lo, int64_t hi, const cl_select_clause* clauses, int32_t n_clauses, int64_t* insts,
             int32_t* ticks, int64_t cap, cl_select_info* info, cl_iset* in, cl_iset* into) {
    SelectParams p{};
    SimTables t{};
    int rc = sample_begin(sid, lo, hi, &p.s, &t, in);
    if (rc) return rc;
    const hipStream_t stream = dev.stream;
    *info = cl_select_info{};
    const int64_t n = hi - lo;
    if (into && n == 0) return iset_clear(into);
    if (n == 0) return CL_OK;
    p.tab = t;
    p.staged = sample_staged(p.s);
    p.n_clauses = n_clauses;
    for (int32_t q = 0; q < n_clauses; ++q) {
      std::memcpy(&p.clause[q], &clauses[q], sizeof(SelectClause));
      const int32_t f = clauses[q].field;
      p.need_records |= f != SEL_TICK;
      p.need_totals |= f == SEL_MSGS || f == SEL_INFLIGHT;
      p.need_key |= f == SEL_KEY;
    }
    p.base = lo / kWave * kWave;
    p.words = (hi - p.base + kWave - 1) / kWave;
    p.cap = std::min(cap, n);
    if (!into && (rc = d_sel_bits.ensure((size_t)p.words))) return rc;
    if ((rc = compact_scratch(&p, ticks != nullptr))) return rc;
    const int32_t blocks = sample_grid(p.s.tile_hi - p.s.tile_lo, select_lds_bytes(p.staged && p.need_records));
    if ((rc = sel.mark(0, stream))) return rc;
    HIP_TRY(hipMemsetAsync(d_sel_info.p, 0, 4 * sizeof(unsigned long long), stream));
    if (into) {
      // the whole set is cleared: the words of [lo, hi) are a part of it
      if ((rc = iset_clear(into))) return rc;
      p.bitmap = into->bits.p + p.base / kWave;
    } else {
      p.bitmap = d_sel_bits.p;
      // block-major: the lanes OR their bits in; instance-major: every word is stored
      if (p.s.blocked) HIP_TRY(hipMemsetAsync(d_sel_bits.p, 0, (size_t)p.words * sizeof(unsigned long long), stream));
    }
    int e = launch_select_eval(p, blocks, stream);
    if (e) return set_err(CL_E_DEVICE, "select kernels: %s", hipGetErrorString((hipError_t)e));
    if ((rc = sel.mark(1, stream))) return rc;
    if ((e = launch_select_compact(p, stream)))
      return set_err(CL_E_DEVICE, "select kernels: %s", hipGetErrorString((hipError_t)e));
    if ((rc = sel.mark(2, stream))) return rc;
    unsigned long long h[4] = {0, 0, 0, 0};
    if ((rc = read_info(d_sel_info.p, n, "select", &sel.done, h))) return rc;
    info->instances = (int64_t)h[0], info->ok = (int64_t)h[1], info->sample = (int64_t)h[2];
    info->n_match = (int64_t)h[3];
    info->n_returned = std::min<int64_t>(info->n_match, cap);
    if (info->n_returned > 0) {
      const size_t k = (size_t)info->n_returned;
      HIP_TRY(hipMemcpyAsync(insts, d_sel_out.p, k * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
      if (ticks) HIP_TRY(hipMemcpyAsync(ticks, d_sel_ticks.p, k * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
    }
    return CL_OK;
  }

  // cl_snapshot_crosstab (arguments checked by the caller): the contingency table and joint
  // moments of axes a and b over [lo, hi) into out[XT_CELLS + a->bins * b->bins].  One kernel; the
  // walk is that of axis a's snapshot, the kernel takes axis b's planes from the same SampleParams.
  int crosstab(int64_t lo, int64_t hi, const cl_crosstab_axis* a, const cl_crosstab_axis* b, int64_t* out,
               cl_iset* in) {
    CrosstabParams p{};
    SimTables t{};
    int rc = sample_begin(a->sid, lo, hi, &p.s, &t, in);
    if (rc) return rc;
    const hipStream_t stream = dev.stream;
    std::memcpy(&p.a, a, sizeof p.a);
    std::memcpy(&p.b, b, sizeof p.b);
    const int32_t cells = a->bins * b->bins;
    std::vector<long long> h((size_t)XT_CELLS + (size_t)cells, 0);
    h[XT_MIN_A] = h[XT_MIN_B] = INT64_MAX;
    h[XT_MAX_A] = h[XT_MAX_B] = INT64_MIN;
    if ((rc = d_xt.ensure(h.size()))) return rc;
    HIP_TRY(hipMemcpyAsync(d_xt.p, h.data(), h.size() * sizeof(long long), hipMemcpyHostToDevice, stream));
    p.tab = t;
    p.staged = sample_staged(p.s);
    p.out = d_xt.p;
    const int64_t tiles = p.s.tile_hi - p.s.tile_lo;
    const bool reads_records = a->field != SEL_TICK || b->field != SEL_TICK;
    const int32_t blocks = sample_grid(tiles, crosstab_lds_bytes(cells, p.staged && reads_records));
    if ((rc = xt.mark(0, stream))) return rc;
    if (tiles > 0) {
      const int e = launch_crosstab(p, blocks, stream);
      if (e) return set_err(CL_E_DEVICE, "crosstab kernel: %s", hipGetErrorString((hipError_t)e));
    }
    if ((rc = xt.mark(1, stream))) return rc;
    xt.done = 1;
    HIP_TRY(hipMemcpyAsync(out, d_xt.p, h.size() * sizeof(long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return CL_OK;
  }

  // The value walk of the ordering calls (arguments checked by the caller; lo < hi): the term's
  // value of every instance of [lo, hi) into d_ord_plane, the sample's membership into d_ord_bits,
  // the counters into *info, and the plane as the engine takes it into *pl.
  int order_walk(int64_t lo, int64_t hi, const cl_group_term* term, cl_iset* in, int32_t desc, cl_order_info* info,
                 OrderEngine::Plane* pl) {
    OrderWalkParams p{};
    SimTables t{};
    int rc = sample_begin(term->sid, lo, hi, &p.s, &t, in);
    if (rc) return rc;
    const hipStream_t stream = dev.stream;
    const int64_t n = hi - lo;
    p.tab = t;
    std::memcpy(&p.term, term, sizeof p.term);
    p.staged = sample_staged(p.s) && term->field != SEL_TICK;
    p.base = lo / kWave * kWave;
    const int64_t words = (hi - p.base + kWave - 1) / kWave;
    if ((rc = d_ord_plane.ensure((size_t)n)) || (rc = d_ord_bits.ensure((size_t)words)) ||
        (rc = d_ord_info.ensure(ORD_INFO_WORDS)))
      return rc;
    p.plane = d_ord_plane.p, p.bitmap = d_ord_bits.p, p.info = d_ord_info.p;
    long long h[ORD_INFO_WORDS] = {0, 0, 0, INT64_MAX, INT64_MIN, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(d_ord_info.p, h, sizeof h, hipMemcpyHostToDevice, stream));
    // block-major: the lanes OR their bits in; instance-major: every word is stored
    if (p.s.blocked) HIP_TRY(hipMemsetAsync(d_ord_bits.p, 0, (size_t)words * sizeof(unsigned long long), stream));
    const int32_t blocks = sample_grid(p.s.tile_hi - p.s.tile_lo, order_walk_lds_bytes(p.staged != 0));
    if ((rc = ord.mark(0, stream))) return rc;
    const int e = launch_order_walk(p, blocks, stream);
    if (e) return set_err(CL_E_DEVICE, "order kernels: %s", hipGetErrorString((hipError_t)e));
    if ((rc = ord.mark(1, stream))) return rc;
    HIP_TRY(hipMemcpyAsync(h, d_ord_info.p, sizeof h, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    ord.done = 1;
    if (h[ORD_SAMPLE] < 0 || h[ORD_SAMPLE] > n)
      return set_err(CL_E_DEVICE, "order: a sample of %lld of %lld instances", h[ORD_SAMPLE], (long long)n);
    info->instances = h[ORD_INSTANCES], info->ok = h[ORD_OK], info->sample = h[ORD_SAMPLE];
    *pl = OrderEngine::Plane{d_ord_plane.p, d_ord_bits.p, n, lo, p.base, h[ORD_MIN], h[ORD_MAX], desc};
    return CL_OK;
  }

  // cl_snapshot_topk (arguments checked by the caller).
  int topk(int64_t lo, int64_t hi, const cl_group_term* term, int32_t flags, int64_t k, int64_t* insts,
           int64_t* values, cl_order_info* info, cl_iset* in) {
    *info = cl_order_info{};
    ord.done = order.ran = 0;
    if (hi == lo) return flush_only(term->sid, in);
    OrderEngine::Plane pl{};
    int rc = order_walk(lo, hi, term, in, (flags & kOrderDesc) != 0, info, &pl);
    if (rc) return rc;
    info->n_returned = std::min(k, info->sample);
    if (info->n_returned == 0) return CL_OK;
    return order.topk(pl, info->n_returned, insts, values, dev.stream, dev.n_cus);
  }

  // cl_snapshot_quantiles (arguments checked by the caller).
  int quantiles(int64_t lo, int64_t hi, const cl_group_term* term, const cl_quantile* q, int32_t n_q, int64_t* values,
                int64_t* ranks, cl_order_info* info, cl_iset* in) {
    *info = cl_order_info{};
    ord.done = order.ran = 0;
    OrderEngine::Plane pl{};
    int rc = hi == lo ? flush_only(term->sid, in) : order_walk(lo, hi, term, in, 0, info, &pl);
    if (rc) return rc;
    if (info->sample == 0) {
      for (int32_t j = 0; j < n_q; ++j) ranks[j] = -1;
      return CL_OK;
    }
    for (int32_t j = 0; j < n_q; ++j) ranks[j] = quantile_rank(q[j], info->sample);
    info->n_returned = n_q;
    return order.at_ranks(pl, ranks, n_q, values, dev.stream, dev.n_cus);
  }

  // cl_snapshot_values (arguments checked by the caller).
  int values_of(int64_t lo, int64_t hi, const cl_group_term* term, int64_t* values, uint8_t* in_sample, cl_iset* in) {
    ord.done = order.ran = 0;
    if (hi == lo) return flush_only(term->sid, in);
    cl_order_info info{};
    OrderEngine::Plane pl{};
    int rc = order_walk(lo, hi, term, in, 0, &info, &pl);
    if (rc) return rc;
    const hipStream_t stream = dev.stream;
    HIP_TRY(hipMemcpyAsync(values, d_ord_plane.p, (size_t)pl.n * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    std::vector<unsigned long long> bits;
    if (in_sample) {
      bits.resize((size_t)((hi - pl.base + kWave - 1) / kWave));
      HIP_TRY(hipMemcpyAsync(bits.data(), d_ord_bits.p, bits.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                             stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    if (in_sample)
      for (int64_t i = lo; i < hi; ++i) in_sample[i - lo] = (uint8_t)((bits[(size_t)((i - pl.base) >> 6)] >> ((i - pl.base) & 63)) & 1);
    return CL_OK;
  }

  // An empty range: what is pending is executed, as in every other result query; nothing is walked.
  int flush_only(int32_t sid, cl_iset* in) {
    SampleParams s{};
    SimTables t{};
    return sample_begin(sid, 0, 0, &s, &t, in);
  }

  // ---- instance sets (cl_iset) -------------------------------------------------------------------
  cl_iset* iset_new() {
    cl_iset* s = new cl_iset();
    s->sim = sim;
    isets.push_back(s);
    return s;
  }

  void iset_delete(cl_iset* s) {
    isets.erase(std::remove(isets.begin(), isets.end(), s), isets.end());
    if (s->bits.p) {
      (void)hipSetDevice(dev.device);
      (void)hipStreamSynchronize(dev.stream);  // (a kernel may still read the bitmap)
    }
    delete s;
  }

  int64_t iset_words() const { return sim_facts(sim).stride / kWave; }

  // The set as an all-zero bitmap on the device (allocated now if it never was).
  int iset_clear(cl_iset* s) {
    int rc = sim_device(sim, &dev);
    if (rc) return rc;
    if ((rc = s->bits.ensure((size_t)iset_words()))) return rc;
    HIP_TRY(hipMemsetAsync(s->bits.p, 0, (size_t)iset_words() * sizeof(unsigned long long), dev.stream));
    s->pending.clear();
    s->resident = true;
    return CL_OK;
  }

  int iset_time_end() {
    const int rc = is.mark(1, dev.stream);
    if (!rc) is.done = 1;
    return rc;
  }

  // The first device use of a set: its bitmap is made, the list it was built from scattered into
  // it (`timed`: as the kernels of cl_iset_time).
  int iset_resident(cl_iset* s, bool timed = false) {
    if (s->resident) return CL_OK;
    std::vector<int64_t> list = std::move(s->pending);
    const int rc = iset_scatter(s, list, timed);
    if (rc) {  // (still the list it was: the next use tries again)
      s->resident = false;
      s->pending = std::move(list);
    }
    return rc;
  }
  int iset_scatter(cl_iset* s, const std::vector<int64_t>& list, bool timed) {
    int rc = iset_clear(s);
    if (rc || list.empty()) return rc;
    const hipStream_t stream = dev.stream;
    if ((rc = d_is_list.ensure(list.size()))) return rc;
    HIP_TRY(hipMemcpyAsync(d_is_list.p, list.data(), list.size() * sizeof(long long), hipMemcpyHostToDevice, stream));
    if (timed && (rc = is.mark(0, stream))) return rc;
    const int e = launch_iset_scatter(d_is_list.p, (int64_t)list.size(), sim_facts(sim).n_inst, s->bits.p, stream);
    if (e) return set_err(CL_E_DEVICE, "instance set kernels: %s", hipGetErrorString((hipError_t)e));
    if (timed && (rc = iset_time_end())) return rc;
    HIP_TRY(hipStreamSynchronize(stream));  // (the list is the host's until the copy is done)
    return CL_OK;
  }

  int iset_combine(cl_iset* dst, cl_iset* a, cl_iset* b, int32_t op) {
    int rc;
    if ((rc = iset_resident(a)) || (rc = iset_resident(b))) return rc;
    // (dst is overwritten: only its bitmap is needed, unless it is an operand)
    if (dst != a && dst != b && (rc = iset_clear(dst))) return rc;
    const hipStream_t stream = dev.stream;
    if ((rc = is.mark(0, stream))) return rc;
    const int e = launch_iset_combine(dst->bits.p, a->bits.p, b->bits.p, op, iset_words(), stream);
    if (e) return set_err(CL_E_DEVICE, "instance set kernels: %s", hipGetErrorString((hipError_t)e));
    if ((rc = iset_time_end())) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    return CL_OK;
  }

  int iset_count(cl_iset* s, int64_t lo, int64_t hi, int64_t* n) {
    int rc = iset_resident(s);
    if (rc) return rc;
    *n = 0;
    if (hi == lo) return CL_OK;
    const hipStream_t stream = dev.stream;
    if ((rc = d_is_count.ensure(1))) return rc;
    HIP_TRY(hipMemsetAsync(d_is_count.p, 0, sizeof(unsigned long long), stream));
    if ((rc = is.mark(0, stream))) return rc;
    const int e = launch_iset_count(s->bits.p, lo, hi, d_is_count.p, stream);
    if (e) return set_err(CL_E_DEVICE, "instance set kernels: %s", hipGetErrorString((hipError_t)e));
    if ((rc = iset_time_end())) return rc;
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, d_is_count.p, sizeof h, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if ((int64_t)h > hi - lo)
      return set_err(CL_E_DEVICE, "instance set: %lld members of %lld instances", (long long)h, (long long)(hi - lo));
    *n = (int64_t)h;
    return CL_OK;
  }

  // The members in [lo, hi), ascending, the first `cap` of them: the words of the range, clipped
  // to it, through the selection's compaction.
  int iset_read(cl_iset* s, int64_t lo, int64_t hi, int64_t* insts, int64_t cap, int64_t* n_match) {
    int rc = iset_resident(s);
    if (rc) return rc;
    *n_match = 0;
    if (hi == lo) return CL_OK;
    const hipStream_t stream = dev.stream;
    SelectParams p{};
    p.base = lo / kWave * kWave;
    p.words = (hi - p.base + kWave - 1) / kWave;
    p.cap = std::min(cap, hi - lo);
    if ((rc = d_sel_bits.ensure((size_t)p.words)) || (rc = compact_scratch(&p, false))) return rc;
    p.bitmap = d_sel_bits.p;
    HIP_TRY(hipMemsetAsync(d_sel_info.p, 0, 4 * sizeof(unsigned long long), stream));
    if ((rc = is.mark(0, stream))) return rc;
    int e = launch_iset_clip(d_sel_bits.p, s->bits.p, lo, hi, stream);
    if (!e) e = launch_select_compact(p, stream);
    if (e) return set_err(CL_E_DEVICE, "instance set kernels: %s", hipGetErrorString((hipError_t)e));
    if ((rc = iset_time_end())) return rc;
    unsigned long long h[4] = {0, 0, 0, 0};
    if ((rc = read_info(d_sel_info.p, hi - lo, "instance set", nullptr, h))) return rc;
    *n_match = (int64_t)h[3];
    const int64_t k = std::min<int64_t>(*n_match, cap);
    if (k > 0) HIP_TRY(hipMemcpy(insts, d_sel_out.p, (size_t)k * sizeof(int64_t), hipMemcpyDeviceToHost));
    return CL_OK;
  }

  // What every cl_*_time waits for before it reads a timer: the marks lie on the sim's stream.
  int marks_done() const {
    HIP_TRY(hipStreamSynchronize(dev.stream));
    return CL_OK;
  }
};

Analytics* analytics_new(cl_sim* sim) { return new Analytics(sim); }
void analytics_delete(Analytics* a) { delete a; }

// The selection's scratch, the bitmaps of the sets alive and their list upload, the crosstab's
// result words, the group-by's representatives and tuples (the statistics and census scratch are
// not counted: DESIGN.md §3).
int64_t analytics_device_bytes(const Analytics* a) {
  int64_t b = a->d_sel_bits.bytes() + a->d_sel_info.bytes() + a->d_sel_bsum.bytes() + a->d_sel_out.bytes() +
              a->d_sel_ticks.bytes();
  for (const cl_iset* s : a->isets) b += s->bits.bytes();
  b += a->d_ord_plane.bytes() + a->d_ord_info.bytes() + a->d_ord_bits.bytes() + a->order.bytes();  // the ordering calls
  return b + a->d_is_list.bytes() + a->d_is_count.bytes() + a->d_xt.bytes() + a->d_gr_first.bytes() +
         a->d_gr_vals.bytes();
}

int sample_args_ok(const cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi) {
  const SimFacts f = sim_facts(sim);
  if (inst_lo < 0 || inst_hi > f.n_inst || inst_lo > inst_hi)
    return set_err(CL_E_INVALID, "instance range out of range");
  if (!f.ran) return set_err(CL_E_STATE, "nothing has run yet: no event was issued");
  if (sid < 0 || sid >= f.n_sids) return set_err(CL_E_INVALID, "snapshot id out of range");
  return CL_OK;
}

}  // namespace clsnap

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
// The set of a conditional call (cl_*_in): given, and this sim's.
static int iset_arg_ok(const cl_sim* sim, const cl_iset* in) {
  if (!in) return set_err(CL_E_INVALID, "null instance set");
  if (in->sim != sim) return set_err(CL_E_INVALID, "the instance set belongs to another sim");
  return CL_OK;
}

// cl_stats_time, cl_crosstab_time, cl_iset_time: the one event pair of timer `t`.
static int pair_time(cl_sim* sim, DevTimer<2> Analytics::*t, const char* none, double* device_ms) {
  SIM_CALL(sim);
  if (!device_ms) return set_err(CL_E_INVALID, "null output");
  const Analytics* a = sim_analytics(sim);
  if (!(a->*t).done) return set_err(CL_E_STATE, "%s", none);
  if (const int rc = a->marks_done()) return rc;
  return (a->*t).ms(0, 1, device_ms);
}

static_assert(sizeof(cl_stats_layout) == sizeof(StatsLayout), "cl_stats_layout mirrors StatsLayout");

static int stats_spec_ok(const cl_stats_spec* spec) {
  if (!spec) return set_err(CL_E_INVALID, "null statistics spec");
  if (spec->tick_bins < 1 || spec->tick_bins > CL_STATS_MAX_TICK_BINS || spec->msg_bins < 1 ||
      spec->msg_bins > CL_STATS_MAX_MSG_BINS)
    return set_err(CL_E_INVALID, "statistics spec: 1 <= tick_bins <= %d, 1 <= msg_bins <= %d", CL_STATS_MAX_TICK_BINS,
                   CL_STATS_MAX_MSG_BINS);
  return CL_OK;
}

static StatsLayout layout_of(const cl_sim* sim, const cl_stats_spec* spec) {
  const SimFacts f = sim_facts(sim);
  return stats_layout(f.n_nodes, f.n_ch, spec->tick_lo, spec->tick_bins, spec->msg_bins);
}

// cl_snapshot_stats, and cl_snapshot_stats_in with its set (`conditional`).
static int stats_call(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, bool conditional, const cl_iset* in,
                      const cl_stats_spec* spec, int64_t* out, int64_t out_words) {
  SIM_CALL(sim);
  // every argument is checked before any device work
  int rc = conditional ? iset_arg_ok(sim, in) : CL_OK;
  if (rc) return rc;
  if ((rc = stats_spec_ok(spec))) return rc;
  if (!out) return set_err(CL_E_INVALID, "null output");
  if ((rc = sample_args_ok(sim, sid, inst_lo, inst_hi))) return rc;
  const StatsLayout L = layout_of(sim, spec);
  if (out_words < L.total_words)
    return set_err(CL_E_LIMIT, "out_words %lld < %lld words of the statistics layout", (long long)out_words,
                   (long long)L.total_words);
  return sim_analytics(sim)->stats(sid, inst_lo, inst_hi, L, out, const_cast<cl_iset*>(in));
}

static int census_spec_ok(const cl_census_spec* spec, const char* what) {
  const int32_t ls = spec->lds_slots;
  if (spec->max_classes < 0 ||
      !(ls == 0 || ls == -1 || (ls >= kCensusMinLdsSlots && ls <= kCensusMaxLdsSlots && (ls & (ls - 1)) == 0)))
    return set_err(CL_E_INVALID, "%s spec: max_classes >= 0; lds_slots 0, -1 or a power of two in [%d, %d]", what,
                   kCensusMinLdsSlots, kCensusMaxLdsSlots);
  return CL_OK;
}

static_assert(sizeof(cl_census_class) == sizeof(CensusEntry) && sizeof(CensusEntry) == 32,
              "cl_census_class mirrors CensusEntry");

// cl_snapshot_census, and cl_snapshot_census_in with its set (`conditional`).
static int census_call(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, bool conditional,
                       const cl_iset* in, const cl_census_spec* spec, cl_census_class* classes, int32_t* class_of,
                       cl_census_info* info) {
  SIM_CALL(sim);
  // every argument is checked before any device work
  if (conditional)
    if (const int rc = iset_arg_ok(sim, in)) return rc;
  if (!spec || !info) return set_err(CL_E_INVALID, "null census spec or info");
  const int32_t ls = spec->lds_slots;
  if (const int rc = census_spec_ok(spec, "census")) return rc;
  if (spec->max_classes > 0 && !classes) return set_err(CL_E_INVALID, "null classes with max_classes > 0");
  if (const int rc = sample_args_ok(sim, sid, inst_lo, inst_hi)) return rc;
  std::vector<CensusEntry> got;
  const int32_t lds_slots = ls == 0 ? kCensusAutoLdsSlots : ls < 0 ? 0 : ls;
  const int rc = sim_analytics(sim)->census(sid, inst_lo, inst_hi, lds_slots, &got, class_of, info,
                                            const_cast<cl_iset*>(in));
  if (rc) return rc;
  info->n_returned = std::min<int64_t>(info->n_classes, spec->max_classes);
  if (info->n_returned > 0) std::memcpy(classes, got.data(), (size_t)info->n_returned * sizeof(cl_census_class));
  return CL_OK;
}

static_assert(sizeof(cl_group_term) == sizeof(GroupTerm) && sizeof(GroupTerm) == 16 &&
                  CL_GROUPS_MAX_TERMS == kGroupsMaxTerms,
              "cl_group_term and CL_GROUPS_MAX_TERMS mirror cl_analytics.h");

// cl_snapshot_groups, and cl_snapshot_groups_in with its set (`conditional`).
static int groups_call(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, bool conditional, const cl_iset* in,
                       const cl_group_term* terms, int32_t n_terms, const cl_census_spec* spec,
                       cl_census_class* groups, int64_t* values, int32_t* group_of, cl_census_info* info) {
  SIM_CALL(sim);
  // every argument is checked before any device work
  if (conditional)
    if (const int rc = iset_arg_ok(sim, in)) return rc;
  if (n_terms < 1 || n_terms > CL_GROUPS_MAX_TERMS || !terms)
    return set_err(CL_E_INVALID, "groups: 1 <= n_terms <= %d, with a term array", CL_GROUPS_MAX_TERMS);
  const SimFacts f = sim_facts(sim);
  for (int32_t k = 0; k < n_terms; ++k) {
    const cl_group_term& z = terms[k];
    if (z.reserved) return set_err(CL_E_INVALID, "groups term %d: non-zero reserved", k);
    if (!quantity_ok(z.field, z.index, SEL_KEY, f.n_nodes, f.n_ch))
      return set_err(CL_E_INVALID, "groups term %d: unknown field %d, or index %d out of range", k, z.field,
                     z.index);
  }
  if (!spec || !info) return set_err(CL_E_INVALID, "null groups spec or info");
  if (const int rc = census_spec_ok(spec, "groups")) return rc;
  if (spec->max_classes > 0 && (!groups || !values))
    return set_err(CL_E_INVALID, "null groups or values with max_classes > 0");
  if (inst_lo < 0 || inst_hi > f.n_inst || inst_lo > inst_hi) return set_err(CL_E_INVALID, "instance range out of range");
  if (inst_hi - inst_lo > ((int64_t)1 << 29)) return set_err(CL_E_LIMIT, "groups of more than 2^29 instances");
  if (!f.ran) return set_err(CL_E_STATE, "nothing has run yet: no event was issued");
  for (int32_t k = 0; k < n_terms; ++k)
    if (terms[k].sid < 0 || terms[k].sid >= f.n_sids)
      return set_err(CL_E_INVALID, "groups term %d: snapshot id out of range", k);
  std::vector<CensusEntry> got;
  const int32_t ls = spec->lds_slots;
  const int32_t lds_slots = ls == 0 ? kCensusAutoLdsSlots : ls < 0 ? 0 : ls;
  const int rc = sim_analytics(sim)->groups(inst_lo, inst_hi, terms, n_terms, lds_slots, spec->max_classes, &got,
                                            values, group_of, info, const_cast<cl_iset*>(in));
  if (rc) return rc;
  info->n_returned = std::min<int64_t>(info->n_classes, spec->max_classes);
  if (info->n_returned > 0) std::memcpy(groups, got.data(), (size_t)info->n_returned * sizeof(cl_census_class));
  return CL_OK;
}

static_assert(sizeof(cl_select_clause) == sizeof(SelectClause) && sizeof(SelectClause) == 32,
              "cl_select_clause mirrors SelectClause");
static_assert(CL_SELECT_MAX_CLAUSES == kSelMaxClauses && CL_SEL_KEY == SEL_KEY && CL_SEL_NOT == kSelNot,
              "CL_SEL_* mirror cl_analytics.h");

// cl_select_instances; cl_select_instances_in with its set (`conditional`); cl_iset_from_clauses
// with the set that takes the matches (`into`: no list, cap 0).
static int select_call(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, bool conditional, const cl_iset* in,
                       const cl_select_clause* clauses, int32_t n_clauses, int64_t* insts, int32_t* ticks,
                       int64_t cap, cl_select_info* info, cl_iset* into) {
  // every argument is checked before any device work
  if (conditional)
    if (const int rc = iset_arg_ok(sim, in)) return rc;
  if (!info) return set_err(CL_E_INVALID, "null select info");
  if (n_clauses < 0 || n_clauses > CL_SELECT_MAX_CLAUSES || (n_clauses > 0 && !clauses))
    return set_err(CL_E_INVALID, "select: 0 <= n_clauses <= %d, with a clause array", CL_SELECT_MAX_CLAUSES);
  const SimFacts f = sim_facts(sim);
  for (int32_t q = 0; q < n_clauses; ++q) {
    const cl_select_clause& z = clauses[q];
    if ((z.flags & ~CL_SEL_NOT) || z.reserved)
      return set_err(CL_E_INVALID, "select clause %d: unknown flag bits or non-zero reserved", q);
    if (!quantity_ok(z.field, z.index, SEL_KEY, f.n_nodes, f.n_ch))
      return set_err(CL_E_INVALID, "select clause %d: unknown field %d, or index %d out of range", q, z.field,
                     z.index);
  }
  if (cap < 0 || (cap > 0 && !insts)) return set_err(CL_E_INVALID, "select: cap >= 0, with an index array when cap > 0");
  if (const int rc = sample_args_ok(sim, sid, inst_lo, inst_hi)) return rc;
  return sim_analytics(sim)->select(sid, inst_lo, inst_hi, clauses, n_clauses, insts, ticks, cap, info,
                                    const_cast<cl_iset*>(in), into);
}

static_assert(sizeof(cl_crosstab_axis) == sizeof(CrosstabAxis) && sizeof(CrosstabAxis) == 32,
              "cl_crosstab_axis mirrors CrosstabAxis");
static_assert(CL_CROSSTAB_MAX_BINS == kXtMaxBins && CL_CROSSTAB_MAX_CELLS == kXtMaxCells && CL_XT_SUM_A == XT_SUM_A &&
                  CL_XT_MIN_A == XT_MIN_A && CL_XT_MAX_A == XT_MAX_A && CL_XT_CELLS == XT_CELLS,
              "CL_CROSSTAB_* and CL_XT_* mirror cl_analytics.h");

static int crosstab_axis_ok(const SimFacts& f, const cl_crosstab_axis* z, const char* name) {
  if (!z) return set_err(CL_E_INVALID, "crosstab: null axis %s", name);
  // (CL_SEL_KEY is not an axis: a hash is not binnable)
  if (!quantity_ok(z->field, z->index, SEL_CH_TOK, f.n_nodes, f.n_ch))
    return set_err(CL_E_INVALID, "crosstab axis %s: field %d is not one of CL_SEL_TICK .. CL_SEL_CH_TOK, or index %d "
                   "out of range", name, z->field, z->index);
  if (z->bins < 1 || z->bins > CL_CROSSTAB_MAX_BINS || z->width < 1)
    return set_err(CL_E_INVALID, "crosstab axis %s: 1 <= bins <= %d, width >= 1", name, CL_CROSSTAB_MAX_BINS);
  return CL_OK;
}

// cl_snapshot_crosstab, and cl_snapshot_crosstab_in with its set (`conditional`).
static int crosstab_call(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, bool conditional, const cl_iset* in,
                         const cl_crosstab_axis* a, const cl_crosstab_axis* b, int64_t* out, int64_t out_words) {
  SIM_CALL(sim);
  // every argument is checked before any device work
  int rc = conditional ? iset_arg_ok(sim, in) : CL_OK;
  if (rc) return rc;
  const SimFacts f = sim_facts(sim);
  if ((rc = crosstab_axis_ok(f, a, "a")) || (rc = crosstab_axis_ok(f, b, "b"))) return rc;
  const int64_t cells = (int64_t)a->bins * (int64_t)b->bins;
  if (cells > CL_CROSSTAB_MAX_CELLS)
    return set_err(CL_E_INVALID, "crosstab: %lld cells, bins_a * bins_b <= %d", (long long)cells, CL_CROSSTAB_MAX_CELLS);
  if (!out) return set_err(CL_E_INVALID, "null output");
  if ((rc = sample_args_ok(sim, a->sid, inst_lo, inst_hi))) return rc;
  if (b->sid < 0 || b->sid >= f.n_sids) return set_err(CL_E_INVALID, "snapshot id out of range");
  if (out_words < CL_XT_CELLS + cells)
    return set_err(CL_E_LIMIT, "out_words %lld < %lld words of the crosstab", (long long)out_words,
                   (long long)(CL_XT_CELLS + cells));
  return sim_analytics(sim)->crosstab(inst_lo, inst_hi, a, b, out, const_cast<cl_iset*>(in));
}

static_assert(CL_ISET_AND == ISET_AND && CL_ISET_OR == ISET_OR && CL_ISET_ANDNOT == ISET_ANDNOT,
              "CL_ISET_* mirror cl_analytics.h");

static_assert(CL_ORDER_DESC == kOrderDesc && CL_ORDER_MAX_K == kOrderMaxK && CL_ORDER_MAX_QUANTILES == kOrderMaxPos &&
                  sizeof(cl_quantile) == 16 && sizeof(cl_order_info) == 32,
              "CL_ORDER_* mirror cl_analytics.h");

// What the three ordering calls share, after the call's own arguments: the set, the term (fields up
// to max_field), the range, its size, a sim that has run something, the term's sid.
static int order_args_ok(const cl_sim* sim, bool conditional, const cl_iset* in, const cl_group_term* term,
                         int32_t max_field, const char* what, int64_t inst_lo, int64_t inst_hi) {
  if (conditional)
    if (const int rc = iset_arg_ok(sim, in)) return rc;
  if (!term) return set_err(CL_E_INVALID, "%s: null term", what);
  const SimFacts f = sim_facts(sim);
  if (term->reserved) return set_err(CL_E_INVALID, "%s term: non-zero reserved", what);
  if (!quantity_ok(term->field, term->index, max_field, f.n_nodes, f.n_ch))
    return set_err(CL_E_INVALID, "%s term: field %d is not one of CL_SEL_TICK .. %s, or index %d out of range", what,
                   term->field, max_field == SEL_KEY ? "CL_SEL_KEY" : "CL_SEL_CH_TOK", term->index);
  if (inst_lo < 0 || inst_hi > f.n_inst || inst_lo > inst_hi) return set_err(CL_E_INVALID, "instance range out of range");
  if (inst_hi - inst_lo > ((int64_t)1 << 29)) return set_err(CL_E_LIMIT, "%s of more than 2^29 instances", what);
  if (!f.ran) return set_err(CL_E_STATE, "nothing has run yet: no event was issued");
  if (term->sid < 0 || term->sid >= f.n_sids) return set_err(CL_E_INVALID, "%s term: snapshot id out of range", what);
  return CL_OK;
}

static int order_k_ok(int32_t flags, int64_t k, const int64_t* insts, const int64_t* values) {
  if (flags & ~CL_ORDER_DESC) return set_err(CL_E_INVALID, "top-k: unknown flag bits");
  if (k < 0 || k > CL_ORDER_MAX_K || (k > 0 && (!insts || !values)))
    return set_err(CL_E_INVALID, "top-k: 0 <= k <= %d, with index and value arrays when k > 0", CL_ORDER_MAX_K);
  return CL_OK;
}

static int order_q_ok(const cl_quantile* q, int32_t n_q, const int64_t* values, const int64_t* ranks) {
  if (n_q < 1 || n_q > CL_ORDER_MAX_QUANTILES || !q || !values || !ranks)
    return set_err(CL_E_INVALID, "quantiles: 1 <= n_q <= %d, with quantile, value and rank arrays",
                   CL_ORDER_MAX_QUANTILES);
  for (int32_t j = 0; j < n_q; ++j)
    if (q[j].den < 1 || q[j].num < 0 || q[j].num > q[j].den)
      return set_err(CL_E_INVALID, "quantile %d: den >= 1 and 0 <= num <= den", j);
  return CL_OK;
}

// cl_snapshot_topk, and cl_snapshot_topk_in with its set (`conditional`).
static int topk_call(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, bool conditional, const cl_iset* in,
                     const cl_group_term* term, int32_t flags, int64_t k, int64_t* insts, int64_t* values,
                     cl_order_info* info) {
  SIM_CALL(sim);
  // every argument is checked before any device work
  if (!info) return set_err(CL_E_INVALID, "top-k: null info");
  int rc = order_k_ok(flags, k, insts, values);
  if (rc || (rc = order_args_ok(sim, conditional, in, term, SEL_CH_TOK, "top-k", inst_lo, inst_hi))) return rc;
  return sim_analytics(sim)->topk(inst_lo, inst_hi, term, flags, k, insts, values, info, const_cast<cl_iset*>(in));
}

static int quantiles_call(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, bool conditional, const cl_iset* in,
                          const cl_group_term* term, const cl_quantile* q, int32_t n_q, int64_t* values,
                          int64_t* ranks, cl_order_info* info) {
  SIM_CALL(sim);
  if (!info) return set_err(CL_E_INVALID, "quantiles: null info");
  int rc = order_q_ok(q, n_q, values, ranks);
  if (rc || (rc = order_args_ok(sim, conditional, in, term, SEL_CH_TOK, "quantiles", inst_lo, inst_hi))) return rc;
  return sim_analytics(sim)->quantiles(inst_lo, inst_hi, term, q, n_q, values, ranks, info, const_cast<cl_iset*>(in));
}

static int values_call(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, bool conditional, const cl_iset* in,
                       const cl_group_term* term, int64_t* values, uint8_t* in_sample) {
  SIM_CALL(sim);
  if (!values && inst_hi > inst_lo) return set_err(CL_E_INVALID, "values: null output");
  if (const int rc = order_args_ok(sim, conditional, in, term, SEL_KEY, "values", inst_lo, inst_hi)) return rc;
  return sim_analytics(sim)->values_of(inst_lo, inst_hi, term, values, in_sample, const_cast<cl_iset*>(in));
}

static int iset_range_ok(const cl_iset* s, int64_t lo, int64_t hi) {
  if (lo < 0 || hi > sim_facts(s->sim).n_inst || lo > hi) return set_err(CL_E_INVALID, "instance range out of range");
  return CL_OK;
}

extern "C" {

int cl_stats_layout_of(const cl_sim* sim, const cl_stats_spec* spec, cl_stats_layout* out) {
  SIM_CALL(sim, false);
  if (!out) return set_err(CL_E_INVALID, "null output");
  int rc = stats_spec_ok(spec);
  if (rc) return rc;
  const StatsLayout L = layout_of(sim, spec);
  std::memcpy(out, &L, sizeof L);
  return CL_OK;
}

int cl_snapshot_stats(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, const cl_stats_spec* spec,
                      int64_t* out, int64_t out_words) {
  return stats_call(sim, sid, inst_lo, inst_hi, false, nullptr, spec, out, out_words);
}

int cl_snapshot_stats_in(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, const cl_iset* in,
                         const cl_stats_spec* spec, int64_t* out, int64_t out_words) {
  return stats_call(sim, sid, inst_lo, inst_hi, true, in, spec, out, out_words);
}

int cl_stats_time(cl_sim* sim, double* device_ms) {
  return pair_time(sim, &Analytics::st, "no statistics call has run", device_ms);
}

int cl_snapshot_census(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, const cl_census_spec* spec,
                       cl_census_class* classes, int32_t* class_of, cl_census_info* info) {
  return census_call(sim, sid, inst_lo, inst_hi, false, nullptr, spec, classes, class_of, info);
}

int cl_snapshot_census_in(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, const cl_iset* in,
                          const cl_census_spec* spec, cl_census_class* classes, int32_t* class_of,
                          cl_census_info* info) {
  return census_call(sim, sid, inst_lo, inst_hi, true, in, spec, classes, class_of, info);
}

int cl_census_time(cl_sim* sim, double* device_ms) {
  SIM_CALL(sim);
  if (!device_ms) return set_err(CL_E_INVALID, "null output");
  const Analytics* a = sim_analytics(sim);
  if (!a->cs.done) return set_err(CL_E_STATE, "no census call has run");
  if (const int rc = a->marks_done()) return rc;
  double sum = 0;
  for (int q = 0; q < a->cs.done; ++q) {  // key pass, gather, class_of: the host's sort lies between
    double ms = 0;
    if (const int rc = a->cs.ms(2 * q, 2 * q + 1, &ms)) return rc;
    sum += ms;
  }
  *device_ms = sum;
  return CL_OK;
}

int cl_snapshot_groups(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_group_term* terms, int32_t n_terms,
                       const cl_census_spec* spec, cl_census_class* groups, int64_t* values, int32_t* group_of,
                       cl_census_info* info) {
  return groups_call(sim, inst_lo, inst_hi, false, nullptr, terms, n_terms, spec, groups, values, group_of, info);
}

int cl_snapshot_groups_in(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_iset* in, const cl_group_term* terms,
                          int32_t n_terms, const cl_census_spec* spec, cl_census_class* groups, int64_t* values,
                          int32_t* group_of, cl_census_info* info) {
  return groups_call(sim, inst_lo, inst_hi, true, in, terms, n_terms, spec, groups, values, group_of, info);
}

int cl_groups_stage_times(cl_sim* sim, double* stage_ms) {
  SIM_CALL(sim);
  if (!stage_ms) return set_err(CL_E_INVALID, "null output");
  const Analytics* a = sim_analytics(sim);
  if (!a->gr.done) return set_err(CL_E_STATE, "no groups call has run");
  int rc = a->marks_done();
  if (rc) return rc;
  for (int q = 0; q < 5; ++q) stage_ms[q] = 0;
  // table initialisation, key pass, gather, group_of (the host's sort lies between), values
  if ((rc = a->gr.ms(0, 6, &stage_ms[0])) || (rc = a->gr.ms(6, 1, &stage_ms[1]))) return rc;
  if (a->gr.done >= 2 && (rc = a->gr.ms(2, 3, &stage_ms[2]))) return rc;
  if (a->gr.done >= 3 && (rc = a->gr.ms(4, 5, &stage_ms[3]))) return rc;
  if (a->grv.done && (rc = a->grv.ms(0, 1, &stage_ms[4]))) return rc;
  return CL_OK;
}

int cl_groups_time(cl_sim* sim, double* device_ms) {
  if (!device_ms) return set_err(CL_E_INVALID, "null output");
  double ms[5];
  const int rc = cl_groups_stage_times(sim, ms);
  if (rc) return rc;
  *device_ms = ms[0] + ms[1] + ms[2] + ms[3] + ms[4];
  return CL_OK;
}

uint64_t cl_group_key(const int64_t* values, int32_t n) {
  uint64_t h = group_key_seed(n);
  for (int32_t k = 0; k < n && values; ++k) h = group_key_fold(h, values[k]);
  return h;
}

int cl_select_instances(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, const cl_select_clause* clauses,
                        int32_t n_clauses, int64_t* insts, int32_t* ticks, int64_t cap, cl_select_info* info) {
  SIM_CALL(sim);
  return select_call(sim, sid, inst_lo, inst_hi, false, nullptr, clauses, n_clauses, insts, ticks, cap, info, nullptr);
}

int cl_select_instances_in(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, const cl_iset* in,
                           const cl_select_clause* clauses, int32_t n_clauses, int64_t* insts, int32_t* ticks,
                           int64_t cap, cl_select_info* info) {
  SIM_CALL(sim);
  return select_call(sim, sid, inst_lo, inst_hi, true, in, clauses, n_clauses, insts, ticks, cap, info, nullptr);
}

int cl_select_stage_times(cl_sim* sim, double* evaluate_ms, double* compact_ms) {
  SIM_CALL(sim);
  const Analytics* an = sim_analytics(sim);
  if (!an->sel.done) return set_err(CL_E_STATE, "no select call has run");
  double a = 0, b = 0;
  int rc;
  if ((rc = an->marks_done()) || (rc = an->sel.ms(0, 1, &a)) || (rc = an->sel.ms(1, 2, &b))) return rc;
  if (evaluate_ms) *evaluate_ms = a;
  if (compact_ms) *compact_ms = b;
  return CL_OK;
}

int cl_select_time(cl_sim* sim, double* device_ms) {
  if (!device_ms) return set_err(CL_E_INVALID, "null output");
  double a = 0, b = 0;
  const int rc = cl_select_stage_times(sim, &a, &b);
  if (rc) return rc;
  *device_ms = a + b;
  return CL_OK;
}

int cl_snapshot_crosstab(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_crosstab_axis* a,
                         const cl_crosstab_axis* b, int64_t* out, int64_t out_words) {
  return crosstab_call(sim, inst_lo, inst_hi, false, nullptr, a, b, out, out_words);
}

int cl_snapshot_crosstab_in(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_iset* in, const cl_crosstab_axis* a,
                            const cl_crosstab_axis* b, int64_t* out, int64_t out_words) {
  return crosstab_call(sim, inst_lo, inst_hi, true, in, a, b, out, out_words);
}

int cl_crosstab_time(cl_sim* sim, double* device_ms) {
  return pair_time(sim, &Analytics::xt, "no crosstab call has run", device_ms);
}

// ---- instance sets ------------------------------------------------------------------------------
int cl_iset_from_clauses(cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi, const cl_select_clause* clauses,
                         int32_t n_clauses, cl_iset** out, cl_select_info* info) {
  SIM_CALL(sim);
  if (!out) return set_err(CL_E_INVALID, "null instance set output");
  Analytics* a = sim_analytics(sim);
  cl_iset* s = a->iset_new();
  const int rc = select_call(sim, sid, inst_lo, inst_hi, false, nullptr, clauses, n_clauses, nullptr, nullptr, 0, info, s);
  if (rc) {
    a->iset_delete(s);
    return rc;
  }
  *out = s;
  return CL_OK;
}

int cl_iset_from_list(cl_sim* sim, const int64_t* insts, int64_t n, cl_iset** out) {
  SIM_CALL(sim);
  if (!out || n < 0 || (n > 0 && !insts)) return set_err(CL_E_INVALID, "instance list or set output out of range");
  const SimFacts f = sim_facts(sim);
  for (int64_t r = 0; r < n; ++r)
    if (insts[r] < 0 || insts[r] >= f.n_inst)
      return set_err(CL_E_INVALID, "instance list entry %lld: instance %lld out of range", (long long)r,
                     (long long)insts[r]);
  Analytics* a = sim_analytics(sim);
  cl_iset* s = a->iset_new();
  s->pending.assign(insts, insts + n);
  // the scatter runs now when the sim already has its device, else with the set's first device use
  if (f.dev_ready) {
    const int rc = a->iset_resident(s, true);
    if (rc) {
      a->iset_delete(s);
      return rc;
    }
  }
  *out = s;
  return CL_OK;
}

int cl_iset_combine(cl_iset* dst, const cl_iset* a, const cl_iset* b, int32_t op) {
  if (!dst || !a || !b) return set_err(CL_E_INVALID, "null instance set");
  cl_sim* sim = dst->sim;
  SIM_CALL(sim);
  if (a->sim != sim || b->sim != sim) return set_err(CL_E_INVALID, "the instance sets belong to different sims");
  if (op < 0 || op >= ISET_NUM_OPS) return set_err(CL_E_INVALID, "unknown instance set operation %d", op);
  return sim_analytics(sim)->iset_combine(dst, const_cast<cl_iset*>(a), const_cast<cl_iset*>(b), op);
}

int cl_iset_count(cl_iset* set, int64_t inst_lo, int64_t inst_hi, int64_t* n) {
  if (!set) return set_err(CL_E_INVALID, "null instance set");
  cl_sim* sim = set->sim;
  SIM_CALL(sim);
  if (!n) return set_err(CL_E_INVALID, "null output");
  if (const int rc = iset_range_ok(set, inst_lo, inst_hi)) return rc;
  return sim_analytics(sim)->iset_count(set, inst_lo, inst_hi, n);
}

int cl_iset_read(cl_iset* set, int64_t inst_lo, int64_t inst_hi, int64_t* insts, int64_t cap, int64_t* n_match) {
  if (!set) return set_err(CL_E_INVALID, "null instance set");
  cl_sim* sim = set->sim;
  SIM_CALL(sim);
  if (!n_match) return set_err(CL_E_INVALID, "null output");
  if (cap < 0 || (cap > 0 && !insts)) return set_err(CL_E_INVALID, "iset read: cap >= 0, with an index array when cap > 0");
  if (const int rc = iset_range_ok(set, inst_lo, inst_hi)) return rc;
  return sim_analytics(sim)->iset_read(set, inst_lo, inst_hi, insts, cap, n_match);
}

int cl_iset_destroy(cl_iset* set) {
  if (!set) return CL_OK;
  cl_sim* sim = set->sim;
  SIM_CALL(sim);
  sim_analytics(sim)->iset_delete(set);
  return CL_OK;
}

int cl_iset_time(cl_sim* sim, double* device_ms) {
  return pair_time(sim, &Analytics::is, "no instance set kernel has run", device_ms);
}

// ---- ordering: top-k, quantiles, values -----------------------------------------------------------
int cl_snapshot_topk(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_group_term* term, int32_t flags,
                     int64_t k, int64_t* insts, int64_t* values, cl_order_info* info) {
  return topk_call(sim, inst_lo, inst_hi, false, nullptr, term, flags, k, insts, values, info);
}

int cl_snapshot_topk_in(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_iset* in, const cl_group_term* term,
                        int32_t flags, int64_t k, int64_t* insts, int64_t* values, cl_order_info* info) {
  return topk_call(sim, inst_lo, inst_hi, true, in, term, flags, k, insts, values, info);
}

int cl_snapshot_quantiles(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_group_term* term,
                          const cl_quantile* q, int32_t n_q, int64_t* values, int64_t* ranks, cl_order_info* info) {
  return quantiles_call(sim, inst_lo, inst_hi, false, nullptr, term, q, n_q, values, ranks, info);
}

int cl_snapshot_quantiles_in(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_iset* in,
                             const cl_group_term* term, const cl_quantile* q, int32_t n_q, int64_t* values,
                             int64_t* ranks, cl_order_info* info) {
  return quantiles_call(sim, inst_lo, inst_hi, true, in, term, q, n_q, values, ranks, info);
}

int cl_snapshot_values(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_group_term* term, int64_t* values,
                       uint8_t* in_sample) {
  return values_call(sim, inst_lo, inst_hi, false, nullptr, term, values, in_sample);
}

int cl_snapshot_values_in(cl_sim* sim, int64_t inst_lo, int64_t inst_hi, const cl_iset* in, const cl_group_term* term,
                          int64_t* values, uint8_t* in_sample) {
  return values_call(sim, inst_lo, inst_hi, true, in, term, values, in_sample);
}

int cl_order_stage_times(cl_sim* sim, double* stage_ms) {
  SIM_CALL(sim);
  if (!stage_ms) return set_err(CL_E_INVALID, "null output");
  const Analytics* a = sim_analytics(sim);
  if (!a->ord.done) return set_err(CL_E_STATE, "no top-k, quantiles or values call has run");
  int rc = a->marks_done();
  if (rc) return rc;
  // the value walk, the select passes, the compaction
  if ((rc = a->ord.ms(0, 1, &stage_ms[0])) || (rc = a->order.stage_ms(&stage_ms[1], &stage_ms[2]))) return rc;
  return CL_OK;
}

int cl_order_time(cl_sim* sim, double* device_ms) {
  if (!device_ms) return set_err(CL_E_INVALID, "null output");
  double ms[3];
  const int rc = cl_order_stage_times(sim, ms);
  if (rc) return rc;
  *device_ms = ms[0] + ms[1] + ms[2];
  return CL_OK;
}

int cl_order_plane_device(int32_t device, const int64_t* values, const uint8_t* in_sample, int64_t n, int32_t flags,
                          int64_t k, int64_t* insts, int64_t* vals, int64_t* n_returned, const cl_quantile* q,
                          int32_t n_q, int64_t* q_values, int64_t* q_ranks, double* device_ms) {
  if (n < 1 || n > ((int64_t)1 << 29) || !values || !n_returned)
    return set_err(CL_E_INVALID, "order plane: 1 <= n <= 2^29 values, with an output for n_returned");
  int rc = order_k_ok(flags, k, insts, vals);
  if (rc || (n_q != 0 && (rc = order_q_ok(q, n_q, q_values, q_ranks)))) return rc;
  hipDeviceProp_t prop;
  if ((rc = open_gfx950(device, &prop))) return rc;
  // the plane as the value walk leaves it: the bitmap, the sample's size, minimum and maximum
  std::vector<unsigned long long> bits((size_t)((n + kWave - 1) / kWave), 0);
  int64_t sample = 0;
  long long vmin = INT64_MAX, vmax = INT64_MIN;
  for (int64_t i = 0; i < n; ++i) {
    if (in_sample && !in_sample[i]) continue;
    bits[(size_t)(i >> 6)] |= 1ULL << (i & 63);
    ++sample;
    vmin = std::min<long long>(vmin, values[i]);
    vmax = std::max<long long>(vmax, values[i]);
  }
  struct Scratch {  // (the buffers and the engine free themselves on every return path)
    DevBuf<long long> plane;
    DevBuf<unsigned long long> bits;
    OrderEngine order;
    hipStream_t stream = nullptr;
    ~Scratch() {
      if (stream) (void)hipStreamDestroy(stream);
    }
  } s;
  if ((rc = s.plane.ensure((size_t)n)) || (rc = s.bits.ensure(bits.size()))) return rc;
  HIP_TRY(hipMemcpy(s.plane.p, values, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s.bits.p, bits.data(), bits.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
  HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  const int32_t n_cus = prop.multiProcessorCount;
  double total = 0, a = 0, b = 0;
  OrderEngine::Plane pl{s.plane.p, s.bits.p, n, 0, 0, vmin, vmax, (flags & CL_ORDER_DESC) != 0};
  *n_returned = std::min(k, sample);
  if (*n_returned > 0) {
    if ((rc = s.order.topk(pl, *n_returned, insts, vals, s.stream, n_cus)) || (rc = s.order.stage_ms(&a, &b))) return rc;
    total += a + b;
  }
  for (int32_t j = 0; j < n_q; ++j) q_ranks[j] = sample ? quantile_rank(q[j], sample) : -1;
  if (n_q > 0 && sample > 0) {
    pl.desc = 0;  // (quantiles are positions of the ascending order)
    if ((rc = s.order.at_ranks(pl, q_ranks, n_q, q_values, s.stream, n_cus)) || (rc = s.order.stage_ms(&a, &b)))
      return rc;
    total += a + b;
  }
  if (device_ms) *device_ms = total;
  HIP_TRY(hipStreamSynchronize(s.stream));
  return CL_OK;
}

}  // extern "C"
