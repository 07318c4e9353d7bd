// cg_readout.cpp -- the graph engine's device-side readouts behind include/clgraph.h: the per-snapshot
// summary table (cg_table.hip), the sparse packed collect (cg_sparse.hip), the marker-wave profile and
// tree (cg_wave.hip) and the node and channel profile over a snapshot range (cg_profile.hip).  Each is written against the view of a cl_graph that cg_host.h gives and owns what it allocates.
#include <algorithm>
#include <vector>

#include "cg_host.h"

using namespace clsnap;

// Scratch of one chunk of sids: the wave's 8-byte pairs over all nodes, the tree's int32 planes
// over the owned ones.  256 MiB holds 32 sids of a 2^20-node graph and every sid of a 20,000-node
// x 256-snapshot run at once, and is small next to the planes of either run; a graph whose single
// sid needs more takes one sid per chunk.
constexpr size_t kWaveScratchBytes = (size_t)256 << 20;
constexpr int32_t kWaveMaxRounds = 32;

// sids per chunk of scratch: as many as the budget holds, at least one, at most all
static size_t chunk_sids(size_t budget, size_t bytes_per_sid, size_t ns) {
  return std::min(ns, std::max<size_t>(1, budget / std::max<size_t>(1, bytes_per_sid)));
}

struct clsnap::Readouts {
  // summary table (cl_graph_snapshot_table): the device rows, the events around the latest call's kernels
  DevBuf<long long> d_table;
  GraphTimer<2> tb;
  // sparse packed collect (cl_graph_collect_sparse): per-(sid, tile) offsets, per-sid totals,
  // the head the host reads between scan and write (row_offsets, message offsets, complete),
  // the packed outputs, and the events around the scan ([0], [1]) and the write ([2], [3]);
  // done: the pairs of the latest call that completed
  DevBuf<ulonglong2> d_sp_tiles, d_sp_rows;
  DevBuf<long long> d_sp_head;
  DevBuf<int32_t> d_sp_chan, d_sp_cnt, d_sp_msg, d_sp_tok;
  GraphTimer<4> sp;
  // marker-wave profile and tree (cl_graph_snapshot_wave / _tree): the device rows, the origins
  // (or initiator ranks) of the rows, the doubling round's flag, and the scratch of one chunk of
  // sids -- the {ancestor, hops} pairs of the wave, the packed planes of the tree; the events
  // around the latest wave call's kernels and its doubling rounds
  DevBuf<long long> d_wv_rows, d_wv_org;
  DevBuf<int32_t> d_wv_flag;
  DevBuf<unsigned long long> d_wv_scratch;
  GraphTimer<2> wv;
  int32_t wv_rounds = 0;
  size_t wv_budget = kWaveScratchBytes;  // bytes of scratch per chunk of sids (cl_graph_set_wave_scratch)
  // node and channel profile (cl_graph_snapshot_profile): the mask, the used list and the used flags
  // ([3][ns]); the origins as given and as used ([2][ns]); the head and histogram; the accumulator
  // planes of the owned in-positions; the node rows; the channel tiles' entry offsets; the entries;
  // the events around the reduction ([0], [1]) and around the node pass and the fill ([2], [3]);
  // done: the pairs of the latest call that completed
  DevBuf<int32_t> d_pf_i32;
  DevBuf<long long> d_pf_org, d_pf_head, d_pf_rows;
  DevBuf<unsigned long long> d_pf_acc, d_pf_tiles;
  DevBuf<cl_graph_profile_entry> d_pf_ent;
  GraphTimer<4> pf;
  int32_t pf_slices = 0;  // slices of the used list (cl_graph_set_profile_slices), 0: automatic
};

Readouts* clsnap::readouts_new() { return new Readouts(); }
void clsnap::readouts_delete(Readouts* r) { delete r; }

// What cl_graph_device_bytes counts of the readouts: the wave's pairs (or the tree's planes), rows
// and origins, and the whole scratch of the range profile.  Known gap: the table's rows, the whole
// sparse scratch and the wave's round flag are not counted.
int64_t clsnap::readouts_device_bytes(const Readouts* r) {
  return (int64_t)(r->d_wv_scratch.bytes() + r->d_wv_rows.bytes() + r->d_wv_org.bytes() + r->d_pf_i32.bytes() +
                   r->d_pf_org.bytes() + r->d_pf_head.bytes() + r->d_pf_rows.bytes() + r->d_pf_acc.bytes() +
                   r->d_pf_tiles.bytes() + r->d_pf_ent.bytes());
}

extern "C" {

int cl_graph_snapshot_table(cl_graph* g, int32_t sid_lo, int32_t sid_hi, cl_graph_snap_row* rows) {
  GRAPH_CALL(g);
  static_assert(sizeof(cl_graph_snap_row) == 16 * sizeof(int64_t), "cl_graph_snap_row is 16 x int64");
  int rc = sid_range_ok(g, sid_lo, sid_hi);
  if (rc) return rc;
  const int32_t ns = sid_hi - sid_lo;
  if (ns == 0) return CL_OK;
  if (!rows) return set_err(CL_E_INVALID, "null output");
  GraphView v;
  if ((rc = graph_view(g, &v))) return rc;
  Readouts* r = graph_readouts(g);
  if ((rc = r->d_table.ensure((size_t)ns * 16))) return rc;
  r->tb.done = 0;
  if ((rc = r->tb.mark(0, v.stream))) return rc;
  if ((rc = launch_err(cg_launch_table(*v.P, v.d_in_ch, v.k_lo, v.k_hi, sid_lo, ns, r->d_table.p, v.n_cus, v.stream)))) return rc;
  if ((rc = r->tb.mark(1, v.stream))) return rc;
  HIP_TRY(hipMemcpyAsync(rows, r->d_table.p, (size_t)ns * sizeof(cl_graph_snap_row), hipMemcpyDeviceToHost, v.stream));
  HIP_TRY(hipStreamSynchronize(v.stream));
  r->tb.done = 1;
  return CL_OK;
}

int cl_graph_table_time(cl_graph* g, double* ms) {
  GRAPH_CALL(g);
  if (!ms) return set_err(CL_E_INVALID, "null output");
  const Readouts* r = graph_readouts(g);
  if (!r->tb.done) return set_err(CL_E_STATE, "no snapshot table has been computed");
  return r->tb.ms(0, 1, ms);
}

// ---- marker-wave profile and marker tree (cg_wave.hip) ------------------------------------
int cl_graph_set_wave_scratch(cl_graph* g, int64_t bytes) {
  GRAPH_CALL(g);
  if (bytes < 0) return set_err(CL_E_INVALID, "negative scratch budget");
  graph_readouts(g)->wv_budget = bytes ? (size_t)bytes : kWaveScratchBytes;  // (0: the default)
  return CL_OK;
}

int cl_graph_snapshot_wave(cl_graph* g, int32_t sid_lo, int32_t sid_hi, const cl_graph_wave_spec* spec,
                           const int64_t* origins, int64_t* out, int64_t out_words) {
  GRAPH_CALL(g);
  static_assert(sizeof(cl_graph_wave_spec) == 4 * sizeof(int32_t), "cl_graph_wave_spec is 4 x int32");
  if (!spec || !out) return set_err(CL_E_INVALID, "null %s", !spec ? "spec" : "output");
  if (spec->lat_bins < 1 || spec->lat_bins > CL_GRAPH_WAVE_MAX_BINS || spec->lat_width < 1 || spec->depth_bins < 0 ||
      spec->depth_bins > CL_GRAPH_WAVE_MAX_BINS || spec->reserved)
    return set_err(CL_E_INVALID, "wave spec: lat_bins %d (1..%d), lat_width %d (>= 1), depth_bins %d (0..%d), reserved %d",
                spec->lat_bins, CL_GRAPH_WAVE_MAX_BINS, spec->lat_width, spec->depth_bins, CL_GRAPH_WAVE_MAX_BINS,
                spec->reserved);
  int rc = sid_range_ok(g, sid_lo, sid_hi);
  if (rc) return rc;
  const int32_t ns = sid_hi - sid_lo, rw = CL_WV_HEAD + spec->lat_bins + spec->depth_bins;
  if (out_words < (int64_t)ns * rw)
    return set_err(CL_E_LIMIT, "%d rows of %d words exceed out_words %lld", ns, rw, (long long)out_words);
  const bool part = graph_facts(g).part;
  if (part && spec->depth_bins > 0)
    return set_err(CL_E_STATE, "a partitioned run has no device depth: the parents' records live on other devices");
  if (part && !origins) return set_err(CL_E_STATE, "a partitioned run needs the origins: only the initiator's owner knows the start");
  if (ns == 0) return CL_OK;
  GraphView v;
  if ((rc = graph_view(g, &v))) return rc;
  Readouts* r = graph_readouts(g);
  const GParams& P = *v.P;
  const bool depth = spec->depth_bins > 0;
  const size_t nsz = (size_t)ns, n = (size_t)P.n;
  const size_t cs = chunk_sids(r->wv_budget, n * sizeof(unsigned long long), nsz);  // sids per chunk of pairs
  if ((rc = r->d_wv_rows.ensure(nsz * (size_t)rw)) || (rc = r->d_wv_org.ensure(nsz)) || (rc = r->d_wv_flag.ensure(1))) return rc;
  if (depth && (rc = r->d_wv_scratch.ensure(cs * n))) return rc;
  // the origins, or the initiators' ranks
  std::vector<long long> org(nsz);
  if (origins) std::copy(origins, origins + ns, org.begin());
  else graph_initiators(g, sid_lo, sid_hi, org.data());
  HIP_TRY(hipMemcpyAsync(r->d_wv_org.p, org.data(), nsz * sizeof(long long), hipMemcpyHostToDevice, v.stream));
  HIP_TRY(hipStreamSynchronize(v.stream));  // (`org` is a local)
  const int32_t user = origins ? 1 : 0;
  r->wv.done = 0;
  r->wv_rounds = 0;
  if ((rc = r->wv.mark(0, v.stream))) return rc;
  if ((rc = launch_err(cg_launch_wave_init(P, r->d_wv_org.p, user, sid_lo, ns, rw, r->d_wv_rows.p, v.stream)))) return rc;
  if (!depth) {
    if ((rc = launch_err(cg_launch_wave(P, sid_lo, ns, rw, spec->lat_bins, spec->lat_width, 0, user, nullptr,
                                        r->d_wv_rows.p, v.n_cus, v.stream))))
      return rc;
  } else {
    for (size_t c0 = 0; c0 < nsz; c0 += cs) {
      const int32_t cn = (int32_t)std::min(cs, nsz - c0), sid0 = sid_lo + (int32_t)c0;
      if ((rc = launch_err(cg_launch_wave_link(P, sid0, cn, r->d_wv_scratch.p, v.stream)))) return rc;
      int32_t rounds = 0, moved = 1;
      while (moved && rounds < kWaveMaxRounds) {  // until a round moves no pair
        HIP_TRY(hipMemsetAsync(r->d_wv_flag.p, 0, sizeof(int32_t), v.stream));
        if ((rc = launch_err(cg_launch_wave_jump(P, cn, r->d_wv_scratch.p, r->d_wv_flag.p, v.stream)))) return rc;
        HIP_TRY(hipMemcpyAsync(&moved, r->d_wv_flag.p, sizeof moved, hipMemcpyDeviceToHost, v.stream));
        HIP_TRY(hipStreamSynchronize(v.stream));
        ++rounds;
      }
      r->wv_rounds = std::max(r->wv_rounds, rounds);
      if ((rc = launch_err(cg_launch_wave(P, sid0, cn, rw, spec->lat_bins, spec->lat_width, spec->depth_bins, user,
                                          r->d_wv_scratch.p, r->d_wv_rows.p + c0 * (size_t)rw, v.n_cus, v.stream))))
        return rc;
    }
  }
  if ((rc = r->wv.mark(1, v.stream))) return rc;
  HIP_TRY(hipMemcpyAsync(out, r->d_wv_rows.p, nsz * (size_t)rw * sizeof(int64_t), hipMemcpyDeviceToHost, v.stream));
  HIP_TRY(hipStreamSynchronize(v.stream));
  r->wv.done = 1;
  return CL_OK;
}

int cl_graph_wave_time(cl_graph* g, double* ms, int32_t* rounds) {
  GRAPH_CALL(g);
  if (!ms) return set_err(CL_E_INVALID, "null output");
  const Readouts* r = graph_readouts(g);
  if (!r->wv.done) return set_err(CL_E_STATE, "no snapshot wave has been computed");
  if (rounds) *rounds = r->wv_rounds;
  return r->wv.ms(0, 1, ms);
}

int cl_graph_snapshot_tree(cl_graph* g, int32_t sid_lo, int32_t sid_hi, int32_t* parent, int32_t* tick) {
  GRAPH_CALL(g);
  if (!parent) return set_err(CL_E_INVALID, "null output");
  int rc = sid_range_ok(g, sid_lo, sid_hi);
  if (rc) return rc;
  const int32_t ns = sid_hi - sid_lo;
  if (ns == 0) return CL_OK;
  GraphView v;
  if ((rc = graph_view(g, &v))) return rc;
  Readouts* r = graph_readouts(g);
  const GParams& P = *v.P;
  const size_t nsz = (size_t)ns, width = (size_t)(P.part_hi - P.part_lo), planes = tick ? 2 : 1;
  if (width == 0) return CL_OK;
  const size_t cs = chunk_sids(r->wv_budget, width * planes * sizeof(int32_t), nsz);  // sids per chunk of packed planes
  if ((rc = r->d_wv_scratch.ensure((cs * width * planes + 1) / 2))) return rc;
  int32_t* d_parent = reinterpret_cast<int32_t*>(r->d_wv_scratch.p);
  int32_t* d_tick = tick ? d_parent + cs * width : nullptr;
  for (size_t c0 = 0; c0 < nsz; c0 += cs) {  // (stream order: a chunk's copies end before the next pack)
    const size_t cn = std::min(cs, nsz - c0);
    if ((rc = launch_err(cg_launch_wave_pack(P, sid_lo + (int32_t)c0, (int32_t)cn, d_parent, d_tick, v.stream)))) return rc;
    HIP_TRY(hipMemcpyAsync(parent + c0 * width, d_parent, cn * width * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
    if (tick) HIP_TRY(hipMemcpyAsync(tick + c0 * width, d_tick, cn * width * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
  }
  HIP_TRY(hipStreamSynchronize(v.stream));
  return CL_OK;
}

int cl_graph_collect_sparse(cl_graph* g, int32_t sid_lo, int32_t sid_hi, int32_t* complete, int64_t* row_offsets,
                            int32_t* ent_channel, int32_t* ent_count, int64_t ent_cap, int32_t* msg_tokens,
                            int64_t msg_cap, int32_t* tokens, cl_graph_sparse_info* info) {
  GRAPH_CALL(g);
  static_assert(sizeof(cl_graph_sparse_info) == 8 * sizeof(int64_t), "cl_graph_sparse_info is 8 x int64");
  if (!info) return set_err(CL_E_INVALID, "null info");
  int rc = sid_range_ok(g, sid_lo, sid_hi);
  if (rc) return rc;
  if (ent_cap < 0 || msg_cap < 0) return set_err(CL_E_INVALID, "negative capacity");
  if (ent_cap > 0 && (!ent_channel || !ent_count)) return set_err(CL_E_INVALID, "null entry arrays with ent_cap > 0");
  const int32_t ns = sid_hi - sid_lo;
  const GraphFacts f = graph_facts(g);
  *info = cl_graph_sparse_info{};
  info->node_lo = f.node_lo;
  info->node_hi = f.node_hi;
  if (ns == 0) {
    if (row_offsets) row_offsets[0] = 0;
    return CL_OK;
  }
  GraphView v;
  if ((rc = graph_view(g, &v))) return rc;
  Readouts* r = graph_readouts(g);
  const GParams& P = *v.P;
  const size_t tiles = (size_t)cg_sparse_tiles(P.e), nsz = (size_t)ns;
  // head: row_offsets[ns + 1], message offsets[ns + 1], then complete[ns] as int32
  const size_t head_words = 2 * (nsz + 1) + (nsz + 1) / 2;
  if ((rc = r->d_sp_tiles.ensure(nsz * tiles)) || (rc = r->d_sp_rows.ensure(nsz)) || (rc = r->d_sp_head.ensure(head_words)))
    return rc;
  long long* d_off = r->d_sp_head.p;
  long long* d_moff = d_off + (nsz + 1);
  int32_t* d_complete = reinterpret_cast<int32_t*>(d_moff + (nsz + 1));
  r->sp.done = 0;
  if ((rc = r->sp.mark(0, v.stream))) return rc;
  if ((rc = launch_err(cg_launch_sparse_scan(P, sid_lo, ns, r->d_sp_tiles.p, r->d_sp_rows.p, d_off, d_moff, d_complete, v.stream))))
    return rc;
  if ((rc = r->sp.mark(1, v.stream))) return rc;
  // the totals decide the sizes: the host reads the head between scan and write
  std::vector<long long> head(head_words);
  HIP_TRY(hipMemcpyAsync(head.data(), d_off, head_words * sizeof(long long), hipMemcpyDeviceToHost, v.stream));
  HIP_TRY(hipStreamSynchronize(v.stream));
  r->sp.done = 1;
  const int32_t* h_complete = reinterpret_cast<const int32_t*>(head.data() + 2 * (nsz + 1));
  const int64_t n_entries = head[nsz], n_msgs = head[2 * nsz + 1];
  info->n_sids = ns;
  for (int32_t i = 0; i < ns; ++i) info->n_complete += h_complete[i] != 0;
  info->n_entries = n_entries;
  info->n_msgs = n_msgs;
  info->unit_payloads = v.hist == 0 ? 1 : 0;
  if (complete) std::copy(h_complete, h_complete + ns, complete);
  if (row_offsets) std::copy(head.begin(), head.begin() + (ns + 1), row_offsets);
  if (n_entries > ent_cap) return set_err(CL_E_LIMIT, "%lld entries exceed ent_cap %lld", (long long)n_entries, (long long)ent_cap);
  if (msg_tokens && n_msgs > msg_cap)
    return set_err(CL_E_LIMIT, "%lld messages exceed msg_cap %lld", (long long)n_msgs, (long long)msg_cap);
  // unit payloads are all 1: no history on the device, nothing to pack or copy
  const bool dev_msgs = msg_tokens && v.hist > 0 && n_msgs > 0;
  const int64_t width = info->node_hi - info->node_lo;
  if ((rc = r->d_sp_chan.ensure((size_t)n_entries)) || (rc = r->d_sp_cnt.ensure((size_t)n_entries))) return rc;
  if (dev_msgs && (rc = r->d_sp_msg.ensure((size_t)n_msgs))) return rc;
  if (tokens && (rc = r->d_sp_tok.ensure(nsz * (size_t)width))) return rc;
  if ((rc = r->sp.mark(2, v.stream))) return rc;
  if (n_entries > 0 &&
      (rc = launch_err(cg_launch_sparse_write(P, sid_lo, ns, r->d_sp_tiles.p, r->d_sp_rows.p, d_off, d_moff,
                                              r->d_sp_chan.p, r->d_sp_cnt.p, dev_msgs ? r->d_sp_msg.p : nullptr,
                                              v.stream))))
    return rc;
  if (tokens && (rc = launch_err(cg_launch_sparse_tokens(P, sid_lo, ns, r->d_sp_tok.p, v.stream)))) return rc;
  if ((rc = r->sp.mark(3, v.stream))) return rc;
  if (n_entries > 0) {
    HIP_TRY(hipMemcpyAsync(ent_channel, r->d_sp_chan.p, (size_t)n_entries * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
    HIP_TRY(hipMemcpyAsync(ent_count, r->d_sp_cnt.p, (size_t)n_entries * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
  }
  if (dev_msgs) HIP_TRY(hipMemcpyAsync(msg_tokens, r->d_sp_msg.p, (size_t)n_msgs * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
  if (tokens && width > 0)
    HIP_TRY(hipMemcpyAsync(tokens, r->d_sp_tok.p, nsz * (size_t)width * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
  HIP_TRY(hipStreamSynchronize(v.stream));
  r->sp.done = 2;
  if (msg_tokens && !dev_msgs) std::fill(msg_tokens, msg_tokens + n_msgs, 1);
  return CL_OK;
}

int cl_graph_sparse_time(cl_graph* g, double* ms) {
  GRAPH_CALL(g);
  if (!ms) return set_err(CL_E_INVALID, "null output");
  const Readouts* r = graph_readouts(g);
  if (!r->sp.done) return set_err(CL_E_STATE, "no sparse collect has run");
  double a = 0, b = 0;
  int rc = r->sp.ms(0, 1, &a);
  if (!rc && r->sp.done > 1) rc = r->sp.ms(2, 3, &b);
  *ms = a + b;
  return rc;
}

// ---- node and channel profile over a snapshot range (cg_profile.hip) -------------------------
int cl_graph_set_profile_slices(cl_graph* g, int32_t slices) {
  GRAPH_CALL(g);
  if (slices < 0) return set_err(CL_E_INVALID, "negative slice count");
  graph_readouts(g)->pf_slices = slices;
  return CL_OK;
}

int cl_graph_snapshot_profile(cl_graph* g, int32_t sid_lo, int32_t sid_hi, const cl_graph_profile_spec* spec,
                              const int32_t* use, const int64_t* origins, int64_t* head, int32_t* used,
                              int64_t* node_rows, cl_graph_profile_entry* entries, int64_t ent_cap) {
  GRAPH_CALL(g);
  static_assert(sizeof(cl_graph_profile_spec) == 4 * sizeof(int32_t), "cl_graph_profile_spec is 4 x int32");
  static_assert(sizeof(cl_graph_profile_entry) == kProfileEntryBytes, "cl_graph_profile_entry is 32 bytes");
  static_assert(CL_PF_NODE_WORDS == kProfileNodeWords && CL_GRAPH_PROFILE_MAX_BINS == kProfileMaxBins, "cg_engine.h");
  if (!spec || !head) return set_err(CL_E_INVALID, "null %s", !spec ? "spec" : "head");
  if (spec->msg_bins < 1 || spec->msg_bins > CL_GRAPH_PROFILE_MAX_BINS || spec->msg_width < 1 || spec->min_msgs < 1 ||
      spec->reserved)
    return set_err(CL_E_INVALID, "profile spec: msg_bins %d (1..%d), msg_width %d (>= 1), min_msgs %d (>= 1), reserved %d",
                spec->msg_bins, CL_GRAPH_PROFILE_MAX_BINS, spec->msg_width, spec->min_msgs, spec->reserved);
  int rc = sid_range_ok(g, sid_lo, sid_hi);
  if (rc) return rc;
  if (ent_cap < 0) return set_err(CL_E_INVALID, "negative capacity");
  if (ent_cap > 0 && !entries) return set_err(CL_E_INVALID, "null entries with ent_cap > 0");
  const GraphFacts f = graph_facts(g);
  if (f.part && node_rows && !origins)
    return set_err(CL_E_STATE, "a partitioned run needs the origins: only the initiator's owner knows the start");
  const int32_t ns = sid_hi - sid_lo, bins = spec->msg_bins;
  const size_t head_words = (size_t)CL_PF_HEAD + (size_t)bins;
  if (ns == 0) {
    std::fill(head, head + head_words, 0);
    head[CL_PF_NODE_LO] = f.node_lo;
    head[CL_PF_NODE_HI] = f.node_hi;
    return CL_OK;
  }
  GraphView v;
  if ((rc = graph_view(g, &v))) return rc;
  Readouts* r = graph_readouts(g);
  const GParams& P = *v.P;
  const size_t nsz = (size_t)ns, ke = (size_t)(v.k_hi - v.k_lo), width = (size_t)(P.part_hi - P.part_lo);
  if ((rc = r->d_pf_i32.ensure(3 * nsz)) || (rc = r->d_pf_org.ensure(2 * nsz)) || (rc = r->d_pf_head.ensure(head_words)) ||
      (rc = r->d_pf_acc.ensure(4 * ke)) || (rc = r->d_pf_tiles.ensure((size_t)cg_profile_tiles(P.e))))
    return rc;
  if (node_rows && (rc = r->d_pf_rows.ensure(width * (size_t)CL_PF_NODE_WORDS))) return rc;
  int32_t* d_use = r->d_pf_i32.p;
  long long* d_org_in = r->d_pf_org.p;
  GProfile s{};
  s.list = d_use + nsz;
  s.used = d_use + 2 * nsz;
  s.org = d_org_in + nsz;
  s.head = r->d_pf_head.p;
  s.acc = r->d_pf_acc.p;
  s.rows = r->d_pf_rows.p;
  s.tiles = r->d_pf_tiles.p;
  // the mask, and the origins or the initiators' ranks
  std::vector<long long> org(nsz);
  if (origins) std::copy(origins, origins + ns, org.begin());
  else graph_initiators(g, sid_lo, sid_hi, org.data());
  if (use) HIP_TRY(hipMemcpyAsync(d_use, use, nsz * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
  HIP_TRY(hipMemcpyAsync(d_org_in, org.data(), nsz * sizeof(long long), hipMemcpyHostToDevice, v.stream));
  HIP_TRY(hipStreamSynchronize(v.stream));  // (`org` is a local, `use` the caller's)
  r->pf.done = 0;
  if ((rc = r->pf.mark(0, v.stream))) return rc;
  if ((rc = launch_err(cg_launch_profile_reduce(P, v.k_lo, v.k_hi, sid_lo, ns, use ? d_use : nullptr, d_org_in,
                                                origins ? 1 : 0, r->pf_slices, spec->min_msgs, bins, spec->msg_width, s,
                                                v.n_cus, v.stream))))
    return rc;
  if ((rc = r->pf.mark(1, v.stream))) return rc;
  // the head decides the sizes: the host reads it between the reduction and the fill
  std::vector<long long> h(head_words);
  std::vector<int32_t> h_used(nsz);
  HIP_TRY(hipMemcpyAsync(h.data(), s.head, head_words * sizeof(long long), hipMemcpyDeviceToHost, v.stream));
  HIP_TRY(hipMemcpyAsync(h_used.data(), s.used, nsz * sizeof(int32_t), hipMemcpyDeviceToHost, v.stream));
  HIP_TRY(hipStreamSynchronize(v.stream));
  r->pf.done = 1;
  h[CL_PF_N_SIDS] = ns;
  h[CL_PF_NODE_LO] = f.node_lo;
  h[CL_PF_NODE_HI] = f.node_hi;
  h[CL_PF_CHANNELS] = (long long)ke;
  h[CL_PF_UNIT_PAYLOADS] = v.hist == 0 ? 1 : 0;
  std::copy(h.begin(), h.end(), head);
  if (used) std::copy(h_used.begin(), h_used.end(), used);
  const int64_t n_entries = h[CL_PF_ENTRIES];
  if (n_entries > ent_cap)
    return set_err(CL_E_LIMIT, "%lld entries exceed ent_cap %lld", (long long)n_entries, (long long)ent_cap);
  if ((rc = r->d_pf_ent.ensure((size_t)n_entries))) return rc;
  if ((rc = r->pf.mark(2, v.stream))) return rc;
  if (node_rows && (rc = launch_err(cg_launch_profile_nodes(P, v.k_lo, v.k_hi, sid_lo, ns, r->pf_slices, s, v.n_cus, v.stream))))
    return rc;
  if (n_entries > 0 &&
      (rc = launch_err(cg_launch_profile_fill(P, v.k_lo, v.k_hi, sid_lo, spec->min_msgs, s, r->d_pf_ent.p, v.stream))))
    return rc;
  if ((rc = r->pf.mark(3, v.stream))) return rc;
  if (node_rows && width > 0)
    HIP_TRY(hipMemcpyAsync(node_rows, s.rows, width * CL_PF_NODE_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost, v.stream));
  if (n_entries > 0)
    HIP_TRY(hipMemcpyAsync(entries, r->d_pf_ent.p, (size_t)n_entries * sizeof(cl_graph_profile_entry),
                           hipMemcpyDeviceToHost, v.stream));
  HIP_TRY(hipStreamSynchronize(v.stream));
  r->pf.done = 2;
  return CL_OK;
}

int cl_graph_profile_time(cl_graph* g, double* ms) {
  GRAPH_CALL(g);
  if (!ms) return set_err(CL_E_INVALID, "null output");
  const Readouts* r = graph_readouts(g);
  if (!r->pf.done) return set_err(CL_E_STATE, "no snapshot profile has been computed");
  double a = 0, b = 0;
  int rc = r->pf.ms(0, 1, &a);
  if (!rc && r->pf.done > 1) rc = r->pf.ms(2, 3, &b);
  *ms = a + b;
  return rc;
}

}  // extern "C"
