// cg_restore_host.cpp -- cl_graph_restore behind include/clgraph.h: a new graph whose time-0 state is a
// completed snapshot of another.  The source is read through its view alone (cg_host.h); the seed
// is built on the device by the sparse collect's passes for one sid (cg_sparse.hip) and the offsets
// and sums of cg_restore.hip, and handed to a clone of the source's frozen topology.  Only the
// entry and message totals and four sums reach the host.
// cl_graph_restore_cut takes the same contents from host arrays instead (a saved, merged or
// hand-made cut): it uploads them into the seed's buffers, proves them well-formed with one kernel
// (cg_cut.hip) next to the same offsets and sums, and clones the template's topology only when the
// verdict is clean, so k_seed never runs on entries nobody checked.
#include <memory>

#include "cg_host.h"

using namespace clsnap;

extern "C" {

int cl_graph_restore(cl_graph* g, int32_t sid, cl_graph** out) {
  static_assert(sizeof(cl_graph_seed_info) == 8 * sizeof(int64_t), "cl_graph_seed_info is 8 x int64");
  if (out) *out = nullptr;
  GRAPH_CALL(g);
  if (!out) return set_err(CL_E_INVALID, "null output");
  const GraphFacts f = graph_facts(g);
  if (sid < 0 || sid >= f.n_sids) return set_err(CL_E_INVALID, "unknown snapshot %d", sid);
  if (f.part) return set_err(CL_E_STATE, "a partitioned run cannot be restored from");
  int32_t status = 0, tick = -1;
  int rc = cl_graph_get_status(g, &status);
  if (rc) return rc;
  if (status != CL_INST_OK) return set_err(CL_E_STATE, "the source run has status %d", status);
  if ((rc = cl_graph_snapshot_tick(g, sid, &tick))) return rc;
  if (tick < 0) return set_err(CL_E_NOT_COMPLETE, "snapshot %d has not completed", sid);
  GraphView v;
  if ((rc = graph_view(g, &v))) return rc;
  const GParams& P = *v.P;

  // scan: the entries and messages of the sid (the head: offsets [2], message offsets [2], complete)
  std::unique_ptr<GraphSeed> seed(new GraphSeed());
  DevBuf<ulonglong2> d_tiles, d_row;
  DevBuf<long long> d_head;
  DevBuf<unsigned long long> d_scan, d_sums;
  GraphTimer<4> t;
  if ((rc = d_tiles.ensure((size_t)cg_sparse_tiles(P.e))) || (rc = d_row.ensure(1)) || (rc = d_head.ensure(5)) ||
      (rc = d_sums.ensure(4)))
    return rc;
  long long* d_off = d_head.p;
  long long* d_moff = d_off + 2;
  int32_t* d_complete = reinterpret_cast<int32_t*>(d_moff + 2);
  if ((rc = t.mark(0, v.stream))) return rc;
  if ((rc = launch_err(cg_launch_sparse_scan(P, sid, 1, d_tiles.p, d_row.p, d_off, d_moff, d_complete, v.stream)))) return rc;
  if ((rc = t.mark(1, v.stream))) return rc;
  long long head[5];
  HIP_TRY(hipMemcpyAsync(head, d_head.p, sizeof head, hipMemcpyDeviceToHost, v.stream));
  HIP_TRY(hipStreamSynchronize(v.stream));
  const int64_t n_ent = head[1], n_msgs = head[3], n = P.n;
  const bool dev_msgs = v.hist > 0 && n_msgs > 0;  // (no history: every payload is 1)

  // write: token plane, entries, payloads; then the message offsets and the sums
  if ((rc = seed->init_tok.ensure((size_t)n)) || (rc = seed->channel.ensure((size_t)n_ent)) ||
      (rc = seed->count.ensure((size_t)n_ent)) || (rc = seed->moff.ensure((size_t)n_ent)) ||
      (rc = d_scan.ensure((size_t)cg_restore_tiles(n_ent))))
    return rc;
  if (dev_msgs && (rc = seed->msgs.ensure((size_t)n_msgs))) return rc;
  if ((rc = t.mark(2, v.stream))) return rc;
  HIP_TRY(hipMemsetAsync(d_sums.p, 0, 4 * sizeof(unsigned long long), v.stream));
  if (n_ent > 0 && (rc = launch_err(cg_launch_sparse_write(P, sid, 1, d_tiles.p, d_row.p, d_off, d_moff, seed->channel.p,
                                                           seed->count.p, dev_msgs ? seed->msgs.p : nullptr, v.stream))))
    return rc;
  if ((rc = launch_err(cg_launch_sparse_tokens(P, sid, 1, seed->init_tok.p, v.stream))) ||
      (rc = launch_err(cg_launch_restore_offsets(seed->count.p, n_ent, seed->moff.p, d_scan.p, v.stream))) ||
      (rc = launch_err(cg_launch_restore_reduce(seed->count.p, n_ent, dev_msgs ? seed->msgs.p : nullptr, n_msgs,
                                                seed->init_tok.p, n, d_sums.p, v.stream))))
    return rc;
  if ((rc = t.mark(3, v.stream))) return rc;
  unsigned long long sums[4];
  HIP_TRY(hipMemcpyAsync(sums, d_sums.p, sizeof sums, hipMemcpyDeviceToHost, v.stream));
  HIP_TRY(hipStreamSynchronize(v.stream));
  double ms_scan = 0, ms_write = 0;
  if ((rc = t.ms(0, 1, &ms_scan)) || (rc = t.ms(2, 3, &ms_write))) return rc;
  seed->build_ms = ms_scan + ms_write;
  cl_graph_seed_info& info = seed->info;
  info.source_sid = sid;
  info.channels = n_ent;
  info.msgs = n_msgs;
  info.tokens = dev_msgs ? (int64_t)sums[1] : n_msgs;
  info.max_ch_msgs = (int64_t)sums[0];
  info.unit_payloads = dev_msgs && sums[2] ? 0 : 1;
  info.node_tokens = (int64_t)sums[3];
  if (info.unit_payloads) seed->msgs.release();  // (all ones: the seed kernel needs no payloads)

  cl_graph* r = nullptr;
  if ((rc = graph_clone_frozen(g, &r))) return rc;
  graph_adopt_seed(r, seed.release());
  *out = r;
  return CL_OK;
}

int cl_graph_restore_cut(cl_graph* topo, const cl_graph_cut* cut, cl_graph** out) {
  static_assert(sizeof(cl_graph_cut) == 64, "cl_graph_cut is 64 bytes");
  if (out) *out = nullptr;
  GRAPH_CALL(topo);
  if (!cut) return set_err(CL_E_INVALID, "null cut");
  if (!out) return set_err(CL_E_INVALID, "null output");
  const int64_t n = cut->n_nodes, n_ent = cut->n_entries, n_msgs = cut->n_msgs;
  if (n < 0 || n_ent < 0 || n_msgs < 0)
    return set_err(CL_E_INVALID, "negative length (n_nodes %lld, n_entries %lld, n_msgs %lld)", (long long)n,
                   (long long)n_ent, (long long)n_msgs);
  if ((n > 0 && !cut->tokens) || (n_ent > 0 && (!cut->channel || !cut->count)))
    return set_err(CL_E_INVALID, "null array with a positive length");  // (msg_tokens NULL: all 1)
  if (graph_facts(topo).part) return set_err(CL_E_STATE, "a partitioned graph cannot be a restore's template");
  GraphTopo tp;
  int rc = graph_topology(topo, &tp);
  if (rc) return rc;
  if (tp.n == 0) return set_err(CL_E_STATE, "the topology has no nodes");
  if (n != tp.n) return set_err(CL_E_INVALID, "n_nodes %lld, the topology has %d", (long long)n, tp.n);
  if (n_ent > tp.e) return set_err(CL_E_INVALID, "n_entries %lld, the topology has %lld channels", (long long)n_ent, (long long)tp.e);
  if (n_msgs < n_ent || n_msgs > n_ent * kCutMaxCount)
    return set_err(CL_E_INVALID, "n_msgs %lld outside [n_entries, n_entries * %d] of %lld entries", (long long)n_msgs,
                   kCutMaxCount, (long long)n_ent);

  // upload; then the check, the offsets and the sums in one submission
  hipStream_t stream = nullptr;
  int32_t n_cus = 0;
  if ((rc = graph_topology_resident(topo, &stream, &n_cus))) return rc;
  const bool dev_msgs = cut->msg_tokens && n_msgs > 0;
  std::unique_ptr<GraphSeed> seed(new GraphSeed());
  DevBuf<unsigned long long> d_scan, d_res;  // d_res: the four sums, the verdict
  if ((rc = seed->init_tok.ensure((size_t)n)) || (rc = seed->channel.ensure((size_t)n_ent)) ||
      (rc = seed->count.ensure((size_t)n_ent)) || (rc = seed->moff.ensure((size_t)n_ent)) ||
      (rc = d_scan.ensure((size_t)cg_restore_tiles(n_ent))) || (rc = d_res.ensure(5)))
    return rc;
  if (dev_msgs && (rc = seed->msgs.ensure((size_t)n_msgs))) return rc;
  auto up = [&](int32_t* dst, const int32_t* src, int64_t count) {
    return count > 0 ? hipMemcpyAsync(dst, src, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, stream) : hipSuccess;
  };
  HIP_TRY(up(seed->init_tok.p, cut->tokens, n));
  HIP_TRY(up(seed->channel.p, cut->channel, n_ent));
  HIP_TRY(up(seed->count.p, cut->count, n_ent));
  if (dev_msgs) HIP_TRY(up(seed->msgs.p, cut->msg_tokens, n_msgs));
  HIP_TRY(hipMemsetAsync(d_res.p, 0, 4 * sizeof(unsigned long long), stream));
  HIP_TRY(hipMemsetAsync(d_res.p + 4, 0xff, sizeof(unsigned long long), stream));  // kCutClean
  GraphTimer<2> t;
  if ((rc = t.mark(0, stream))) return rc;
  const int32_t* d_msgs = dev_msgs ? seed->msgs.p : nullptr;
  // (neither the offsets nor the sums index by a value they read: they may run on unchecked arrays)
  if ((rc = launch_err(cg_launch_cut_check(seed->init_tok.p, n, seed->channel.p, seed->count.p, n_ent, d_msgs, n_msgs,
                                           (int32_t)tp.e, d_res.p + 4, n_cus, stream))) ||
      (rc = launch_err(cg_launch_restore_offsets(seed->count.p, n_ent, seed->moff.p, d_scan.p, stream))) ||
      (rc = launch_err(cg_launch_restore_reduce(seed->count.p, n_ent, d_msgs, n_msgs, seed->init_tok.p, n, d_res.p, stream))))
    return rc;
  if ((rc = t.mark(1, stream))) return rc;
  unsigned long long res[5];
  long long last_off = 0;
  HIP_TRY(hipMemcpyAsync(res, d_res.p, sizeof res, hipMemcpyDeviceToHost, stream));
  if (n_ent > 0)
    HIP_TRY(hipMemcpyAsync(&last_off, seed->moff.p + (n_ent - 1), sizeof last_off, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));

  // the verdict: the lowest rule, then the lowest index
  if (res[4] != kCutClean) {
    const uint32_t rule = (uint32_t)(res[4] >> 56);
    const int64_t i = (int64_t)(res[4] & ((1ull << 56) - 1));
    switch (rule) {
      case kCutRuleTokens:
        return set_err(CL_E_INVALID, "tokens[%lld] = %d is negative", (long long)i, cut->tokens[i]);
      case kCutRuleChannel:
        if ((uint32_t)cut->channel[i] >= (uint32_t)tp.e)
          return set_err(CL_E_INVALID, "channel[%lld] = %d is outside [0, %lld)", (long long)i, cut->channel[i], (long long)tp.e);
        return set_err(CL_E_INVALID, "channel[%lld] = %d does not ascend from channel[%lld] = %d", (long long)i,
                       cut->channel[i], (long long)i - 1, cut->channel[i - 1]);
      case kCutRuleCount:
        return set_err(CL_E_INVALID, "count[%lld] = %d is outside [1, %d]", (long long)i, cut->count[i], kCutMaxCount);
      case kCutRulePayload:
        return set_err(CL_E_INVALID, "msg_tokens[%lld] = %d is outside [0, 0x7fffffff]", (long long)i, cut->msg_tokens[i]);
    }
    return set_err(CL_E_DEVICE, "the cut check returned the unknown verdict %llx", res[4]);
  }
  // (every count is in [1, kCutMaxCount] here, so the offsets' total is the true sum)
  const int64_t total = n_ent > 0 ? (int64_t)last_off + cut->count[n_ent - 1] : 0;
  if (total != n_msgs)
    return set_err(CL_E_INVALID, "n_msgs = %lld, the counts sum to %lld", (long long)n_msgs, (long long)total);

  if ((rc = t.ms(0, 1, &seed->build_ms))) return rc;
  cl_graph_seed_info& info = seed->info;
  info.source_sid = cut->source_sid;
  info.channels = n_ent;
  info.msgs = n_msgs;
  info.tokens = dev_msgs ? (int64_t)res[1] : n_msgs;
  info.max_ch_msgs = (int64_t)res[0];
  info.unit_payloads = dev_msgs && res[2] ? 0 : 1;
  info.node_tokens = (int64_t)res[3];
  if (info.unit_payloads) seed->msgs.release();  // (all ones: the seed kernel needs no payloads)

  cl_graph* r = nullptr;
  if ((rc = graph_clone_frozen(topo, &r))) return rc;
  graph_adopt_seed(r, seed.release());
  *out = r;
  return CL_OK;
}

int cl_graph_seed_info_of(cl_graph* r, cl_graph_seed_info* info) {
  GRAPH_CALL(r);
  if (!info) return set_err(CL_E_INVALID, "null output");
  const GraphSeed* s = graph_seed(r);
  if (!s) return set_err(CL_E_STATE, "not a restored graph (cl_graph_restore)");
  *info = s->info;
  return CL_OK;
}

int cl_graph_restore_time(cl_graph* r, double* build_ms, double* seed_ms) {
  GRAPH_CALL(r);
  if (!build_ms || !seed_ms) return set_err(CL_E_INVALID, "null output");
  const GraphSeed* s = graph_seed(r);
  if (!s) return set_err(CL_E_STATE, "not a restored graph (cl_graph_restore)");
  *build_ms = s->build_ms;
  *seed_ms = 0;
  if (!s->seed_t.done) return CL_OK;
  int rc = cl_graph_synchronize(r);
  return rc ? rc : s->seed_t.ms(0, 1, seed_ms);
}

}  // extern "C"
