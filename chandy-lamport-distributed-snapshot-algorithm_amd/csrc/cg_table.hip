// cg_table.hip -- per-snapshot summary table of the graph engine (cl_graph_snapshot_table).
//
// One pass over the snapshot planes of a run reduces, for every snapshot id of a range, one
// row of 16 int64 (TableField below == cl_graph_snap_row, clgraph.h): who started it and when,
// how far its marker wave got, what the created local snapshots hold, and -- for completed
// snapshots -- the recorded messages, their token payloads and the snapshot's content digest
// (its term of CL_GSUM_DIGEST, cg_kernels.hip k_checks_snap).  n_sids x 128 B leave the device.
//
// Read pattern.  grid = (chunks, sids): blockIdx.y strides over the snapshot ids, the
// workgroups of one sid share its planes grid-stride, and the grid is sized to the chip (a few
// workgroups per CU), not to sids x nodes.  Every lane keeps two 16-byte loads in flight.
//   node part     one 16-byte load of the SNode record per lane, lane-linear over the owned
//                 node ranks.  A record counts iff its creation key W is set; the reset leaves
//                 stale stok words under W == ~0, so stok is used for created nodes only.
//   channel part  (completed snapshots only: the cursors of a channel into a node without its
//                 local snapshot are undefined)  walks the in-positions k of the owned nodes'
//                 in-CSR range: rec, histv and the in-position -> channel map `in_ch` are all
//                 indexed by k, so every load is lane-linear; two cursors per 16-byte load from
//                 the first 16-byte aligned cursor of the plane's range on, the at most two
//                 cursors left at the ends by one lane.
// The hash of the digest terms is cg_hash(seed, sid, x) = mix64(mix64(seed ^ sid * G) ^ x * D):
// the inner mix is the same for the whole plane and is taken once per sid.
//
// Reduction.  Per-lane partials stay in registers over the grid-stride loops; a wave folds them
// with shuffles, the workgroup's waves meet in LDS, and one lane per field issues one global
// 64-bit integer atomic (add / min / max) on the device row -- skipped when the workgroup's
// value is still the field's identity.  All integer: the table does not depend on the grid.
#include <hip/hip_runtime.h>

#include "cg_engine.h"

namespace clsnap {
namespace {

// Grid shape (measured, DESIGN.md §10 'k_table'): the closing atomics of all workgroups of one
// sid land on one 128-byte row, so few large workgroups per sid beat many small ones -- a
// single snapshot over 2^20 nodes took 0.094 ms with 2048 workgroups of 256 threads and 0.042 ms
// with 512 of 512 -- while many sids want the chip full of waves (4 x 512 threads per CU).
constexpr int32_t kTableThreads = 512;
constexpr int32_t kTableWaves = kTableThreads / 64;
constexpr int32_t kTableBlocksPerCu = 4;
constexpr int32_t kTableSharePerCu = 2;  // workgroups per CU that may share one sid's row
constexpr int32_t kTableItems = 4;  // records (cursor pairs) per lane the grid's x extent is sized for
constexpr long long kI64Max = 0x7fffffffffffffffLL;
constexpr long long kI64Min = -kI64Max - 1;

// Field order of cl_graph_snap_row (include/clgraph.h).
enum TableField : int32_t {
  TF_SID = 0, TF_INITIATOR, TF_START, TF_COMPLETE, TF_CREATED, TF_LAST_CREATE, TF_NODE_TOKENS, TF_MIN_TOKENS,
  TF_MAX_TOKENS, TF_REC_MSGS, TF_REC_TOKENS, TF_REC_CHANNELS, TF_MAX_CH_MSGS, TF_DIGEST, kTableFields = 16
};
// The reduced fields TF_INITIATOR .. TF_DIGEST without TF_COMPLETE, in LDS slot order.
constexpr int32_t kTableSlots = 12;
__device__ constexpr int32_t kSlotField[kTableSlots] = {TF_INITIATOR, TF_START, TF_CREATED, TF_LAST_CREATE,
                                                        TF_NODE_TOKENS, TF_MIN_TOKENS, TF_MAX_TOKENS, TF_REC_MSGS,
                                                        TF_REC_TOKENS, TF_REC_CHANNELS, TF_MAX_CH_MSGS, TF_DIGEST};
enum SlotOp : int32_t { OP_ADD = 0, OP_MIN = 1, OP_MAX = 2 };
__device__ constexpr int32_t kSlotOp[kTableSlots] = {OP_MAX, OP_MAX, OP_ADD, OP_MAX, OP_ADD, OP_MIN,
                                                     OP_MAX, OP_ADD, OP_ADD, OP_ADD, OP_MAX, OP_ADD};
// Identity of every slot: what k_table_init leaves in the row, and what a workgroup skips.
__device__ constexpr long long kSlotIdentity[kTableSlots] = {-1, -1, 0, -1, 0, kI64Max, kI64Min, 0, 0, 0, 0, 0};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// One 16-byte load per lane.  The empty asm keeps all four words live, so the load is not
// narrowed to the words the code goes on to use (it issues no instruction and touches no memory).
__device__ __forceinline__ u32x4 load16(const u32x4* p) { return *p; }
__device__ __forceinline__ void keep16(u32x4& x) { asm volatile("" : "+v"(x)); }

__device__ __forceinline__ long long wave_fold(long long v, int32_t op) {
  for (int o = 32; o > 0; o >>= 1) {
    const long long w = __shfl_xor(v, o);
    v = op == OP_ADD ? (long long)((unsigned long long)v + (unsigned long long)w)
                     : op == OP_MIN ? (w < v ? w : v) : (w > v ? w : v);
  }
  return v;
}

// Rows [0, n_sids) of snapshots sid_lo + i at their identities; complete_tick is final here.
__global__ void __launch_bounds__(kTableThreads) k_table_init(const int32_t* ctick, int32_t sid_lo, int32_t n_sids,
                                                              long long* rows) {
  const int32_t i = blockIdx.x * kTableThreads + threadIdx.x;
  if (i >= n_sids * kTableFields) return;
  const int32_t r = i / kTableFields, f = i - r * kTableFields, sid = sid_lo + r;
  long long v = 0;
  if (f == TF_SID) v = sid;
  else if (f == TF_INITIATOR || f == TF_START || f == TF_LAST_CREATE) v = -1;
  else if (f == TF_COMPLETE) {
    const int32_t t = ctick[sid];
    v = t < 0 ? -1 : t;
  } else if (f == TF_MIN_TOKENS) v = kI64Max;
  else if (f == TF_MAX_TOKENS) v = kI64Min;
  rows[i] = v;
}

struct ChanAcc {
  unsigned long long msgs, toks, chans, dig;
  uint32_t mx;
};

// One recording cursor pair x of in-position k (channel c) of a completed snapshot.
__device__ __forceinline__ void table_channel(const GParams& p, uint64_t h_sid, int32_t k, int32_t c, uint64_t x,
                                              ChanAcc& a) {
  const uint32_t b = (uint32_t)x, e = (uint32_t)(x >> 32);
  const uint32_t cnt = e - b;
  long long s = (long long)cnt;  // unit payloads (the payload rule of k_checks_snap's hist_sum)
  if (p.hist) {
    s = 0;
    const uint32_t* h = p.histv + (size_t)k * p.hist;
    for (uint32_t q = b; q < e; ++q) s += h[q];
  }
  a.msgs += cnt;
  a.toks += (unsigned long long)s;
  a.chans += cnt != 0;
  a.mx = cnt > a.mx ? cnt : a.mx;
  const uint64_t hc = mix64(h_sid ^ ((uint64_t)c * 0xD6E8FEB86659FD93ULL));  // cg_hash(0xC4A1, sid, c)
  a.dig += mix64(hc ^ (((uint64_t)cnt << 32) | (uint32_t)s));
}

// in_ch: channel of every in-position (the inverse of route[c].y); [k_lo, k_hi) the in-CSR
// range of the owned nodes.  rows: device rows of the snapshots sid_lo + [0, n_sids).
__global__ void __launch_bounds__(kTableThreads) k_table(GParams p, const int32_t* __restrict__ in_ch, int32_t k_lo,
                                                         int32_t k_hi, int32_t sid_lo, int32_t n_sids,
                                                         long long* rows) {
  __shared__ long long part[kTableWaves][kTableSlots];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gt = (int64_t)blockIdx.x * kTableThreads + threadIdx.x, gs = (int64_t)gridDim.x * kTableThreads;

  for (int32_t r = blockIdx.y; r < n_sids; r += gridDim.y) {
    const int32_t sid = sid_lo + r;
    const bool complete = p.ctick[sid] >= 0;  // (uniform over the workgroup)
    // ---- node part
    const uint64_t hn_sid = mix64(0x5107ull ^ ((uint64_t)sid * 0x9E3779B97F4A7C15ULL));
    const u32x4* sn = reinterpret_cast<const u32x4*>(p.sn + (size_t)sid * p.n);
    unsigned long long created = 0, dig = 0;
    long long tok_sum = 0;
    int32_t tok_min = INT32_MAX, tok_max = INT32_MIN, last = -1, initiator = -1, start = -1;
    // x: W lo32 (creating sender), W hi32 (creation tick), cnt, stok
    auto node = [&](const u32x4 x, int64_t v) {
      if ((x.x & x.y) == 0xffffffffu) return;  // W == ~0: no local snapshot
      const int32_t tick = (int32_t)x.y, st = (int32_t)x.w;
      created += 1;
      tok_sum += st;
      tok_min = st < tok_min ? st : tok_min;
      tok_max = st > tok_max ? st : tok_max;
      last = tick > last ? tick : last;
      if (x.x == 0xffffffffu) initiator = (int32_t)v, start = tick;
      if (complete) {
        const uint64_t h = mix64(hn_sid ^ ((uint64_t)v * 0xD6E8FEB86659FD93ULL));  // cg_hash(0x5107, sid, v)
        dig += mix64(h ^ (uint64_t)(uint32_t)st);
      }
    };
    int64_t v = p.part_lo + gt;
    for (; v + gs < p.part_hi; v += 2 * gs) {  // two records in flight per lane
      u32x4 x0 = load16(sn + v), x1 = load16(sn + v + gs);
      keep16(x0), keep16(x1);
      node(x0, v), node(x1, v + gs);
    }
    if (v < p.part_hi) {
      u32x4 x0 = load16(sn + v);
      keep16(x0);
      node(x0, v);
    }
    // ---- channel part
    ChanAcc a{0, 0, 0, dig, 0};
    if (complete && k_hi > k_lo) {
      const uint64_t hc_sid = mix64(0xC4A1ull ^ ((uint64_t)sid * 0x9E3779B97F4A7C15ULL));
      const int64_t base = (int64_t)sid * p.e;
      const uint64_t* rec = p.rec + base;
      // first in-position of the range whose cursor is 16-byte aligned in the plane
      const int32_t ka = k_lo + (int32_t)((base + k_lo) & 1);  // (<= k_hi: the range is not empty)
      const int32_t n_pairs = (k_hi - ka) >> 1;
      auto pair = [&](const u32x4 x, int32_t k, int32_t c0, int32_t c1) {
        table_channel(p, hc_sid, k, c0, (uint64_t)x.x | ((uint64_t)x.y << 32), a);
        table_channel(p, hc_sid, k + 1, c1, (uint64_t)x.z | ((uint64_t)x.w << 32), a);
      };
      const u32x4* rec2 = reinterpret_cast<const u32x4*>(rec + ka);  // pair j: in-positions ka + 2 j, + 1
      const int32_t* ch2 = in_ch + ka;
      int64_t j = gt;
      for (; j + gs < n_pairs; j += 2 * gs) {  // two pairs in flight per lane
        u32x4 x0 = load16(rec2 + j), x1 = load16(rec2 + j + gs);
        const int32_t c00 = ch2[2 * j], c01 = ch2[2 * j + 1], c10 = ch2[2 * (j + gs)], c11 = ch2[2 * (j + gs) + 1];
        keep16(x0), keep16(x1);
        pair(x0, ka + 2 * (int32_t)j, c00, c01);
        pair(x1, ka + 2 * (int32_t)(j + gs), c10, c11);
      }
      if (j < n_pairs) {
        u32x4 x0 = load16(rec2 + j);
        const int32_t c00 = ch2[2 * j], c01 = ch2[2 * j + 1];
        keep16(x0);
        pair(x0, ka + 2 * (int32_t)j, c00, c01);
      }
      if (gt == 0) {  // the cursors left in front of and behind the pairs
        if (ka > k_lo) table_channel(p, hc_sid, k_lo, in_ch[k_lo], rec[k_lo], a);
        const int32_t kt = ka + 2 * n_pairs;
        if (kt < k_hi) table_channel(p, hc_sid, kt, in_ch[kt], rec[kt], a);
      }
    }
    // ---- wave, then workgroup, then one atomic per field
    const long long mine[kTableSlots] = {initiator, start, (long long)created, last, tok_sum,
                                         created ? (long long)tok_min : kI64Max, created ? (long long)tok_max : kI64Min,
                                         (long long)a.msgs, (long long)a.toks, (long long)a.chans, (long long)a.mx,
                                         (long long)a.dig};
#pragma unroll
    for (int32_t s = 0; s < kTableSlots; ++s) {
      const long long w = wave_fold(mine[s], kSlotOp[s]);
      if (lane == 0) part[wave][s] = w;
    }
    __syncthreads();
    if (threadIdx.x < kTableSlots) {
      const int32_t s = threadIdx.x, op = kSlotOp[s];
      long long v = part[0][s];
      for (int32_t w = 1; w < kTableWaves; ++w) {
        const long long u = part[w][s];
        v = op == OP_ADD ? (long long)((unsigned long long)v + (unsigned long long)u)
                         : op == OP_MIN ? (u < v ? u : v) : (u > v ? u : v);
      }
      if (v != kSlotIdentity[s]) {
        long long* dst = rows + (size_t)r * kTableFields + kSlotField[s];
        if (op == OP_ADD) atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)v);
        else if (op == OP_MIN) atomicMin(dst, v);
        else atomicMax(dst, v);
      }
    }
    __syncthreads();  // (the next sid's partials reuse `part`)
  }
}

}  // namespace

int cg_launch_table(const GParams& p, const int32_t* in_ch, int32_t k_lo, int32_t k_hi, int32_t sid_lo,
                    int32_t n_sids, long long* rows, int32_t n_cus, void* stream) {
  if (n_sids <= 0) return (int)hipSuccess;
  hipStream_t s = (hipStream_t)stream;
  const int32_t cells = n_sids * kTableFields;
  hipLaunchKernelGGL(k_table_init, dim3((unsigned)((cells + kTableThreads - 1) / kTableThreads)), dim3(kTableThreads),
                     0, s, p.ctick, sid_lo, n_sids, rows);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  // a grid-stride grid sized to the chip: y strides over the sids, x shares one sid's planes
  const int64_t budget = (int64_t)kTableBlocksPerCu * (n_cus > 0 ? n_cus : 1);
  const int64_t gy = n_sids < budget ? (n_sids < 65535 ? n_sids : 65535) : (budget < 65535 ? budget : 65535);
  const int64_t nodes = (int64_t)p.part_hi - p.part_lo, pairs = ((int64_t)k_hi - k_lo + 1) / 2;
  const int64_t work = nodes > pairs ? nodes : pairs, per = (int64_t)kTableThreads * kTableItems;
  int64_t gx = (work + per - 1) / per;
  if (gx > budget / gy) gx = budget / gy;
  const int64_t share = (int64_t)kTableSharePerCu * (n_cus > 0 ? n_cus : 1);
  if (gx > share) gx = share;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(k_table, dim3((unsigned)gx, (unsigned)gy), dim3(kTableThreads), 0, s, p, in_ch, k_lo, k_hi, sid_lo,
                     n_sids, rows);
  return (int)hipGetLastError();
}

}  // namespace clsnap
