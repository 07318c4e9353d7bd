// cg_sparse.hip -- sparse packed collect of snapshot contents (cl_graph_collect_sparse).
//
// A Chandy-Lamport snapshot's channel state is sparse: only the channels that delivered
// something between the receiver's local snapshot and the marker's arrival hold messages.
// For the snapshot ids sid_lo + [0, n_sids) this file compacts, on the device, one entry per
// channel into an owned node that recorded at least one message of a COMPLETED snapshot --
// (channel, count) -- and the entries' payloads back to back, ordered by (sid, channel):
// the channel order of cl_graph_channels and of the dense cl_graph_collect_snapshot.
// Incomplete snapshots have no entries and their cursors are never read (they are undefined;
// the same rule as cg_table.hip).
//
// Count -> scan -> write, all integer, so the result is a pure function of the run's records:
//   k_sparse_count      grid (channel tiles, sids).  A tile is kSparseTile consecutive channels,
//                       kSparseItems consecutive channels per lane.  Channel c reads its cursor
//                       pair at rec[sid * e + route[c].y] (the gather of k_checks_snap); the
//                       workgroup stores the tile's (entries, messages).
//   k_sparse_scan_rows  one workgroup per sid: exclusive scan of its tiles' pairs in place,
//                       the row's totals aside.
//   k_sparse_scan_top   one workgroup: exclusive scan of the row totals -> row_offsets, the
//                       rows' message bases, `complete`, and the grand totals the host reads.
//   k_sparse_write      grid as the count's: a workgroup whose tile holds entries recomputes
//                       it, ranks its lanes' entries by a wave prefix (shuffles) and LDS across
//                       the waves, and stores entries and payloads at the tile's base.
//   k_sparse_tokens     the stok words of the SNode records, one 16-byte load per lane, packed
//                       into a dense int32 plane [n_sids][owned nodes]; -1 rows for incomplete
//                       snapshots (whose stok words may be stale).
#include <hip/hip_runtime.h>

#include "cg_engine.h"

namespace clsnap {
namespace {

constexpr int32_t kSparseThreads = 256;
constexpr int32_t kSparseWaves = kSparseThreads / 64;
constexpr int32_t kSparseItems = 8;  // consecutive channels per lane (8 in-flight cursor gathers)
constexpr int32_t kSparseTile = kSparseThreads * kSparseItems;
// A lane's (entries, messages) travel as one word through the workgroup's prefix: entries in
// the low kSparseEntBits (a tile holds at most kSparseTile = 2^11 of them), messages above.
constexpr int32_t kSparseEntBits = 16;
constexpr uint64_t kSparseEntMask = (1ull << kSparseEntBits) - 1;
static_assert(kSparseTile <= (1 << kSparseEntBits) - 1, "a tile's entries must fit the low field");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// In-positions of the lane's channels c0 + [0, kSparseItems): -1 for a channel past the end or
// into a node this device does not own (its cursors belong to another device).
__device__ __forceinline__ void tile_inpos(const GParams& p, int64_t c0, int32_t (&k)[kSparseItems]) {
  if (c0 + kSparseItems <= p.e) {  // (c0 is a multiple of kSparseItems: 16-byte aligned pairs of routes)
    const u32x4* r4 = reinterpret_cast<const u32x4*>(p.route + c0);
#pragma unroll
    for (int32_t j = 0; j < kSparseItems / 2; ++j) {
      const u32x4 x = r4[j];
      const int32_t d0 = (int32_t)x.x, d1 = (int32_t)x.z;
      k[2 * j] = d0 >= p.part_lo && d0 < p.part_hi ? (int32_t)x.y : -1;
      k[2 * j + 1] = d1 >= p.part_lo && d1 < p.part_hi ? (int32_t)x.w : -1;
    }
  } else {
#pragma unroll
    for (int32_t i = 0; i < kSparseItems; ++i) {
      k[i] = -1;
      if (c0 + i < p.e) {
        const int2 r = p.route[c0 + i];
        if (r.x >= p.part_lo && r.x < p.part_hi) k[i] = r.y;
      }
    }
  }
}

// Cursor pairs of the lane's channels in the plane `rec` of one completed snapshot: begin and
// count per channel, and the lane's packed (entries, messages).
__device__ __forceinline__ uint64_t tile_cursors(const uint64_t* __restrict__ rec, const int32_t (&k)[kSparseItems],
                                                 uint32_t (&b)[kSparseItems], uint32_t (&n)[kSparseItems]) {
  uint64_t x[kSparseItems];
#pragma unroll
  for (int32_t i = 0; i < kSparseItems; ++i) x[i] = k[i] >= 0 ? rec[k[i]] : 0;  // (all gathers in flight)
  uint64_t w = 0;
#pragma unroll
  for (int32_t i = 0; i < kSparseItems; ++i) {
    b[i] = (uint32_t)x[i];
    n[i] = (uint32_t)(x[i] >> 32) - b[i];
    w += ((uint64_t)n[i] << kSparseEntBits) | (n[i] != 0);
  }
  return w;
}

// tb[r * tiles + t] = (entries, messages) of tile t of snapshot sid_lo + r; (0, 0) if incomplete.
__global__ void __launch_bounds__(kSparseThreads) k_sparse_count(GParams p, int32_t sid_lo, int32_t n_sids,
                                                                 int32_t tiles, ulonglong2* __restrict__ tb) {
  __shared__ uint64_t lds[kSparseWaves];
  const int64_t c0 = (int64_t)blockIdx.x * kSparseTile + (int64_t)threadIdx.x * kSparseItems;
  int32_t k[kSparseItems];
  tile_inpos(p, c0, k);
  for (int32_t r = blockIdx.y; r < n_sids; r += gridDim.y) {
    const int32_t sid = sid_lo + r;
    uint64_t w = 0;
    if (p.ctick[sid] >= 0) {  // (uniform over the workgroup)
      uint32_t b[kSparseItems], n[kSparseItems];
      w = tile_cursors(p.rec + (int64_t)sid * p.e, k, b, n);
    }
    uint64_t total;
    (void)cg_block_prefix<kSparseWaves>(w, lds, total);
    if (threadIdx.x == 0)
      tb[(int64_t)r * tiles + blockIdx.x] = make_ulonglong2(total & kSparseEntMask, total >> kSparseEntBits);
  }
}

// Row r (one workgroup): its tiles' pairs become their exclusive prefix within the row, in place;
// rtot[r] = the row's (entries, messages).
__global__ void __launch_bounds__(kSparseThreads) k_sparse_scan_rows(int32_t tiles, ulonglong2* __restrict__ tb,
                                                                     ulonglong2* __restrict__ rtot) {
  __shared__ uint64_t lds[kSparseWaves];
  ulonglong2* row = tb + (int64_t)blockIdx.x * tiles;
  uint64_t ce = 0, cm = 0;
  for (int32_t t0 = 0; t0 < tiles; t0 += kSparseThreads) {
    const int32_t t = t0 + threadIdx.x;
    const ulonglong2 v = t < tiles ? row[t] : make_ulonglong2(0, 0);
    uint64_t te, tm;
    const uint64_t xe = cg_block_prefix<kSparseWaves>(v.x, lds, te), xm = cg_block_prefix<kSparseWaves>(v.y, lds, tm);
    if (t < tiles) row[t] = make_ulonglong2(ce + xe, cm + xm);
    ce += te;
    cm += tm;
  }
  if (threadIdx.x == 0) rtot[blockIdx.x] = make_ulonglong2(ce, cm);
}

// One workgroup: row_off[r] / row_moff[r] = entries / messages of the rows before r
// ([n_sids] = the totals), complete[r] = whether snapshot sid_lo + r completed.
__global__ void __launch_bounds__(kSparseThreads) k_sparse_scan_top(const int32_t* __restrict__ ctick, int32_t sid_lo,
                                                                    int32_t n_sids, const ulonglong2* __restrict__ rtot,
                                                                    long long* __restrict__ row_off,
                                                                    long long* __restrict__ row_moff,
                                                                    int32_t* __restrict__ complete) {
  __shared__ uint64_t lds[kSparseWaves];
  uint64_t ce = 0, cm = 0;
  for (int32_t r0 = 0; r0 < n_sids; r0 += kSparseThreads) {
    const int32_t r = r0 + threadIdx.x;
    const ulonglong2 v = r < n_sids ? rtot[r] : make_ulonglong2(0, 0);
    uint64_t te, tm;
    const uint64_t xe = cg_block_prefix<kSparseWaves>(v.x, lds, te), xm = cg_block_prefix<kSparseWaves>(v.y, lds, tm);
    if (r < n_sids) {
      row_off[r] = (long long)(ce + xe);
      row_moff[r] = (long long)(cm + xm);
      complete[r] = ctick[sid_lo + r] >= 0 ? 1 : 0;
    }
    ce += te;
    cm += tm;
  }
  if (threadIdx.x == 0) {
    row_off[n_sids] = (long long)ce;
    row_moff[n_sids] = (long long)cm;
  }
}

// Entries (and, with msg != nullptr, payloads from the history p.histv) of every tile at its base.
__global__ void __launch_bounds__(kSparseThreads) k_sparse_write(GParams p, int32_t sid_lo, int32_t n_sids,
                                                                 int32_t tiles, const ulonglong2* __restrict__ tb,
                                                                 const ulonglong2* __restrict__ rtot,
                                                                 const long long* __restrict__ row_off,
                                                                 const long long* __restrict__ row_moff,
                                                                 int32_t* __restrict__ ent_channel,
                                                                 int32_t* __restrict__ ent_count,
                                                                 int32_t* __restrict__ msg) {
  __shared__ uint64_t lds[kSparseWaves];
  const int64_t c0 = (int64_t)blockIdx.x * kSparseTile + (int64_t)threadIdx.x * kSparseItems;
  int32_t k[kSparseItems];
  tile_inpos(p, c0, k);
  for (int32_t r = blockIdx.y; r < n_sids; r += gridDim.y) {
    const int32_t sid = sid_lo + r;
    if (p.ctick[sid] < 0) continue;  // (uniform over the workgroup, like the exit below)
    const int64_t i = (int64_t)r * tiles + blockIdx.x;
    const ulonglong2 me = tb[i];
    const uint64_t next = (int32_t)blockIdx.x + 1 < tiles ? tb[i + 1].x : rtot[r].x;
    if (next == me.x) continue;  // no entry in this tile
    uint32_t b[kSparseItems], n[kSparseItems];
    const uint64_t w = tile_cursors(p.rec + (int64_t)sid * p.e, k, b, n);
    uint64_t total;
    const uint64_t x = cg_block_prefix<kSparseWaves>(w, lds, total);
    int64_t e_at = row_off[r] + (int64_t)me.x + (int64_t)(x & kSparseEntMask);
    int64_t m_at = row_moff[r] + (int64_t)me.y + (int64_t)(x >> kSparseEntBits);
#pragma unroll
    for (int32_t j = 0; j < kSparseItems; ++j) {
      if (n[j] == 0) continue;
      ent_channel[e_at] = (int32_t)(c0 + j);
      ent_count[e_at] = (int32_t)n[j];
      ++e_at;
      if (msg) {
        const uint32_t* h = p.histv + (size_t)k[j] * p.hist;
        for (uint32_t q = 0; q < n[j]; ++q) {
          const uint32_t at = b[j] + q;  // (a history that overflowed froze the run: no read past it)
          msg[m_at + q] = at < (uint32_t)p.hist ? (int32_t)h[at] : 0;
        }
      }
      m_at += n[j];
    }
  }
}

// out[r * (part_hi - part_lo) + (v - part_lo)] = recorded tokens of owned node v in snapshot
// sid_lo + r, -1 everywhere in the row of an incomplete snapshot.
__global__ void __launch_bounds__(kSparseThreads) k_sparse_tokens(GParams p, int32_t sid_lo, int32_t n_sids,
                                                                  int32_t* __restrict__ out) {
  const int64_t width = (int64_t)p.part_hi - p.part_lo;
  const int64_t j = (int64_t)blockIdx.x * kSparseThreads + threadIdx.x;
  if (j >= width) return;
  for (int32_t r = blockIdx.y; r < n_sids; r += gridDim.y) {
    const int32_t sid = sid_lo + r;
    int32_t st = -1;
    if (p.ctick[sid] >= 0) {
      u32x4 x = *reinterpret_cast<const u32x4*>(p.sn + (int64_t)sid * p.n + p.part_lo + j);
      asm volatile("" : "+v"(x));  // (keeps the 16-byte load whole: cg_table.hip keep16)
      st = (int32_t)x.w;
    }
    out[(int64_t)r * width + j] = st;
  }
}

inline unsigned grid_y(int32_t n_sids) { return (unsigned)(n_sids < 65535 ? n_sids : 65535); }

}  // namespace

int32_t cg_sparse_tiles(int64_t e) {
  const int64_t t = (e + kSparseTile - 1) / kSparseTile;
  return (int32_t)(t > 0 ? t : 1);
}

int cg_launch_sparse_scan(const GParams& p, int32_t sid_lo, int32_t n_sids, ulonglong2* tb, ulonglong2* rtot,
                          long long* row_off, long long* row_moff, int32_t* complete, void* stream) {
  if (n_sids <= 0) return (int)hipSuccess;
  hipStream_t s = (hipStream_t)stream;
  const int32_t tiles = cg_sparse_tiles(p.e);
  hipLaunchKernelGGL(k_sparse_count, dim3((unsigned)tiles, grid_y(n_sids)), dim3(kSparseThreads), 0, s, p, sid_lo,
                     n_sids, tiles, tb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_sparse_scan_rows, dim3((unsigned)n_sids), dim3(kSparseThreads), 0, s, tiles, tb, rtot);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_sparse_scan_top, dim3(1), dim3(kSparseThreads), 0, s, p.ctick, sid_lo, n_sids, rtot, row_off,
                     row_moff, complete);
  return (int)hipGetLastError();
}

int cg_launch_sparse_write(const GParams& p, int32_t sid_lo, int32_t n_sids, const ulonglong2* tb,
                           const ulonglong2* rtot, const long long* row_off, const long long* row_moff,
                           int32_t* ent_channel, int32_t* ent_count, int32_t* msg, void* stream) {
  if (n_sids <= 0) return (int)hipSuccess;
  const int32_t tiles = cg_sparse_tiles(p.e);
  hipLaunchKernelGGL(k_sparse_write, dim3((unsigned)tiles, grid_y(n_sids)), dim3(kSparseThreads), 0,
                     (hipStream_t)stream, p, sid_lo, n_sids, tiles, tb, rtot, row_off, row_moff, ent_channel, ent_count,
                     msg);
  return (int)hipGetLastError();
}

int cg_launch_sparse_tokens(const GParams& p, int32_t sid_lo, int32_t n_sids, int32_t* out, void* stream) {
  const int64_t width = (int64_t)p.part_hi - p.part_lo;
  if (n_sids <= 0 || width <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(k_sparse_tokens, dim3((unsigned)((width + kSparseThreads - 1) / kSparseThreads), grid_y(n_sids)),
                     dim3(kSparseThreads), 0, (hipStream_t)stream, p, sid_lo, n_sids, out);
  return (int)hipGetLastError();
}

}  // namespace clsnap
