// cg_wave.hip -- marker-wave profile and marker tree of the graph engine's snapshots
// (cl_graph_snapshot_wave, cl_graph_snapshot_tree; DESIGN.md §10 'Marker wave and tree').
//
// The creation key W of a node's SNode record is (creation tick << 32) | creating sender, so
// the node part of the snapshot planes already holds, per snapshot id, when the marker wave
// reached every node and along which spanning tree.  Nothing else is read here: no channel plane.
//
//   k_wave_init   one row per sid at its identities; the origin the latencies are measured from
//                 is the caller's, or the creation tick of the initiator's record.
//   k_wave        the reduction (the shape of cg_table.hip's k_table: grid (x, sids), grid-stride,
//                 two 16-byte record loads in flight per lane): latency = tick - origin per
//                 created node into moments (registers, then shuffles, then LDS) and a histogram
//                 (LDS per workgroup, flushed with 64-bit atomics, non-zero bins only); with the
//                 depth on, the node's resolved {ancestor, hops} pair the same way.
//   k_wave_link   depth, step 0: every created node's pair is {parent, 1} -- after the guard
//   k_wave_jump   depth, one pointer-doubling round in place: {a, h} <- {anc(a), h + hops(a)}
//   k_wave_pack   the tree: records -> int32 parent / tick planes over the owned ranks.
//
// The pair.  One 8-byte word per (sid, node): lo32 = ancestor, hi32 = hops.  ancestor >= 0 is a
// node rank `hops` tree edges above; the terminal values say where the chain ended and `hops` is
// then the whole distance: kAtRoot at the initiator (hops = the depth), kAtBroken at a node the
// guard cut loose.  kNone: no local snapshot.  Every version a pair goes through names a true
// ancestor at a true distance, and a pair is read and written as one aligned 8-byte access, so a
// round that reads a pair another lane of the same launch has or has not yet rewritten -- a
// copy gone stale in another XCD's L2 included -- still composes two true statements.
//
// The guard.  k_wave_link accepts a parent only if it lies in [0, n), holds a local snapshot of
// the sid and was created at a strictly smaller tick: ancestors then only ever come from accepted
// links (no load outside the plane), and ticks fall strictly along a chain (no cycle, so the
// rounds end).  A node that fails is a root that is not the initiator; whatever hangs below it
// is left out of the depth fields and counted in CL_WV_BROKEN, which is 0 in every run.
#include <hip/hip_runtime.h>

#include "cg_engine.h"

namespace clsnap {
namespace {

// The reduction takes k_table's grid (cg_table.hip): few large workgroups per sid, since the
// closing atomics of one sid's workgroups land on one row.
constexpr int32_t kWaveThreads = 512;
constexpr int32_t kWaveWaves = kWaveThreads / 64;
constexpr int32_t kWaveBlocksPerCu = 4;
constexpr int32_t kWaveSharePerCu = 2;
constexpr int32_t kWaveItems = 4;
constexpr int32_t kWaveMaxBins = 1024;  // CL_GRAPH_WAVE_MAX_BINS
// link / jump / pack: one pair per thread, grid (node blocks, sids)
constexpr int32_t kLinkThreads = 256;
constexpr long long kI64Max = 0x7fffffffffffffffLL;
constexpr long long kI64Min = -kI64Max - 1;

// Head words of a row (CL_WV_*, include/clgraph.h); the histograms follow at WV_HEAD.
enum WaveWord : int32_t {
  WV_SID = 0, WV_ORIGIN, WV_CREATED, WV_LAT_SUM, WV_LAT_SUMSQ, WV_LAT_MIN, WV_LAT_MAX, WV_DEPTH_SUM, WV_DEPTH_SUMSQ,
  WV_DEPTH_MAX, WV_BROKEN, WV_HEAD = 12
};
// The reduced words WV_CREATED .. WV_BROKEN are LDS slots 0 .. 8 in row order.
constexpr int32_t kWaveSlots = 9;
enum SlotOp : int32_t { OP_ADD = 0, OP_MIN = 1, OP_MAX = 2 };
__device__ constexpr int32_t kSlotOp[kWaveSlots] = {OP_ADD, OP_ADD, OP_ADD, OP_MIN, OP_MAX, OP_ADD, OP_ADD, OP_MAX, OP_ADD};
__device__ constexpr long long kSlotIdentity[kWaveSlots] = {0, 0, 0, kI64Max, kI64Min, 0, 0, -1, 0};

constexpr int32_t kAtRoot = -1, kNone = -2, kAtBroken = -3;
constexpr unsigned long long kNoW = ~0ull;

__device__ __forceinline__ unsigned long long make_pair(int32_t anc, int32_t hops) {
  return (unsigned long long)(uint32_t)anc | ((unsigned long long)(uint32_t)hops << 32);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// One 16-byte load per lane, kept whole (cg_table.hip keep16).
__device__ __forceinline__ u32x4 load16(const u32x4* p) { return *p; }
__device__ __forceinline__ void keep16(u32x4& x) { asm volatile("" : "+v"(x)); }

__device__ __forceinline__ long long fold(long long v, long long w, int32_t op) {
  return op == OP_ADD ? (long long)((unsigned long long)v + (unsigned long long)w)
                      : op == OP_MIN ? (w < v ? w : v) : (w > v ? w : v);
}
__device__ __forceinline__ long long wave_fold(long long v, int32_t op) {
  for (int o = 32; o > 0; o >>= 1) v = fold(v, __shfl_xor(v, o), op);
  return v;
}

// Rows [0, n_rows) of the snapshots sid_lo + r at their identities.  org[r]: the caller's origin
// (user != 0), else the rank of the snapshot's initiator (-1: unknown), whose record's creation
// tick is the origin -- -1 when this device does not hold that record.
__global__ void __launch_bounds__(kLinkThreads) k_wave_init(GParams p, const long long* __restrict__ org, int32_t user,
                                                            int32_t sid_lo, int32_t n_rows, int32_t rw, long long* rows) {
  const int64_t i = (int64_t)blockIdx.x * kLinkThreads + threadIdx.x;
  if (i >= (int64_t)n_rows * rw) return;
  const int32_t r = (int32_t)(i / rw), f = (int32_t)(i - (int64_t)r * rw), sid = sid_lo + r;
  long long v = 0;
  if (f == WV_SID) v = sid;
  else if (f == WV_ORIGIN) {
    v = org[r];
    if (!user) {
      const long long node = v;
      v = -1;
      if (node >= p.part_lo && node < p.part_hi) {
        const unsigned long long W = p.sn[(size_t)sid * p.n + (size_t)node].W;
        if (W != kNoW && (uint32_t)W == 0xffffffffu) v = (long long)(W >> 32);
      }
    }
  } else if (f == WV_LAT_MIN) v = kI64Max;
  else if (f == WV_LAT_MAX) v = kI64Min;
  else if (f == WV_DEPTH_MAX) v = -1;
  rows[i] = v;
}

// pairs: [n_rows][p.n] resolved pairs of the snapshots sid_lo + r (kDepth only).
template <bool kDepth>
__global__ void __launch_bounds__(kWaveThreads) k_wave(GParams p, int32_t sid_lo, int32_t n_rows, int32_t rw,
                                                       int32_t lat_bins, int32_t lat_width, int32_t depth_bins,
                                                       int32_t user, const unsigned long long* __restrict__ pairs,
                                                       long long* rows) {
  __shared__ long long part[kWaveWaves][kWaveSlots];
  __shared__ uint32_t hist[kDepth ? 2 * kWaveMaxBins : kWaveMaxBins];  // latency bins, then depth bins
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gt = (int64_t)blockIdx.x * kWaveThreads + threadIdx.x, gs = (int64_t)gridDim.x * kWaveThreads;
  const int32_t bins = lat_bins + (kDepth ? depth_bins : 0);
  // latencies at or above lat_width * lat_bins clamp to the last bin; below it the quotient is
  // taken in 32 bits whenever the limit fits (a 64-bit division is a long emulated sequence)
  const unsigned long long lat_lim = (unsigned long long)lat_width * (unsigned long long)lat_bins;
  const bool narrow = lat_lim <= 0x100000000ull;

  for (int32_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
    long long* row = rows + (size_t)r * rw;
    const long long origin = row[WV_ORIGIN];  // (k_wave_init's; uniform over the workgroup)
    if (!user && origin < 0) continue;        // the initiator's record is not here: identities
    const int32_t sid = sid_lo + r;
    for (int32_t b = threadIdx.x; b < bins; b += kWaveThreads) hist[b] = 0;
    __syncthreads();
    const u32x4* sn = reinterpret_cast<const u32x4*>(p.sn + (size_t)sid * p.n);
    const unsigned long long* pr = kDepth ? pairs + (size_t)r * p.n : nullptr;
    unsigned long long created = 0, lat_sq = 0, dep_sum = 0, dep_sq = 0, broken = 0;
    long long lat_sum = 0, lat_min = kI64Max, lat_max = kI64Min;
    int32_t dep_max = -1;
    // x: W lo32 (creating sender), W hi32 (creation tick), cnt, stok; q: the node's pair
    auto node = [&](const u32x4 x, unsigned long long q) {
      if ((x.x & x.y) == 0xffffffffu) return;  // W == ~0: no local snapshot
      const long long lat = (long long)(int32_t)x.y - origin;
      created += 1;
      lat_sum = (long long)((unsigned long long)lat_sum + (unsigned long long)lat);
      lat_sq += (unsigned long long)lat * (unsigned long long)lat;
      lat_min = lat < lat_min ? lat : lat_min;
      lat_max = lat > lat_max ? lat : lat_max;
      int32_t b = 0;
      if (lat >= 0) {
        const unsigned long long u = (unsigned long long)lat;
        b = u >= lat_lim ? lat_bins - 1
                         : narrow ? (int32_t)((uint32_t)u / (uint32_t)lat_width) : (int32_t)(u / (uint32_t)lat_width);
      }
      atomicAdd(&hist[b], 1u);
      if (kDepth) {
        const int32_t anc = (int32_t)(uint32_t)q, hops = (int32_t)(uint32_t)(q >> 32);
        if (anc == kAtRoot) {
          dep_sum += (unsigned long long)hops;
          dep_sq += (unsigned long long)hops * (unsigned long long)hops;
          dep_max = hops > dep_max ? hops : dep_max;
          atomicAdd(&hist[lat_bins + (hops < depth_bins - 1 ? hops : depth_bins - 1)], 1u);
        } else {
          broken += 1;  // under a root the guard made (or, after the last round, not resolved)
        }
      }
    };
    int64_t v = p.part_lo + gt;
    for (; v + gs < p.part_hi; v += 2 * gs) {  // two records in flight per lane
      u32x4 x0 = load16(sn + v), x1 = load16(sn + v + gs);
      const unsigned long long q0 = kDepth ? pr[v] : 0, q1 = kDepth ? pr[v + gs] : 0;
      keep16(x0), keep16(x1);
      node(x0, q0), node(x1, q1);
    }
    if (v < p.part_hi) {
      u32x4 x0 = load16(sn + v);
      const unsigned long long q0 = kDepth ? pr[v] : 0;
      keep16(x0);
      node(x0, q0);
    }
    // ---- wave, then workgroup, then one atomic per word and per non-zero bin
    const long long mine[kWaveSlots] = {(long long)created, lat_sum, (long long)lat_sq, lat_min, lat_max,
                                        (long long)dep_sum, (long long)dep_sq, (long long)dep_max, (long long)broken};
#pragma unroll
    for (int32_t s = 0; s < kWaveSlots; ++s) {
      const long long w = wave_fold(mine[s], kSlotOp[s]);
      if (lane == 0) part[wave][s] = w;
    }
    __syncthreads();  // (and every lane's histogram atomics are done)
    if (threadIdx.x < kWaveSlots) {
      const int32_t s = threadIdx.x, op = kSlotOp[s];
      long long t = part[0][s];
      for (int32_t w = 1; w < kWaveWaves; ++w) t = fold(t, part[w][s], op);
      if (t != kSlotIdentity[s]) {
        long long* dst = row + WV_CREATED + s;
        if (op == OP_ADD) atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)t);
        else if (op == OP_MIN) atomicMin(dst, t);
        else atomicMax(dst, t);
      }
    }
    for (int32_t b = threadIdx.x; b < bins; b += kWaveThreads) {
      const uint32_t c = hist[b];
      if (c) atomicAdd(reinterpret_cast<unsigned long long*>(row + WV_HEAD + b), (unsigned long long)c);
    }
    __syncthreads();  // (the next sid reuses `part` and `hist`)
  }
}

// pairs[r][v] of the snapshots sid_lo + r, r < n_rows, over all n nodes: the guarded first link.
__global__ void __launch_bounds__(kLinkThreads) k_wave_link(GParams p, int32_t sid_lo, int32_t n_rows,
                                                            unsigned long long* pairs) {
  const uint32_t n = (uint32_t)p.n;
  for (int32_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
    const SNode* sn = p.sn + (size_t)(sid_lo + r) * n;
    unsigned long long* pr = pairs + (size_t)r * n;
    for (int64_t v = (int64_t)blockIdx.x * kLinkThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kLinkThreads) {
      const unsigned long long W = sn[v].W;
      unsigned long long q = make_pair(kNone, 0);
      if (W != kNoW) {
        const uint32_t par = (uint32_t)W;
        if (par == 0xffffffffu) q = make_pair(kAtRoot, 0);  // the initiator
        else {
          bool ok = par < n;
          if (ok) {
            const unsigned long long Wp = sn[par].W;
            ok = Wp != kNoW && (uint32_t)(Wp >> 32) < (uint32_t)(W >> 32);
          }
          q = ok ? make_pair((int32_t)par, 1) : make_pair(kAtBroken, 0);
        }
      }
      pr[v] = q;
    }
  }
}

// One doubling round in place; *changed = 1 if any pair moved.
__global__ void __launch_bounds__(kLinkThreads) k_wave_jump(int32_t n, int32_t n_rows, unsigned long long* pairs,
                                                            int32_t* changed) {
  bool moved = false;
  for (int32_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
    unsigned long long* pr = pairs + (size_t)r * n;
    for (int64_t v = (int64_t)blockIdx.x * kLinkThreads + threadIdx.x; v < n; v += (int64_t)gridDim.x * kLinkThreads) {
      const unsigned long long a = pr[v];
      const int32_t anc = (int32_t)(uint32_t)a;
      if (anc < 0) continue;             // terminal, or no local snapshot
      const unsigned long long b = pr[anc];  // (anc came from an accepted link: inside the plane)
      int32_t up = (int32_t)(uint32_t)b;
      if (up == kNone) up = kAtBroken;   // (an accepted parent holds a local snapshot: not reached)
      pr[v] = make_pair(up, (int32_t)(uint32_t)(a >> 32) + (int32_t)(uint32_t)(b >> 32));
      moved = true;
    }
  }
  if (moved) *changed = 1;
}

// parent / tick planes [n_rows][part_hi - part_lo] of the snapshots sid_lo + r; tick may be null.
__global__ void __launch_bounds__(kLinkThreads) k_wave_pack(GParams p, int32_t sid_lo, int32_t n_rows, int32_t* parent,
                                                            int32_t* tick) {
  const int64_t width = (int64_t)p.part_hi - p.part_lo;
  for (int32_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
    const SNode* sn = p.sn + (size_t)(sid_lo + r) * p.n + p.part_lo;
    for (int64_t i = (int64_t)blockIdx.x * kLinkThreads + threadIdx.x; i < width; i += (int64_t)gridDim.x * kLinkThreads) {
      const unsigned long long W = sn[i].W;
      const bool made = W != kNoW;
      const uint32_t lo = (uint32_t)W;
      parent[(size_t)r * width + i] = !made ? -2 : lo == 0xffffffffu ? -1 : (int32_t)lo;
      if (tick) tick[(size_t)r * width + i] = made ? (int32_t)(uint32_t)(W >> 32) : -1;
    }
  }
}

dim3 pair_grid(int64_t width, int32_t n_rows) {
  int64_t gx = (width + kLinkThreads - 1) / kLinkThreads;
  if (gx < 1) gx = 1;
  if (gx > (1 << 20)) gx = 1 << 20;
  return dim3((unsigned)gx, (unsigned)(n_rows < 65535 ? n_rows : 65535));
}

}  // namespace

int cg_launch_wave_init(const GParams& p, const long long* org, int32_t user, int32_t sid_lo, int32_t n_rows, int32_t rw,
                        long long* rows, void* stream) {
  if (n_rows <= 0) return (int)hipSuccess;
  const int64_t cells = (int64_t)n_rows * rw;
  hipLaunchKernelGGL(k_wave_init, dim3((unsigned)((cells + kLinkThreads - 1) / kLinkThreads)), dim3(kLinkThreads), 0,
                     (hipStream_t)stream, p, org, user, sid_lo, n_rows, rw, rows);
  return (int)hipGetLastError();
}

int cg_launch_wave(const GParams& p, int32_t sid_lo, int32_t n_rows, int32_t rw, int32_t lat_bins, int32_t lat_width,
                   int32_t depth_bins, int32_t user, const unsigned long long* pairs, long long* rows, int32_t n_cus,
                   void* stream) {
  if (n_rows <= 0) return (int)hipSuccess;
  // k_table's grid (cg_table.hip): y strides over the sids, x shares one sid's plane
  const int64_t budget = (int64_t)kWaveBlocksPerCu * (n_cus > 0 ? n_cus : 1);
  const int64_t gy = n_rows < budget ? (n_rows < 65535 ? n_rows : 65535) : (budget < 65535 ? budget : 65535);
  const int64_t nodes = (int64_t)p.part_hi - p.part_lo, per = (int64_t)kWaveThreads * kWaveItems;
  int64_t gx = (nodes + per - 1) / per;
  if (gx > budget / gy) gx = budget / gy;
  const int64_t share = (int64_t)kWaveSharePerCu * (n_cus > 0 ? n_cus : 1);
  if (gx > share) gx = share;
  if (gx < 1) gx = 1;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (pairs)
    hipLaunchKernelGGL(k_wave<true>, grid, dim3(kWaveThreads), 0, (hipStream_t)stream, p, sid_lo, n_rows, rw, lat_bins,
                       lat_width, depth_bins, user, pairs, rows);
  else
    hipLaunchKernelGGL(k_wave<false>, grid, dim3(kWaveThreads), 0, (hipStream_t)stream, p, sid_lo, n_rows, rw, lat_bins,
                       lat_width, 0, user, pairs, rows);
  return (int)hipGetLastError();
}

int cg_launch_wave_link(const GParams& p, int32_t sid_lo, int32_t n_rows, unsigned long long* pairs, void* stream) {
  if (n_rows <= 0 || p.n <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(k_wave_link, pair_grid(p.n, n_rows), dim3(kLinkThreads), 0, (hipStream_t)stream, p, sid_lo, n_rows,
                     pairs);
  return (int)hipGetLastError();
}

int cg_launch_wave_jump(const GParams& p, int32_t n_rows, unsigned long long* pairs, int32_t* changed, void* stream) {
  if (n_rows <= 0 || p.n <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(k_wave_jump, pair_grid(p.n, n_rows), dim3(kLinkThreads), 0, (hipStream_t)stream, p.n, n_rows, pairs,
                     changed);
  return (int)hipGetLastError();
}

int cg_launch_wave_pack(const GParams& p, int32_t sid_lo, int32_t n_rows, int32_t* parent, int32_t* tick, void* stream) {
  if (n_rows <= 0 || p.part_hi <= p.part_lo) return (int)hipSuccess;
  hipLaunchKernelGGL(k_wave_pack, pair_grid((int64_t)p.part_hi - p.part_lo, n_rows), dim3(kLinkThreads), 0,
                     (hipStream_t)stream, p, sid_lo, n_rows, parent, tick);
  return (int)hipGetLastError();
}

}  // namespace clsnap
