// cg_restore.hip -- restore a run from a snapshot (cl_graph_restore): what the build of a seed adds to
// the sparse collect's passes (cg_sparse.hip), and the kernel that seeds a run.
//
// The seed of a restored graph is the sparse collect of one completed snapshot kept on the device:
// the recorded node tokens as the initial token plane, one entry (channel, count) per channel with
// recorded messages in channel order, and the payloads back to back.  Two things are new here:
//   k_restore_tile_sums / _scan_tiles / _offsets
//                     moff = the exclusive prefix of the entries' counts, device-wide: a tile is
//                     kRsTile consecutive entries, kRsItems per lane; the tiles' sums, one
//                     workgroup's exclusive scan over them, then every tile's own prefix on its base.
//                     moff[i] is the index of entry i's first message among all n_msgs -- and, since
//                     the seed pushes the messages in (channel, position) order, its delay draw index.
//   k_restore_reduce  the largest count, the payload sum, the payloads that differ from 1 and the
//                     sum of the token plane, for cl_graph_seed_info and the history sizing.
// and the seed itself:
//   k_seed            one message per thread (grid-stride): message j finds its entry by a binary
//                     search of moff (the last entry with moff <= j), so a channel holding 32,768
//                     messages and eight million channels holding one each cost the same per
//                     message.  Ring slot q = j - moff[i] of the channel gets (receiveTime << 32) |
//                     payload, position 0 also writes the channel's hq word.  Plain stores; no two
//                     threads write the same word, and nothing else runs between the reset and the
//                     kernel after this one.
// and, for a partitioned run that starts from the seed (cl_graph_part_begin_seeded):
//   k_seed_share      this device's slice of the entries and of the messages, by two binary
//                     searches of the entries' channels at the bounds of the owned channel range.
//   k_seed_range      k_seed over that slice: the same search and stores per message (one device
//                     function serves both), global draw indices, the draw counter past the whole seed.
#include <hip/hip_runtime.h>

#include "cg_engine.h"

namespace clsnap {
namespace {

constexpr int32_t kRsThreads = 256;
constexpr int32_t kRsWaves = kRsThreads / 64;
constexpr int32_t kRsItems = 8;
constexpr int32_t kRsTile = kRsThreads * kRsItems;

// The lane's counts i0 + [0, kRsItems) (0 past the end) and their sum.
__device__ __forceinline__ uint64_t lane_counts(const int32_t* __restrict__ count, int64_t i0, int64_t n_ent,
                                                uint32_t (&c)[kRsItems]) {
  if (i0 + kRsItems <= n_ent) {  // (i0 is a multiple of kRsItems: two aligned 16-byte loads)
    const int4* c4 = reinterpret_cast<const int4*>(count + i0);
    const int4 a = c4[0], b = c4[1];
    c[0] = a.x, c[1] = a.y, c[2] = a.z, c[3] = a.w, c[4] = b.x, c[5] = b.y, c[6] = b.z, c[7] = b.w;
  } else {
#pragma unroll
    for (int32_t k = 0; k < kRsItems; ++k) c[k] = i0 + k < n_ent ? (uint32_t)count[i0 + k] : 0u;
  }
  uint64_t s = 0;
#pragma unroll
  for (int32_t k = 0; k < kRsItems; ++k) s += c[k];
  return s;
}

__global__ void __launch_bounds__(kRsThreads) k_restore_tile_sums(const int32_t* __restrict__ count, int64_t n_ent,
                                                                  unsigned long long* __restrict__ tiles) {
  __shared__ uint64_t lds[kRsWaves];
  uint32_t c[kRsItems];
  const uint64_t s = lane_counts(count, (int64_t)blockIdx.x * kRsTile + (int64_t)threadIdx.x * kRsItems, n_ent, c);
  uint64_t total;
  (void)cg_block_prefix<kRsWaves>(s, lds, total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// One workgroup: the tiles' sums become their exclusive prefix, in place.
__global__ void __launch_bounds__(kRsThreads) k_restore_scan_tiles(unsigned long long* __restrict__ tiles,
                                                                   int64_t n_tiles) {
  __shared__ uint64_t lds[kRsWaves];
  uint64_t carry = 0;
  for (int64_t t0 = 0; t0 < n_tiles; t0 += kRsThreads) {
    const int64_t t = t0 + threadIdx.x;
    const uint64_t v = t < n_tiles ? tiles[t] : 0;
    uint64_t total;
    const uint64_t x = cg_block_prefix<kRsWaves>(v, lds, total);
    if (t < n_tiles) tiles[t] = carry + x;
    carry += total;
  }
}

__global__ void __launch_bounds__(kRsThreads) k_restore_offsets(const int32_t* __restrict__ count, int64_t n_ent,
                                                                const unsigned long long* __restrict__ tiles,
                                                                long long* __restrict__ moff) {
  __shared__ uint64_t lds[kRsWaves];
  const int64_t i0 = (int64_t)blockIdx.x * kRsTile + (int64_t)threadIdx.x * kRsItems;
  uint32_t c[kRsItems];
  const uint64_t s = lane_counts(count, i0, n_ent, c);
  uint64_t total;
  uint64_t at = tiles[blockIdx.x] + cg_block_prefix<kRsWaves>(s, lds, total);
#pragma unroll
  for (int32_t k = 0; k < kRsItems; ++k) {
    if (i0 + k < n_ent) moff[i0 + k] = (long long)at;
    at += c[k];
  }
}

// out[0] max= count, out[1] += payloads, out[2] += payloads != 1, out[3] += tok.
__global__ void __launch_bounds__(kRsThreads) k_restore_reduce(const int32_t* __restrict__ count, int64_t n_ent,
                                                               const int32_t* __restrict__ msgs, int64_t n_msgs,
                                                               const int32_t* __restrict__ tok, int64_t n,
                                                               unsigned long long* __restrict__ out) {
  __shared__ uint64_t lds[4][kRsWaves];
  uint64_t mx = 0, pay = 0, odd = 0, ts = 0;
  const int64_t stride = (int64_t)gridDim.x * kRsThreads;
  for (int64_t i = (int64_t)blockIdx.x * kRsThreads + threadIdx.x; i < n_ent; i += stride) {
    const uint64_t c = (uint32_t)count[i];
    mx = c > mx ? c : mx;
  }
  if (msgs)
    for (int64_t i = (int64_t)blockIdx.x * kRsThreads + threadIdx.x; i < n_msgs; i += stride) {
      const uint32_t m = (uint32_t)msgs[i];
      pay += m;
      odd += m != 1u;
    }
  for (int64_t i = (int64_t)blockIdx.x * kRsThreads + threadIdx.x; i < n; i += stride) ts += (uint64_t)(int64_t)tok[i];
#pragma unroll
  for (int32_t o = 32; o > 0; o >>= 1) {
    const uint64_t m2 = __shfl_down(mx, o);
    mx = m2 > mx ? m2 : mx;
    pay += __shfl_down(pay, o);
    odd += __shfl_down(odd, o);
    ts += __shfl_down(ts, o);
  }
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[0][wave] = mx, lds[1][wave] = pay, lds[2][wave] = odd, lds[3][wave] = ts;
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = pay = odd = ts = 0;
    for (int32_t w = 0; w < kRsWaves; ++w) {
      mx = lds[0][w] > mx ? lds[0][w] : mx;
      pay += lds[1][w];
      odd += lds[2][w];
      ts += lds[3][w];
    }
    if (mx) atomicMax(&out[0], (unsigned long long)mx);
    if (pay) atomicAdd(&out[1], (unsigned long long)pay);
    if (odd) atomicAdd(&out[2], (unsigned long long)odd);
    if (ts) atomicAdd(&out[3], (unsigned long long)ts);
  }
}

// GetReceiveTime (sim.go:100-102) of draw index k at simulator time 0 (cg_kernels.hip
// receive_time; the caller has checked k against the schedule's length).
__device__ __forceinline__ uint32_t seed_receive_time(const GParams& p, uint64_t k) {
  const uint32_t d = p.delay_mode == 0 ? (uint32_t)((cg_hash(p.delay_seed, k, 0) >> 32) % 5u) : p.sched[k];
  return 1u + d;
}

// What cannot be seeded, judged on the whole seed: it freezes the run before its first event, and
// queues nothing.
__device__ __forceinline__ int32_t seed_unseedable(const GParams& p, const GSeed& s) {
  if (s.max_count > ((int64_t)1 << p.cap_log2)) return ST_FIFO_OVERFLOW;
  if (p.delay_mode != 0 && s.n_msgs > p.sched_len) return ST_DELAY_EXHAUSTED;
  return ST_OK;
}

// Message j of the seed, whose entry lies in [lo, hi) with moff[lo] <= j: the last entry with
// moff <= j, then the ring slot and, at position 0, the channel's hq word.
__device__ __forceinline__ void seed_message(const GParams& p, const GSeed& s, int64_t j, int64_t lo, int64_t hi) {
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (s.moff[mid] <= j) lo = mid;
    else hi = mid;
  }
  const uint32_t q = (uint32_t)(j - s.moff[lo]);
  const int32_t c = s.channel[lo];
  const uint32_t rt = seed_receive_time(p, (uint64_t)j);
  const uint32_t pay = s.msgs ? (uint32_t)s.msgs[j] : 1u;
  p.fifo[((size_t)c << p.cap_log2) + q] = ((uint64_t)rt << 32) | pay;
  if (q == 0) p.hq[c] = ((uint64_t)((uint32_t)s.count[lo] << 16) << 32) | rt;  // head 0, count, head receiveTime
}

__global__ void __launch_bounds__(kRsThreads) k_seed(GParams p, GSeed s) {
  const int32_t bad = seed_unseedable(p, s);
  const int64_t gid = (int64_t)blockIdx.x * kRsThreads + threadIdx.x;
  if (gid == 0) {  // (after the reset: status 0, draw 0, counters 0)
    if (bad) {
      p.sc->status = bad;
    } else {
      p.sc->draw = (unsigned long long)s.n_msgs;
      p.cpart[GC_PUSH] += (unsigned long long)s.n_msgs;
    }
  }
  if (bad) return;
  const int64_t stride = (int64_t)gridDim.x * kRsThreads;
  for (int64_t j = gid; j < s.n_msgs; j += stride) seed_message(p, s, j, 0, s.n_ent);  // (moff[0] = 0)
}

// The share of a partitioned run's device (cl_graph_part_begin_seeded): the owned channels are
// [out_off[part_lo], out_off[part_hi]), so its entries are [e_lo, e_hi) = the first entries with
// a channel at or above either bound, and its messages [moff[e_lo], moff[e_hi]) of the global
// draw order (moff[n_ent] = n_msgs).  Lane 0 finds the lower pair, lane 1 the upper:
// share[0..4) = e_lo, e_hi, m_lo, m_hi.
__global__ void __launch_bounds__(64) k_seed_share(GParams p, GSeed s, long long* __restrict__ share) {
  if (threadIdx.x > 1 || blockIdx.x) return;
  const int32_t bound = p.out_off[threadIdx.x ? p.part_hi : p.part_lo];
  int64_t lo = 0, hi = s.n_ent;  // the first entry with channel >= bound (n_ent: none)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (s.channel[mid] < bound) lo = mid + 1;
    else hi = mid;
  }
  share[threadIdx.x] = lo;
  share[2 + threadIdx.x] = lo < s.n_ent ? s.moff[lo] : s.n_msgs;
}

// k_seed over this device's share alone: message j of [m_lo, m_hi) keeps its global draw index j
// and searches the entries [e_lo, e_hi) only (moff[e_lo] = m_lo <= j), so an owned channel gets
// the very words k_seed writes for it and every other channel none.  The verdict on what cannot
// be seeded is the whole seed's, the same on every device; the draw counter starts past all n_msgs
// draws and GC_PUSH counts the messages queued here -- also when the share is empty.
__global__ void __launch_bounds__(kRsThreads) k_seed_range(GParams p, GSeed s, const long long* __restrict__ share) {
  const int32_t bad = seed_unseedable(p, s);
  const int64_t e_lo = share[0], e_hi = share[1], m_lo = share[2], m_hi = share[3];
  const int64_t gid = (int64_t)blockIdx.x * kRsThreads + threadIdx.x;
  if (gid == 0) {  // (after the reset: status 0, draw 0, counters 0)
    if (bad) {
      p.sc->status = bad;
    } else {
      p.sc->draw = (unsigned long long)s.n_msgs;
      p.cpart[GC_PUSH] += (unsigned long long)(m_hi - m_lo);
    }
  }
  if (bad) return;
  const int64_t stride = (int64_t)gridDim.x * kRsThreads;
  for (int64_t j = m_lo + gid; j < m_hi; j += stride) seed_message(p, s, j, e_lo, e_hi);
}

inline unsigned grid_for(int64_t n, int64_t most) {
  const int64_t g = (n + kRsThreads - 1) / kRsThreads;
  return (unsigned)(g < 1 ? 1 : g > most ? most : g);
}

}  // namespace

int64_t cg_restore_tiles(int64_t n_ent) {
  const int64_t t = (n_ent + kRsTile - 1) / kRsTile;
  return t > 0 ? t : 1;
}

int cg_launch_restore_offsets(const int32_t* count, int64_t n_ent, long long* moff, unsigned long long* tiles,
                              void* stream) {
  if (n_ent <= 0) return (int)hipSuccess;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n_tiles = cg_restore_tiles(n_ent);
  hipLaunchKernelGGL(k_restore_tile_sums, dim3((unsigned)n_tiles), dim3(kRsThreads), 0, s, count, n_ent, tiles);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_restore_scan_tiles, dim3(1), dim3(kRsThreads), 0, s, tiles, n_tiles);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_restore_offsets, dim3((unsigned)n_tiles), dim3(kRsThreads), 0, s, count, n_ent, tiles, moff);
  return (int)hipGetLastError();
}

int cg_launch_restore_reduce(const int32_t* count, int64_t n_ent, const int32_t* msgs, int64_t n_msgs,
                             const int32_t* tok, int64_t n, unsigned long long* out, void* stream) {
  int64_t m = n_ent > n ? n_ent : n;
  if (msgs && n_msgs > m) m = n_msgs;
  hipLaunchKernelGGL(k_restore_reduce, dim3(grid_for(m, 2048)), dim3(kRsThreads), 0, (hipStream_t)stream, count, n_ent,
                     msgs, n_msgs, tok, n, out);
  return (int)hipGetLastError();
}

int cg_launch_seed(const GParams& p, const GSeed& s, void* stream) {
  hipLaunchKernelGGL(k_seed, dim3(grid_for(s.n_msgs, 65535)), dim3(kRsThreads), 0, (hipStream_t)stream, p, s);
  return (int)hipGetLastError();
}

int cg_launch_seed_share(const GParams& p, const GSeed& s, long long* share, void* stream) {
  hipLaunchKernelGGL(k_seed_share, dim3(1), dim3(64), 0, (hipStream_t)stream, p, s, share);
  return (int)hipGetLastError();
}

int cg_launch_seed_range(const GParams& p, const GSeed& s, const long long* share, void* stream) {
  // (the share is on the device only: the grid covers the whole seed, of which it is a slice)
  hipLaunchKernelGGL(k_seed_range, dim3(grid_for(s.n_msgs, 65535)), dim3(kRsThreads), 0, (hipStream_t)stream, p, s,
                     share);
  return (int)hipGetLastError();
}

}  // namespace clsnap
