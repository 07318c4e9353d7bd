// cg_profile.hip -- node and channel profile over a snapshot range (cl_graph_snapshot_profile).
//
// The other readouts give one row per snapshot id; this one reduces the other way: over the used
// snapshots of a range, one record per channel into an owned node (messages, token payloads,
// snapshots with a message, the peak and its sid) and one row per owned node (moments of the
// recorded tokens and of the creation latency, what its in-channels recorded).  The planes are
// snapshot-major -- sn[S * n], rec[S * e], histv by in-position -- so a lane that owns a node or a
// pair of in-positions reads lane-linear in every sid.  All integer: the result is a pure
// function of the run, the range, the mask, the origins and the spec, whatever the grid.
//
//   k_profile_used    one workgroup: the used rows (mask and completion) compacted into a list,
//                     their count into the head, and the origin of every row (the caller's, or the
//                     creation tick of the initiator's record: k_wave_init's gather).
//   k_profile_chan    grid (in-position pairs, slices).  A lane owns two consecutive in-positions
//                     from an even one on, so a cursor pair of a sid is one 16-byte load wherever
//                     sid * e is even (uniform over the grid), two 8-byte loads otherwise and at the
//                     range's ragged ends.  kProfileFlight sids in flight; histv only where a
//                     cursor pair is not empty.  blockIdx.y takes a contiguous slice of the used
//                     list: one slice stores its accumulators, several meet by 64-bit atomics (add,
//                     max) on planes the launcher zeroed.
//   k_profile_node    the same shape over the 16-byte SNode records of the owned nodes.
//   k_profile_in      in_msgs / in_tokens: the channel accumulators summed over every owned node's
//                     in-CSR range.  In-degree <= kProfileLaneDeg: the node's lane; <=
//                     kProfileWaveDeg: a wave, lane-strided; above: the workgroup.  No thread walks
//                     a hub's range alone.
//   k_profile_count   channel tiles as in cg_sparse.hip (ascending channels through route[c].y):
//                     the histogram in LDS and one atomic per non-zero bin, the head's sums and
//                     maxima folded per workgroup, and every tile's entry count.
//   k_profile_scan    one workgroup: the exclusive scan of the tile counts, the total into the head.
//   k_profile_fill    the entries of every tile at its base, in ascending channel order.
#include <hip/hip_runtime.h>

#include "cg_engine.h"

namespace clsnap {
namespace {

constexpr int32_t kProfileThreads = 256;
constexpr int32_t kProfileWaves = kProfileThreads / 64;
constexpr int32_t kProfileFlight = 4;  // sids in flight per lane
constexpr int32_t kProfileItems = 8;   // consecutive channels per lane of a channel tile
constexpr int32_t kProfileTile = kProfileThreads * kProfileItems;
constexpr int32_t kProfileBlocksPerCu = 4;  // workgroups per CU the slices fill the chip to
constexpr int32_t kProfileSliceSids = 8;    // fewest used rows worth a slice of their own
constexpr long long kI64Max = 0x7fffffffffffffffLL;
constexpr long long kI64Min = -kI64Max - 1;

// Head words the kernels write (CL_PF_*, include/clgraph.h).
enum : int32_t { PF_N_USED = 1, PF_ACTIVE = 5, PF_ENTRIES = 6, PF_MSGS = 7, PF_TOKENS = 8, PF_MAX_MSGS = 9,
                 PF_MAX_PEAK = 10, PF_MAX_SNAPS = 11, PF_HEAD = 16 };
enum : int32_t { PN_TOK_SUM = 0, PN_TOK_SUMSQ, PN_TOK_MIN, PN_TOK_MAX, PN_LAT_SUM, PN_LAT_MAX, PN_IN_MSGS,
                 PN_IN_TOKENS, kNodeWords = 8 };
static_assert(kNodeWords == kProfileNodeWords, "a node row is kProfileNodeWords int64");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 load16(const u32x4* p) { return *p; }
// (keeps a 16-byte load whole: cg_table.hip keep16)
__device__ __forceinline__ void keep16(u32x4& x) { asm volatile("" : "+v"(x)); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}

// Slice y of ny of the used list's n entries: [lo, hi), contiguous, empty past the end.
__device__ __forceinline__ void slice_of(int32_t n, int32_t y, int32_t ny, int32_t& lo, int32_t& hi) {
  const int32_t per = (n + ny - 1) / ny;
  lo = y * per < n ? y * per : n;
  hi = lo + per < n ? lo + per : n;
}

__global__ void __launch_bounds__(kProfileThreads) k_profile_used(GParams p, const int32_t* __restrict__ use,
                                                                  const long long* __restrict__ org_in, int32_t user,
                                                                  int32_t sid_lo, int32_t ns, int32_t* __restrict__ list,
                                                                  int32_t* __restrict__ used,
                                                                  long long* __restrict__ org, long long* head) {
  __shared__ uint64_t lds[kProfileWaves];
  uint64_t base = 0;
  for (int32_t r0 = 0; r0 < ns; r0 += kProfileThreads) {
    const int32_t r = r0 + threadIdx.x;
    uint64_t u = 0;
    if (r < ns) {
      const int32_t sid = sid_lo + r;
      u = (!use || use[r] != 0) && p.ctick[sid] >= 0 ? 1 : 0;
      used[r] = (int32_t)u;
      long long o = org_in[r];
      if (!user) {  // org_in[r]: the initiator's rank; its record's creation tick is the origin
        const long long node = o;
        o = -1;
        if (node >= p.part_lo && node < p.part_hi) {
          const unsigned long long W = p.sn[(size_t)sid * p.n + (size_t)node].W;
          if (W != ~0ull && (uint32_t)W == 0xffffffffu) o = (long long)(W >> 32);
        }
      }
      org[r] = o;
    }
    uint64_t total;
    const uint64_t x = cg_block_prefix<kProfileWaves>(u, lds, total);
    if (u) list[base + x] = r;
    base += total;
  }
  if (threadIdx.x == 0) head[PF_N_USED] = (long long)base;
}

struct ChanAcc {
  unsigned long long msgs = 0, toks = 0, pk = 0, snaps = 0;
};

// One cursor pair x of in-position k in used row r.
__device__ __forceinline__ void profile_channel(const GParams& p, int32_t k, int32_t r, uint64_t x, ChanAcc& a) {
  const uint32_t b = (uint32_t)x, e = (uint32_t)(x >> 32), cnt = e - b;
  if (cnt == 0) return;
  unsigned long long t = cnt;  // unit payloads
  if (p.hist) {
    t = 0;
    const uint32_t* h = p.histv + (size_t)k * p.hist;
    for (uint32_t q = b; q != e; ++q) t += q < (uint32_t)p.hist ? h[q] : 0;  // (cg_sparse.hip: no read past the history)
  }
  a.msgs += cnt;
  a.toks += t;
  a.snaps += 1;
  const unsigned long long cand = ((unsigned long long)cnt << 32) | (uint32_t)~(uint32_t)r;  // the lowest row wins a tie
  a.pk = cand > a.pk ? cand : a.pk;
}

template <bool ATOMIC>
__device__ __forceinline__ void store_channel(unsigned long long* __restrict__ acc, int64_t ke, int64_t i,
                                              const ChanAcc& a) {
  if (ATOMIC) {
    if (a.msgs == 0) return;
    atomicAdd(acc + i, a.msgs);
    atomicAdd(acc + ke + i, a.toks);
    atomicMax(acc + 2 * ke + i, a.pk);
    atomicAdd(acc + 3 * ke + i, a.snaps);
  } else {
    acc[i] = a.msgs;
    acc[ke + i] = a.toks;
    acc[2 * ke + i] = a.pk;
    acc[3 * ke + i] = a.snaps;
  }
}

// acc: four planes over the owned in-positions [k_lo, k_hi): msgs, tokens, (peak << 32 | ~row), snaps.
template <bool ATOMIC>
__global__ void __launch_bounds__(kProfileThreads) k_profile_chan(GParams p, int32_t k_lo, int32_t k_hi, int32_t sid_lo,
                                                                  const int32_t* __restrict__ list,
                                                                  const long long* __restrict__ head,
                                                                  unsigned long long* __restrict__ acc) {
  const int64_t k0l = (int64_t)(k_lo & ~1) + 2 * ((int64_t)blockIdx.x * kProfileThreads + threadIdx.x);
  if (k0l >= k_hi) return;
  const int32_t k0 = (int32_t)k0l;
  const bool v0 = k0 >= k_lo, v1 = k0 + 1 < k_hi;  // (the pair may stick out of the range at either end)
  int32_t lo, hi;
  slice_of((int32_t)head[PF_N_USED], blockIdx.y, gridDim.y, lo, hi);
  if (ATOMIC && lo == hi) return;
  ChanAcc a0, a1;
  auto load = [&](int32_t r, uint64_t& x0, uint64_t& x1) {
    const int64_t base = (int64_t)(sid_lo + r) * p.e;
    const uint64_t* rec = p.rec + base;
    if ((base & 1) == 0 && v0 && v1) {  // k0 is even: the pair is 16-byte aligned in this sid's plane
      u32x4 x = load16(reinterpret_cast<const u32x4*>(rec + k0));
      keep16(x);
      x0 = (uint64_t)x.x | ((uint64_t)x.y << 32);
      x1 = (uint64_t)x.z | ((uint64_t)x.w << 32);
    } else {
      x0 = v0 ? rec[k0] : 0;
      x1 = v1 ? rec[k0 + 1] : 0;
    }
  };
  int32_t i = lo;
  for (; i + kProfileFlight <= hi; i += kProfileFlight) {
    int32_t r[kProfileFlight];
    uint64_t x0[kProfileFlight], x1[kProfileFlight];
#pragma unroll
    for (int32_t u = 0; u < kProfileFlight; ++u) r[u] = list[i + u];
#pragma unroll
    for (int32_t u = 0; u < kProfileFlight; ++u) load(r[u], x0[u], x1[u]);
#pragma unroll
    for (int32_t u = 0; u < kProfileFlight; ++u) {
      profile_channel(p, k0, r[u], x0[u], a0);
      profile_channel(p, k0 + 1, r[u], x1[u], a1);
    }
  }
  for (; i < hi; ++i) {
    const int32_t r = list[i];
    uint64_t x0, x1;
    load(r, x0, x1);
    profile_channel(p, k0, r, x0, a0);
    profile_channel(p, k0 + 1, r, x1, a1);
  }
  const int64_t ke = (int64_t)k_hi - k_lo;
  if (v0) store_channel<ATOMIC>(acc, ke, (int64_t)k0 - k_lo, a0);
  if (v1) store_channel<ATOMIC>(acc, ke, (int64_t)k0 + 1 - k_lo, a1);
}

// rows[(v - part_lo) * 8 + w] at the identities of the node words (for the atomics of several slices).
__global__ void __launch_bounds__(kProfileThreads) k_profile_node_init(int64_t words, long long* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * kProfileThreads + threadIdx.x;
  if (i >= words) return;
  const int32_t w = (int32_t)(i & (kNodeWords - 1));
  rows[i] = w == PN_TOK_MIN ? kI64Max : w == PN_TOK_MAX || w == PN_LAT_MAX ? kI64Min : 0;
}

template <bool ATOMIC>
__global__ void __launch_bounds__(kProfileThreads) k_profile_node(GParams p, int32_t sid_lo,
                                                                  const int32_t* __restrict__ list,
                                                                  const long long* __restrict__ org,
                                                                  const long long* __restrict__ head,
                                                                  long long* __restrict__ rows) {
  const int64_t v = (int64_t)p.part_lo + (int64_t)blockIdx.x * kProfileThreads + threadIdx.x;
  if (v >= p.part_hi) return;
  int32_t lo, hi;
  slice_of((int32_t)head[PF_N_USED], blockIdx.y, gridDim.y, lo, hi);
  if (ATOMIC && lo == hi) return;
  unsigned long long tok_sum = 0, tok_sq = 0, lat_sum = 0;
  long long tok_min = kI64Max, tok_max = kI64Min, lat_max = kI64Min;
  // x: W lo32 (creating sender), W hi32 (creation tick), cnt, stok -- a used snapshot is complete, so v holds one
  auto node = [&](const u32x4 x, long long origin) {
    const long long st = (int32_t)x.w, lat = (long long)(int32_t)x.y - origin;
    tok_sum += (unsigned long long)st;
    tok_sq += (unsigned long long)st * (unsigned long long)st;
    tok_min = st < tok_min ? st : tok_min;
    tok_max = st > tok_max ? st : tok_max;
    lat_sum += (unsigned long long)lat;
    lat_max = lat > lat_max ? lat : lat_max;
  };
  const u32x4* sn = reinterpret_cast<const u32x4*>(p.sn) + v;
  int32_t i = lo;
  for (; i + kProfileFlight <= hi; i += kProfileFlight) {
    u32x4 x[kProfileFlight];
    long long o[kProfileFlight];
#pragma unroll
    for (int32_t u = 0; u < kProfileFlight; ++u) {
      const int32_t r = list[i + u];
      x[u] = load16(sn + (size_t)(sid_lo + r) * p.n);
      o[u] = org[r];
    }
#pragma unroll
    for (int32_t u = 0; u < kProfileFlight; ++u) {
      keep16(x[u]);
      node(x[u], o[u]);
    }
  }
  for (; i < hi; ++i) {
    const int32_t r = list[i];
    u32x4 x = load16(sn + (size_t)(sid_lo + r) * p.n);
    keep16(x);
    node(x, org[r]);
  }
  long long* row = rows + (v - p.part_lo) * kNodeWords;
  if (ATOMIC) {
    atomicAdd(reinterpret_cast<unsigned long long*>(row + PN_TOK_SUM), tok_sum);
    atomicAdd(reinterpret_cast<unsigned long long*>(row + PN_TOK_SUMSQ), tok_sq);
    atomicMin(row + PN_TOK_MIN, tok_min);
    atomicMax(row + PN_TOK_MAX, tok_max);
    atomicAdd(reinterpret_cast<unsigned long long*>(row + PN_LAT_SUM), lat_sum);
    atomicMax(row + PN_LAT_MAX, lat_max);
  } else {
    row[PN_TOK_SUM] = (long long)tok_sum;
    row[PN_TOK_SUMSQ] = (long long)tok_sq;
    row[PN_TOK_MIN] = tok_min;
    row[PN_TOK_MAX] = tok_max;
    row[PN_LAT_SUM] = (long long)lat_sum;
    row[PN_LAT_MAX] = lat_max;
  }
}

// in_msgs / in_tokens of every owned node: msgs and tokens of `acc` over its in-CSR range.
__global__ void __launch_bounds__(kProfileThreads) k_profile_in(GParams p, int32_t k_lo, int64_t ke,
                                                                const unsigned long long* __restrict__ acc,
                                                                long long* __restrict__ rows) {
  __shared__ int32_t wave_nodes[kProfileThreads], block_nodes[kProfileThreads];
  __shared__ int32_t n_wave, n_block;
  __shared__ unsigned long long red[kProfileWaves][2];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long* msgs = acc - k_lo;  // (indexed by in-position)
  const unsigned long long* toks = acc + ke - k_lo;
  if (threadIdx.x == 0) n_wave = n_block = 0;
  __syncthreads();
  const int64_t v = (int64_t)p.part_lo + (int64_t)blockIdx.x * kProfileThreads + threadIdx.x;
  if (v < p.part_hi) {
    const int32_t lo = p.in_off[v], hi = p.in_off[v + 1], deg = hi - lo;
    if (deg <= kProfileLaneDeg) {
      unsigned long long m = 0, t = 0;
      for (int32_t k = lo; k < hi; ++k) m += msgs[k], t += toks[k];
      long long* row = rows + (v - p.part_lo) * kNodeWords;
      row[PN_IN_MSGS] = (long long)m;
      row[PN_IN_TOKENS] = (long long)t;
    } else if (deg <= kProfileWaveDeg) {
      wave_nodes[atomicAdd(&n_wave, 1)] = (int32_t)v;
    } else {
      block_nodes[atomicAdd(&n_block, 1)] = (int32_t)v;
    }
  }
  __syncthreads();
  const int32_t nw = n_wave, nb = n_block;  // (uniform over the workgroup)
  for (int32_t i = wave; i < nw; i += kProfileWaves) {
    const int32_t u = wave_nodes[i], lo = p.in_off[u], hi = p.in_off[u + 1];
    unsigned long long m = 0, t = 0;
    for (int32_t k = lo + lane; k < hi; k += 64) m += msgs[k], t += toks[k];
    m = wave_sum(m), t = wave_sum(t);
    if (lane == 0) {
      long long* row = rows + (int64_t)(u - p.part_lo) * kNodeWords;
      row[PN_IN_MSGS] = (long long)m;
      row[PN_IN_TOKENS] = (long long)t;
    }
  }
  for (int32_t i = 0; i < nb; ++i) {
    const int32_t u = block_nodes[i], lo = p.in_off[u], hi = p.in_off[u + 1];
    unsigned long long m = 0, t = 0;
    for (int32_t k = lo + (int32_t)threadIdx.x; k < hi; k += kProfileThreads) m += msgs[k], t += toks[k];
    m = wave_sum(m), t = wave_sum(t);
    if (lane == 0) red[wave][0] = m, red[wave][1] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
      m = t = 0;
      for (int32_t w = 0; w < kProfileWaves; ++w) m += red[w][0], t += red[w][1];
      long long* row = rows + (int64_t)(u - p.part_lo) * kNodeWords;
      row[PN_IN_MSGS] = (long long)m;
      row[PN_IN_TOKENS] = (long long)t;
    }
    __syncthreads();  // (the next node's partials reuse `red`)
  }
}

// In-positions of the lane's channels c0 + [0, kProfileItems), -1 for a channel past the end or
// into a node this device does not own (cg_sparse.hip tile_inpos).
__device__ __forceinline__ void tile_inpos(const GParams& p, int64_t c0, int32_t (&k)[kProfileItems]) {
#pragma unroll
  for (int32_t i = 0; i < kProfileItems; ++i) {
    k[i] = -1;
    if (c0 + i < p.e) {
      const int2 r = p.route[c0 + i];
      if (r.x >= p.part_lo && r.x < p.part_hi) k[i] = r.y;
    }
  }
}

constexpr int32_t kCountSlots = 7;  // active, msgs, tokens, entries (sums); max msgs, max peak, max snaps
__device__ constexpr int32_t kCountWord[kCountSlots] = {PF_ACTIVE, PF_MSGS, PF_TOKENS, PF_ENTRIES, PF_MAX_MSGS,
                                                        PF_MAX_PEAK, PF_MAX_SNAPS};
__global__ void __launch_bounds__(kProfileThreads) k_profile_count(GParams p, int32_t k_lo, int64_t ke,
                                                                   const unsigned long long* __restrict__ acc,
                                                                   int32_t min_msgs, int32_t bins, int32_t width,
                                                                   long long* head, unsigned long long* __restrict__ tiles) {
  __shared__ uint32_t hist[kProfileMaxBins];
  __shared__ unsigned long long part[kProfileWaves][kCountSlots];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int32_t b = threadIdx.x; b < bins; b += kProfileThreads) hist[b] = 0;
  __syncthreads();
  const int64_t c0 = (int64_t)blockIdx.x * kProfileTile + (int64_t)threadIdx.x * kProfileItems;
  int32_t k[kProfileItems];
  tile_inpos(p, c0, k);
  unsigned long long mine[kCountSlots] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int32_t i = 0; i < kProfileItems; ++i) {
    if (k[i] < 0) continue;
    const int64_t at = (int64_t)k[i] - k_lo;
    const unsigned long long m = acc[at], t = acc[ke + at], pk = acc[2 * ke + at], s = acc[3 * ke + at];
    mine[0] += m != 0;
    mine[1] += m;
    mine[2] += t;
    mine[3] += m >= (unsigned long long)min_msgs;
    mine[4] = m > mine[4] ? m : mine[4];
    mine[5] = (pk >> 32) > mine[5] ? (pk >> 32) : mine[5];
    mine[6] = s > mine[6] ? s : mine[6];
    const unsigned long long q = width == 1 ? m : m / (unsigned long long)width;
    atomicAdd(&hist[q < (unsigned long long)(bins - 1) ? (int32_t)q : bins - 1], 1u);
  }
#pragma unroll
  for (int32_t s = 0; s < kCountSlots; ++s) {
    const unsigned long long w = s < 4 ? wave_sum(mine[s]) : wave_max(mine[s]);
    if (lane == 0) part[wave][s] = w;
  }
  __syncthreads();
  for (int32_t b = threadIdx.x; b < bins; b += kProfileThreads)
    if (hist[b]) atomicAdd(reinterpret_cast<unsigned long long*>(head + PF_HEAD + b), (unsigned long long)hist[b]);
  if (threadIdx.x < kCountSlots) {
    const int32_t s = threadIdx.x;
    unsigned long long v = part[0][s];
    for (int32_t w = 1; w < kProfileWaves; ++w) v = s < 4 ? v + part[w][s] : (part[w][s] > v ? part[w][s] : v);
    if (s == 3) tiles[blockIdx.x] = v;
    else if (v != 0) {  // 0: the identity of every slot
      unsigned long long* dst = reinterpret_cast<unsigned long long*>(head + kCountWord[s]);
      if (s < 4) atomicAdd(dst, v);
      else atomicMax(dst, v);
    }
  }
}

// The tiles' entry counts become their exclusive prefix, in place; the total is the head's ENTRIES.
__global__ void __launch_bounds__(kProfileThreads) k_profile_scan(int32_t n_tiles, unsigned long long* __restrict__ tiles,
                                                                  long long* __restrict__ head) {
  __shared__ uint64_t lds[kProfileWaves];
  uint64_t carry = 0;
  for (int32_t t0 = 0; t0 < n_tiles; t0 += kProfileThreads) {
    const int32_t t = t0 + threadIdx.x;
    const uint64_t v = t < n_tiles ? tiles[t] : 0;
    uint64_t total;
    const uint64_t x = cg_block_prefix<kProfileWaves>(v, lds, total);
    if (t < n_tiles) tiles[t] = carry + x;
    carry += total;
  }
  if (threadIdx.x == 0) head[PF_ENTRIES] = (long long)carry;
}

struct alignas(16) ProfileEntry {  // cl_graph_profile_entry (include/clgraph.h)
  int32_t channel, snaps, peak, peak_sid;
  long long msgs, tokens;
};
static_assert(sizeof(ProfileEntry) == kProfileEntryBytes, "cl_graph_profile_entry is 32 bytes");

__global__ void __launch_bounds__(kProfileThreads) k_profile_fill(GParams p, int32_t k_lo, int64_t ke, int32_t sid_lo,
                                                                  const unsigned long long* __restrict__ acc,
                                                                  int32_t min_msgs, int32_t n_tiles,
                                                                  const unsigned long long* __restrict__ tiles,
                                                                  const long long* __restrict__ head,
                                                                  ProfileEntry* __restrict__ ent) {
  __shared__ uint64_t lds[kProfileWaves];
  const uint64_t me = tiles[blockIdx.x];
  const uint64_t next = (int32_t)blockIdx.x + 1 < n_tiles ? tiles[blockIdx.x + 1] : (uint64_t)head[PF_ENTRIES];
  if (next == me) return;  // no entry in this tile (uniform over the workgroup)
  const int64_t c0 = (int64_t)blockIdx.x * kProfileTile + (int64_t)threadIdx.x * kProfileItems;
  int32_t k[kProfileItems];
  tile_inpos(p, c0, k);
  unsigned long long m[kProfileItems];
  uint64_t w = 0;
#pragma unroll
  for (int32_t i = 0; i < kProfileItems; ++i) {
    m[i] = k[i] >= 0 ? acc[(int64_t)k[i] - k_lo] : 0;
    w += m[i] >= (unsigned long long)min_msgs;  // (min_msgs >= 1: a channel that is not owned makes no entry)
  }
  uint64_t total;
  int64_t at = (int64_t)(me + cg_block_prefix<kProfileWaves>(w, lds, total));
#pragma unroll
  for (int32_t i = 0; i < kProfileItems; ++i) {
    if (m[i] < (unsigned long long)min_msgs) continue;
    const int64_t j = (int64_t)k[i] - k_lo;
    const unsigned long long pk = acc[2 * ke + j];
    ProfileEntry e;
    e.channel = (int32_t)(c0 + i);
    e.snaps = (int32_t)acc[3 * ke + j];
    e.peak = (int32_t)(pk >> 32);
    e.peak_sid = sid_lo + (int32_t)~(uint32_t)pk;
    e.msgs = (long long)m[i];
    e.tokens = (long long)acc[ke + j];
    ent[at++] = e;
  }
}

inline unsigned blocks_for(int64_t items) { return (unsigned)((items + kProfileThreads - 1) / kProfileThreads); }

// Slices of the used list for a pass of `blocks` workgroups per slice: enough to fill the chip,
// none shorter than kProfileSliceSids rows; `forced` > 0 overrides.  The results do not depend on it.
int32_t slices_for(int64_t blocks, int32_t ns, int32_t n_cus, int32_t forced) {
  int64_t s = forced;
  if (s <= 0) {
    const int64_t want = (int64_t)kProfileBlocksPerCu * (n_cus > 0 ? n_cus : 1);
    s = (want + blocks - 1) / (blocks > 0 ? blocks : 1);
    if (s > ns / kProfileSliceSids) s = ns / kProfileSliceSids;
  }
  return (int32_t)(s < 1 ? 1 : s > 65535 ? 65535 : s);
}

}  // namespace

int32_t cg_profile_tiles(int64_t e) {
  const int64_t t = (e + kProfileTile - 1) / kProfileTile;
  return (int32_t)(t > 0 ? t : 1);
}

int cg_launch_profile_reduce(const GParams& p, int32_t k_lo, int32_t k_hi, int32_t sid_lo, int32_t ns,
                             const int32_t* use, const long long* org_in, int32_t user, int32_t slices, int32_t min_msgs,
                             int32_t bins, int32_t width, const GProfile& s, int32_t n_cus, void* stream) {
  if (ns <= 0) return (int)hipSuccess;
  hipStream_t st = (hipStream_t)stream;
  const int64_t ke = (int64_t)k_hi - k_lo;
  const int32_t n_tiles = cg_profile_tiles(p.e);
  hipError_t e = hipMemsetAsync(s.head, 0, (size_t)(PF_HEAD + bins) * sizeof(long long), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_profile_used, dim3(1), dim3(kProfileThreads), 0, st, p, use, org_in, user, sid_lo, ns, s.list,
                     s.used, s.org, s.head);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if (ke > 0) {
    const unsigned gx = blocks_for(((int64_t)k_hi - (k_lo & ~1) + 1) / 2);
    const int32_t gy = slices_for(gx, ns, n_cus, slices);
    if (gy == 1) {
      hipLaunchKernelGGL(k_profile_chan<false>, dim3(gx, 1), dim3(kProfileThreads), 0, st, p, k_lo, k_hi, sid_lo, s.list,
                         s.head, s.acc);
    } else {
      if ((e = hipMemsetAsync(s.acc, 0, (size_t)ke * 4 * sizeof(unsigned long long), st)) != hipSuccess) return (int)e;
      hipLaunchKernelGGL(k_profile_chan<true>, dim3(gx, (unsigned)gy), dim3(kProfileThreads), 0, st, p, k_lo, k_hi, sid_lo,
                         s.list, s.head, s.acc);
    }
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k_profile_count, dim3((unsigned)n_tiles), dim3(kProfileThreads), 0, st, p, k_lo, ke, s.acc, min_msgs,
                     bins, width, s.head, s.tiles);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_profile_scan, dim3(1), dim3(kProfileThreads), 0, st, n_tiles, s.tiles, s.head);
  return (int)hipGetLastError();
}

int cg_launch_profile_nodes(const GParams& p, int32_t k_lo, int32_t k_hi, int32_t sid_lo, int32_t ns, int32_t slices,
                            const GProfile& s, int32_t n_cus, void* stream) {
  const int64_t width = (int64_t)p.part_hi - p.part_lo;
  if (ns <= 0 || width <= 0) return (int)hipSuccess;
  hipStream_t st = (hipStream_t)stream;
  const unsigned gx = blocks_for(width);
  const int32_t gy = slices_for(gx, ns, n_cus, slices);
  if (gy == 1) {
    hipLaunchKernelGGL(k_profile_node<false>, dim3(gx, 1), dim3(kProfileThreads), 0, st, p, sid_lo, s.list, s.org, s.head,
                       s.rows);
  } else {
    hipLaunchKernelGGL(k_profile_node_init, dim3(blocks_for(width * kNodeWords)), dim3(kProfileThreads), 0, st,
                       width * kNodeWords, s.rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_profile_node<true>, dim3(gx, (unsigned)gy), dim3(kProfileThreads), 0, st, p, sid_lo, s.list, s.org,
                       s.head, s.rows);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_profile_in, dim3(gx), dim3(kProfileThreads), 0, st, p, k_lo, (int64_t)k_hi - k_lo, s.acc, s.rows);
  return (int)hipGetLastError();
}

int cg_launch_profile_fill(const GParams& p, int32_t k_lo, int32_t k_hi, int32_t sid_lo, int32_t min_msgs,
                           const GProfile& s, void* entries, void* stream) {
  const int32_t n_tiles = cg_profile_tiles(p.e);
  hipLaunchKernelGGL(k_profile_fill, dim3((unsigned)n_tiles), dim3(kProfileThreads), 0, (hipStream_t)stream, p, k_lo,
                     (int64_t)k_hi - k_lo, sid_lo, s.acc, min_msgs, n_tiles, s.tiles, s.head,
                     reinterpret_cast<ProfileEntry*>(entries));
  return (int)hipGetLastError();
}

}  // namespace clsnap
