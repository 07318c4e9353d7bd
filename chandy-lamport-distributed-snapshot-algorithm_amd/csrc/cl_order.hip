// cl_order.hip -- ordering a batch by a snapshot quantity: top-k instances and exact quantiles of
// the batch engine (cl_snapshot_topk, cl_snapshot_quantiles, cl_snapshot_values).
//
// ORDER BY q LIMIT k and the value at given positions of the ascending order, over the sample of
// cl_snapshot_stats (cl_sample.h).  The order is total: ascending by (key, instance), key =
// order_key(value) -- the value with its sign bit flipped, complemented for descending -- so a tie
// always goes to the smaller instance index.  All integer and order-preserving, so the result does
// not depend on the grid, the record layout, the slot map or the exec kernel.
//
// Value walk (cl_order_walk).  The sample walk of cl_sample.h, lane = slot.  Records of at most
// kCensusStageWords words are staged in LDS as one chunk (stage_tile) when the term reads them,
// longer ones are read word by word (RecordRow); the value is quantity_value()'s.  Every instance
// of the range gets its entry of the int64 value plane [hi - lo], indexed by instance - lo: the
// value, or 0 outside the sample.  A lane whose slot is at or past n_inst (a ragged last tile) has
// no instance -- its map entry is poison and is never read -- and the scatter itself is guarded by
// the instance range, not only the record read.  Membership goes into a bitmap in the select
// bitmap's convention (base = lo rounded down to 64): instance-major a tile is one word, the wave's
// ballot; block-major every sample lane ORs its bit into the zeroed bitmap.  The three counters and
// the sample's min and max are reduced per wave, then per workgroup in LDS, then one atomic each.
//
// Radix select (cl_order_hist, cl_order_choose).  MSD digit passes of kOrderDigitBits bits over the
// keys, one launch pair per pass; the host fixes the number of passes from the walk's min and max
// (the bits above the highest differing bit are common to every key) -- up to 8 for the full 64
// bits.  The state is one OrderPos per order position (the top-k's k - 1; up to 64 quantile ranks),
// kept by ascending rank: the prefix its key is known to have, its rank among the candidates with
// that prefix, and the index of that prefix among the positions' distinct prefixes (its group).  The
// histogram kernel counts the current digit of every member whose upper bits match a group's prefix
// (a binary search over the at most 64 ascending prefixes in LDS) in a per-workgroup LDS histogram
// [groups][256] and merges it with one integer atomic per non-empty bin.  The one-workgroup choice
// then scans each position's row for the bucket that holds its rank, extends the prefix, reduces the
// rank, regroups the positions and zeroes the histogram.  No kernel waits on another workgroup; the
// loop bounds are fixed by the digit count.
//
// Top-k compaction (cl_order_mark, launch_select_compact twice, cl_order_gather).  With T the key at
// position k - 1, two bitmaps mark the members with key < T and with key == T; the select's
// compaction lists each in ascending instance order; the result is all of the first list and the
// first k - n_less of the second, with their values gathered from the plane.  The host sorts these at
// most k rows by (key, instance).
#include <hip/hip_runtime.h>

#include "cl_quantity.h"

namespace clsnap {
namespace {

__global__ __launch_bounds__(kOrderThreads) void cl_order_walk(OrderWalkParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char order_lds[];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* scal = reinterpret_cast<unsigned long long*>(order_lds);                // [8]: 3 counters, min, max
  long long* ext = reinterpret_cast<long long*>(scal);
  uint32_t* tile = reinterpret_cast<uint32_t*>(scal + 8) + (size_t)wave * kStatsStageWords;  // [64][N * rw | 1]
  if (threadIdx.x < 3) scal[threadIdx.x] = 0;
  if (threadIdx.x == ORD_MIN) ext[ORD_MIN] = kI64Max;
  if (threadIdx.x == ORD_MAX) ext[ORD_MAX] = kI64Min;
  __syncthreads();

  SampleCounts counts;
  long long mn = kI64Max, mx = kI64Min;
  for (int64_t t = sample_first_tile(p.s, wave); t < p.s.tile_hi; t += sample_tile_stride()) {
    const SampleLane l = sample_lane(p.s, t, lane);
    counts.add(l);
    long long v = 0;
    if (__ballot(l.sample) != 0) {  // (wave-uniform)
      if (p.staged) stage_tile(p.s, t, whole_record_chunk(p.s), tile, lane);
      if (l.sample) {
        const RecordRow rb(p.s, t, lane, tile, p.staged);
        v = quantity_value<SEL_KEY>(p.s, p.tab, p.s.sid, p.term.field, p.term.index, rb, l.tick);
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
      }
    }
    // ---- the plane and the membership bit.  The scatter is guarded by the range itself: a slot at or
    // past n_inst has inst = -1 (its map entry was never read) and forms no address.
    const bool inside = l.inst >= p.s.lo && l.inst < p.s.hi;
    if (inside) p.plane[l.inst - p.s.lo] = l.sample ? v : 0;
    if (!p.s.blocked) {
      const unsigned long long word = __ballot(l.sample && inside);
      if (lane == 0) p.bitmap[t - p.s.tile_lo] = word;
    } else if (l.sample && inside) {
      const int64_t bit = l.inst - p.base;
      atomicOr(&p.bitmap[bit >> 6], 1ULL << (bit & 63));
    }
  }

  for (int o = 32; o > 0; o >>= 1) {
    const long long a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if (lane == 0 && mn <= mx) atomicMin(&ext[ORD_MIN], mn), atomicMax(&ext[ORD_MAX], mx);
  counts.fold_wave(scal, lane);
  __syncthreads();
  unsigned long long* info = reinterpret_cast<unsigned long long*>(p.info);
  sample_counts_to_global(scal, &info[ORD_INSTANCES], &info[ORD_OK], &info[ORD_SAMPLE]);
  if (threadIdx.x == ORD_MIN && ext[ORD_MIN] != kI64Max) atomicMin(&p.info[ORD_MIN], ext[ORD_MIN]);
  if (threadIdx.x == ORD_MAX && ext[ORD_MAX] != kI64Min) atomicMax(&p.info[ORD_MAX], ext[ORD_MAX]);
}

// The bits of `key` above the digit at `shift`.
__device__ __forceinline__ unsigned long long key_prefix(unsigned long long key, int32_t shift) {
  return shift + kOrderDigitBits >= 64 ? 0ULL : key >> (shift + kOrderDigitBits);
}

__device__ __forceinline__ bool plane_member(const OrderSelectParams& p, int64_t i) {
  const int64_t bit = i + p.off;
  return (p.bitmap[bit >> 6] >> (bit & 63)) & 1ULL;
}

__global__ __launch_bounds__(kOrderThreads) void cl_order_hist(OrderSelectParams p, int32_t shift) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hist_lds[];
  unsigned long long* gp = reinterpret_cast<unsigned long long*>(hist_lds);  // [n_pos] the groups' prefixes
  uint32_t* hist = reinterpret_cast<uint32_t*>(gp + p.n_pos);                // [n_pos][kOrderBins]
  // groups are numbered 0 .. G - 1 by ascending prefix; never more than positions
  int32_t G = p.pos[p.n_pos - 1].group + 1;
  G = G < 1 ? 1 : G > p.n_pos ? p.n_pos : G;
  for (int32_t j = threadIdx.x; j < p.n_pos; j += kOrderThreads) {
    const int32_t g = p.pos[j].group;
    if (g >= 0 && g < G) gp[g] = p.pos[j].prefix;  // (positions of one group store the same prefix)
  }
  for (int32_t e = threadIdx.x; e < G * kOrderBins; e += kOrderThreads) hist[e] = 0;
  __syncthreads();

  const int64_t stride = (int64_t)gridDim.x * kOrderThreads;
  for (int64_t i = (int64_t)blockIdx.x * kOrderThreads + threadIdx.x; i < p.n; i += stride) {
    if (!plane_member(p, i)) continue;
    const unsigned long long key = order_key(p.plane[i], p.desc);
    const unsigned long long pre = key_prefix(key, shift);
    int32_t a = 0, b = G;  // the first group whose prefix is >= pre
    while (a < b) {
      const int32_t m = (a + b) >> 1;
      if (gp[m] < pre) a = m + 1;
      else b = m;
    }
    if (a < G && gp[a] == pre) atomicAdd(&hist[a * kOrderBins + (int32_t)((key >> shift) & (kOrderBins - 1))], 1u);
  }
  __syncthreads();
  for (int32_t e = threadIdx.x; e < G * kOrderBins; e += kOrderThreads)
    if (hist[e]) atomicAdd(&p.hist[e], hist[e]);
}

// One workgroup.  Position j: the bucket of its group's row that holds its rank; the prefix takes the
// bucket's digit, the rank loses the buckets before it.  Then the positions are regrouped by their
// new prefixes and the rows that were used are zeroed for the next pass.
__global__ __launch_bounds__(kOrderThreads) void cl_order_choose(OrderSelectParams p) {
  __shared__ unsigned long long s_prefix[kOrderMaxPos];
  __shared__ int32_t s_groups;
  const int32_t j = threadIdx.x;
  if (j == 0) {
    const int32_t G = p.pos[p.n_pos - 1].group + 1;
    s_groups = G < 1 ? 1 : G > p.n_pos ? p.n_pos : G;
  }
  if (j < p.n_pos) {
    OrderPos z = p.pos[j];
    const int32_t g = z.group < 0 ? 0 : z.group >= p.n_pos ? p.n_pos - 1 : z.group;
    const uint32_t* row = p.hist + (size_t)g * kOrderBins;
    long long before = 0;
    int32_t b = 0;
    for (; b < kOrderBins; ++b) {
      const long long c = row[b];
      if (z.rank < before + c) break;
      before += c;
    }
    if (b == kOrderBins || z.rank < 0) {  // (the histogram does not hold the rank: reported, not followed)
      z.bad = 1;
      b = kOrderBins - 1;
      before = z.rank;
    }
    z.prefix = (z.prefix << kOrderDigitBits) | (unsigned long long)b;
    z.rank -= before;
    s_prefix[j] = z.prefix;
    p.pos[j].prefix = z.prefix;
    p.pos[j].rank = z.rank;
    p.pos[j].bad = z.bad;
  }
  __syncthreads();  // (every row has been read)
  if (j == 0) {
    int32_t g = 0;
    p.pos[0].group = 0;
    for (int32_t q = 1; q < p.n_pos; ++q) {
      g += s_prefix[q] != s_prefix[q - 1];
      p.pos[q].group = g;
    }
  }
  for (int32_t e = threadIdx.x; e < s_groups * kOrderBins; e += kOrderThreads) p.hist[e] = 0;
}

// One wave per bitmap word, lane = bit.
__global__ __launch_bounds__(kOrderThreads) void cl_order_mark(OrderSelectParams p, int64_t words,
                                                               unsigned long long* less, unsigned long long* equal) {
  const int32_t lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * (kOrderThreads / 64) + (threadIdx.x >> 6);
  if (w >= words) return;  // (wave-uniform)
  const unsigned long long T = p.pos[0].prefix;
  const int64_t i = w * 64 + lane - p.off;
  bool lt = false, eq = false;
  if (i >= 0 && i < p.n && ((p.bitmap[w] >> lane) & 1ULL)) {
    const unsigned long long key = order_key(p.plane[i], p.desc);
    lt = key < T;
    eq = key == T;
  }
  const unsigned long long wl = __ballot(lt), we = __ballot(eq);
  if (lane == 0) less[w] = wl, equal[w] = we;
}

__global__ __launch_bounds__(kOrderThreads) void cl_order_gather(OrderSelectParams p, int64_t lo, int64_t k,
                                                                 const long long* list_a,
                                                                 const unsigned long long* info_a,
                                                                 const long long* list_b,
                                                                 const unsigned long long* info_b, long long* out_inst,
                                                                 long long* out_val) {
  const int64_t j = (int64_t)blockIdx.x * kOrderThreads + threadIdx.x;
  if (j >= k) return;
  // (the lists hold at most k entries each: the compaction's cap)
  const int64_t n_a = (int64_t)info_a[3] < k ? (int64_t)info_a[3] : k;
  const int64_t n_b = (int64_t)info_b[3] < k ? (int64_t)info_b[3] : k;
  long long inst = -1, v = 0;
  if (j < n_a) inst = list_a[j];
  else if (j - n_a < n_b) inst = list_b[j - n_a];
  if (inst >= lo && inst - lo < p.n) v = p.plane[inst - lo];
  else inst = -1;
  out_inst[j] = inst;
  out_val[j] = v;
}

bool select_ok(const OrderSelectParams& p) {
  return p.n >= 1 && p.off >= 0 && p.off < 64 && p.n_pos >= 1 && p.n_pos <= kOrderMaxPos && p.plane && p.bitmap &&
         p.pos && p.hist;
}

}  // namespace

int launch_order_walk(const OrderWalkParams& p, int32_t blocks, void* stream) {
  const SampleParams& s = p.s;
  if (blocks < 1 || !quantity_ok(p.term.field, p.term.index, SEL_KEY, s.n_nodes, s.n_ch) || p.term.sid != s.sid ||
      s.sid < 0 || s.sid >= s.s_cap || !staged_ok(s, p.staged) || !p.plane || !p.bitmap || !p.info)
    return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)order_walk_lds_bytes(p.staged != 0);
  hipLaunchKernelGGL(cl_order_walk, dim3((unsigned)blocks), dim3(kOrderThreads), lds, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

int launch_order_pass(const OrderSelectParams& p, int32_t shift, int32_t blocks, void* stream) {
  if (!select_ok(p) || blocks < 1 || shift < 0 || shift > 64 - kOrderDigitBits || shift % kOrderDigitBits)
    return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)order_hist_lds_bytes(p.n_pos);
  if (lds > (size_t)kMaxLdsBytes) return (int)hipErrorInvalidValue;
  if (lds > 64 * 1024) {
    const hipError_t e =
        hipFuncSetAttribute((const void*)cl_order_hist, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(cl_order_hist, dim3((unsigned)blocks), dim3(kOrderThreads), lds, (hipStream_t)stream, p, shift);
  hipLaunchKernelGGL(cl_order_choose, dim3(1), dim3(kOrderThreads), 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

int launch_order_mark(const OrderSelectParams& p, int64_t words, unsigned long long* less, unsigned long long* equal,
                      void* stream) {
  const int64_t blocks = (words + kOrderThreads / 64 - 1) / (kOrderThreads / 64);
  // the words cover the plane: no element beyond the last word, no word beyond the last element
  if (!select_ok(p) || words != (p.n + p.off + 63) / 64 || blocks > 0x7fffffffLL || !less || !equal)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(cl_order_mark, dim3((unsigned)blocks), dim3(kOrderThreads), 0, (hipStream_t)stream, p, words, less,
                     equal);
  return (int)hipGetLastError();
}

int launch_order_gather(const OrderSelectParams& p, int64_t lo, int64_t k, const long long* list_a,
                        const unsigned long long* info_a, const long long* list_b, const unsigned long long* info_b,
                        long long* out_inst, long long* out_val, void* stream) {
  if (k < 1) return 0;
  if (!select_ok(p) || k > kOrderMaxK || !list_a || !info_a || !list_b || !info_b || !out_inst || !out_val)
    return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((k + kOrderThreads - 1) / kOrderThreads);
  hipLaunchKernelGGL(cl_order_gather, dim3(blocks), dim3(kOrderThreads), 0, (hipStream_t)stream, p, lo, k, list_a,
                     info_a, list_b, info_b, out_inst, out_val);
  return (int)hipGetLastError();
}

}  // namespace clsnap
