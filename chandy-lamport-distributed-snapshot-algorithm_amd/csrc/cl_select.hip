// cl_select.hip -- instance selection by snapshot predicate of the batch engine (cl_select_instances).
//
// Which instances of a batch have a snapshot with given properties: a conjunction of at most
// kSelMaxClauses range clauses over quantities of one snapshot (cl_quantity.h: completion tick, a
// node's tokenMap entry, a channel's recorded messages and tokens, the instance's totals, the
// census key), evaluated over the sample of cl_snapshot_stats (cl_sample.h) -- the instances of [lo, hi)
// with status OK in which snapshot `sid` completed.  The answer is the ascending list of matching instance
// indices.  All integer and order-preserving, so it does not depend on the grid, the record layout
// or the exec kernel.
//
// Evaluate (cl_select_eval).  The sample walk of cl_sample.h, lane = slot.  When a clause reads the
// records, those of at most kCensusStageWords words per instance are staged in LDS as one chunk
// (stage_tile); longer ones are read word by word by their lane (RecordRow).  A sample lane computes only what the
// clauses name, each clause with quantity_value(): the totals once, in one pass over the channels'
// cursor words, and the key once, however many clauses name them (QuantityOnce).  The
// verdict goes into a bitmap indexed by instance - base, base = lo rounded down to a multiple of 64:
//   instance-major records: a tile is 64 consecutive instances, i.e. one bitmap word -- the wave's
//     ballot, one store (every word of the bitmap is written, none needs zeroing);
//   block-major records: the slots of a wave scatter over instances -- each matching lane ORs its
//     bit into the bitmap, which the host zeroed.
//
// Compact (cl_select_count, cl_select_scan, cl_select_fill).  An order-preserving stream compaction
// of the bitmap: a workgroup takes kSelBlockWords words, one per thread; popcount per word and the
// workgroup's total (count); an exclusive scan of the totals by one workgroup, which leaves the
// number of matches in info[3] (scan); then each workgroup scans its popcounts again and every
// wave writes the set bits of its 64 words, word by word with lane = bit, to out[] at the word's
// offset -- consecutive lanes, consecutive entries -- and gathers their completion ticks (fill).
// Entries from `cap` on are dropped.
#include <hip/hip_runtime.h>

#include "cl_quantity.h"

namespace clsnap {
namespace {

__global__ __launch_bounds__(kSelThreads) void cl_select_eval(SelectParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char select_lds[];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* scal = reinterpret_cast<unsigned long long*>(select_lds);               // [4] (3 used)
  uint32_t* tile = reinterpret_cast<uint32_t*>(scal + 4) + (size_t)wave * kStatsStageWords;  // [64][N * rw | 1]
  if (threadIdx.x < 4) scal[threadIdx.x] = 0;
  __syncthreads();

  SampleCounts counts;
  for (int64_t t = sample_first_tile(p.s, wave); t < p.s.tile_hi; t += sample_tile_stride()) {
    const SampleLane l = sample_lane(p.s, t, lane);
    counts.add(l);
    bool hit = false;
    if (__ballot(l.sample) != 0) {  // (wave-uniform)
      if (p.need_records && p.staged) stage_tile(p.s, t, whole_record_chunk(p.s), tile, lane);
      if (l.sample) {
        const RecordRow rb(p.s, t, lane, tile, p.staged);
        // what several clauses may name, once: both totals in one pass over the cursor words, the key
        QuantityOnce once{};
        if (p.need_totals) once.totals = channel_totals(p.s, p.tab, rb);
        if (p.need_key) once.key = record_key(p.s, p.tab, p.s.sid, rb);
        hit = true;
        for (int32_t q = 0; q < p.n_clauses; ++q) {
          const SelectClause& z = p.clause[q];
          const long long v = quantity_value<SEL_KEY>(p.s, p.tab, p.s.sid, z.field, z.index, rb, l.tick, &once);
          // (a key is compared as the unsigned value it is)
          const bool inside = z.field == SEL_KEY ? (unsigned long long)v >= (unsigned long long)z.lo &&
                                                       (unsigned long long)v <= (unsigned long long)z.hi
                                                 : v >= z.lo && v <= z.hi;
          hit = hit && inside != ((z.flags & kSelNot) != 0);
        }
      }
    }
    // ---- the verdict
    if (!p.s.blocked) {
      const unsigned long long word = __ballot(hit);
      if (lane == 0) p.bitmap[t - p.s.tile_lo] = word;
    } else if (hit) {
      const int64_t bit = l.inst - p.base;
      atomicOr(&p.bitmap[bit >> 6], 1ULL << (bit & 63));
    }
  }

  counts.fold_wave(scal, lane);
  __syncthreads();
  sample_counts_to_global(scal, &p.info[0], &p.info[1], &p.info[2]);
}

// Inclusive scan of x over the wave's lanes.
template <class T>
__device__ __forceinline__ T wave_scan(T x, int32_t lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  return x;
}

__global__ __launch_bounds__(kSelThreads) void cl_select_count(SelectParams p) {
  __shared__ uint32_t wtot[kSelThreads / 64];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * kSelBlockWords + threadIdx.x;
  uint32_t c = w < p.words ? (uint32_t)__popcll(p.bitmap[w]) : 0;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) wtot[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long s = 0;
    for (int32_t k = 0; k < kSelThreads / 64; ++k) s += wtot[k];
    p.bsum[blockIdx.x] = s;
  }
}

// One workgroup: bsum[0 .. n_blocks) -> its exclusive prefix; the total to info[3].
__global__ __launch_bounds__(kSelThreads) void cl_select_scan(SelectParams p, int64_t n_blocks) {
  __shared__ long long wtot[kSelThreads / 64];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long carry = 0;
  for (int64_t i0 = 0; i0 < n_blocks; i0 += kSelThreads) {
    const int64_t i = i0 + threadIdx.x;
    const long long v = i < n_blocks ? p.bsum[i] : 0;
    const long long x = wave_scan(v, lane);
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    long long before = 0, total = 0;
    for (int32_t k = 0; k < kSelThreads / 64; ++k) {
      if (k < wave) before += wtot[k];
      total += wtot[k];
    }
    if (i < n_blocks) p.bsum[i] = carry + before + x - v;
    carry += total;
    __syncthreads();  // (wtot is rewritten by the next round)
  }
  if (threadIdx.x == 0) p.info[3] = (unsigned long long)carry;
}

__global__ __launch_bounds__(kSelThreads) void cl_select_fill(SelectParams p) {
  __shared__ uint32_t wtot[kSelThreads / 64];
  const long long block_off = p.bsum[blockIdx.x];
  if (block_off >= p.cap) return;  // (the same for the whole workgroup: every later entry is dropped)
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * kSelBlockWords + threadIdx.x;
  const unsigned long long word = w < p.words ? p.bitmap[w] : 0;
  const uint32_t c = (uint32_t)__popcll(word);
  const uint32_t x = wave_scan(c, lane);
  if (lane == 63) wtot[wave] = x;
  __syncthreads();
  uint32_t before = 0;
  for (int32_t k = 0; k < wave; ++k) before += wtot[k];
  const long long off = block_off + before + (x - c);  // where this word's first match goes
  // the wave's 64 words, one at a time with lane = bit
  for (int32_t k = 0; k < 64; ++k) {
    const unsigned long long wk = __shfl(word, k);
    if (wk == 0) continue;  // (wave-uniform)
    const long long ok = __shfl(off, k);
    if (ok >= p.cap) break;  // (wave-uniform; the words after it start later still)
    if ((wk >> lane) & 1ULL) {
      const long long pos = ok + __popcll(wk & ((1ULL << lane) - 1));
      if (pos < p.cap) {
        const int64_t inst = p.base + (w - lane + k) * 64 + lane;
        p.out[pos] = inst;
        if (p.ticks) p.ticks[pos] = p.s.snap_tick[inst * p.s.s_cap + p.s.sid];
      }
    }
  }
}

}  // namespace

int launch_select_eval(const SelectParams& p, int32_t blocks, void* stream) {
  const size_t lds = (size_t)select_lds_bytes(p.staged != 0 && p.need_records != 0);
  if (blocks < 1 || p.n_clauses < 0 || p.n_clauses > kSelMaxClauses) return (int)hipErrorInvalidValue;
  if (!staged_ok(p.s, p.staged)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(cl_select_eval, dim3((unsigned)blocks), dim3(kSelThreads), lds, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

int launch_select_compact(const SelectParams& p, void* stream) {
  const int64_t n_blocks = (p.words + kSelBlockWords - 1) / kSelBlockWords;
  if (n_blocks < 1 || n_blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(cl_select_count, dim3((unsigned)n_blocks), dim3(kSelThreads), 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(cl_select_scan, dim3(1), dim3(kSelThreads), 0, (hipStream_t)stream, p, n_blocks);
  if (p.cap > 0)
    hipLaunchKernelGGL(cl_select_fill, dim3((unsigned)n_blocks), dim3(kSelThreads), 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

}  // namespace clsnap
