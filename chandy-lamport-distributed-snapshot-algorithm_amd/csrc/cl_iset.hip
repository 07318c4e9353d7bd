// cl_iset.hip -- device-resident instance sets of the batch engine (cl_iset, include/clsnap.h).
//
// A set is a bitmap over the batch: bit inst & 63 of word inst >> 6, stride / 64 words, the bits
// at and above n_instances always 0.  cl_select_eval writes one from clauses (cl_select.hip); the
// kernels here build one from an index list, combine two word by word, and count or clip the words
// of an index range.  The analytics kernels read a set through SampleParams::where (cl_sample.h);
// the listing of a set is the selection's compaction (launch_select_compact) over the clipped words.
//
//   scatter   one atomicOr per listed instance into a zeroed bitmap (duplicates set the same bit).
//   combine   dst[w] = a[w] AND / OR / AND NOT b[w]: a thread reads both words before it stores its
//             own, so dst may be a or b; operands without bits past n_instances give none.
//   clip      the words that overlap [lo, hi), the first and the last masked to the range.
//   count     the set bits of those words: popcount per word, wave and workgroup totals, one
//             global atomic per workgroup.
// All plain loads, stores and integer atomics; grids are sized to the words, capped, grid-stride.
#include <hip/hip_runtime.h>

#include "cl_analytics.h"

namespace clsnap {
namespace {

constexpr int64_t kIsetMaxBlocks = 2048;

// The bits of word w (instances [64 w, 64 w + 64)) that lie in [lo, hi); w overlaps the range.
__device__ __forceinline__ unsigned long long range_mask(int64_t w, int64_t lo, int64_t hi) {
  unsigned long long m = ~0ULL;
  const int64_t first = w * 64;
  if (lo > first) m &= ~0ULL << (lo - first);                // 0 < lo - first < 64
  if (hi < first + 64) m &= (1ULL << (hi - first)) - 1ULL;   // 0 < hi - first < 64
  return m;
}

__global__ __launch_bounds__(kIsetThreads) void cl_iset_scatter(const long long* list, int64_t n, int64_t n_inst,
                                                                unsigned long long* bits) {
  const int64_t stride = (int64_t)gridDim.x * kIsetThreads;
  for (int64_t r = (int64_t)blockIdx.x * kIsetThreads + threadIdx.x; r < n; r += stride) {
    const long long i = list[r];
    if (i >= 0 && i < n_inst) atomicOr(&bits[i >> 6], 1ULL << (i & 63));
  }
}

__global__ __launch_bounds__(kIsetThreads) void cl_iset_combine(unsigned long long* dst, const unsigned long long* a,
                                                                const unsigned long long* b, int32_t op,
                                                                int64_t words) {
  const int64_t stride = (int64_t)gridDim.x * kIsetThreads;
  for (int64_t w = (int64_t)blockIdx.x * kIsetThreads + threadIdx.x; w < words; w += stride) {
    const unsigned long long x = a[w], y = b[w];
    dst[w] = op == ISET_AND ? x & y : op == ISET_OR ? x | y : x & ~y;
  }
}

__global__ __launch_bounds__(kIsetThreads) void cl_iset_clip(unsigned long long* dst, const unsigned long long* src,
                                                             int64_t lo, int64_t hi) {
  const int64_t w0 = lo >> 6, words = ((hi + 63) >> 6) - w0;
  const int64_t stride = (int64_t)gridDim.x * kIsetThreads;
  for (int64_t j = (int64_t)blockIdx.x * kIsetThreads + threadIdx.x; j < words; j += stride)
    dst[j] = src[w0 + j] & range_mask(w0 + j, lo, hi);
}

__global__ __launch_bounds__(kIsetThreads) void cl_iset_count(const unsigned long long* src, int64_t lo, int64_t hi,
                                                              unsigned long long* count) {
  __shared__ unsigned long long wtot[kIsetThreads / 64];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w0 = lo >> 6, words = ((hi + 63) >> 6) - w0;
  const int64_t stride = (int64_t)gridDim.x * kIsetThreads;
  unsigned long long c = 0;
  for (int64_t j = (int64_t)blockIdx.x * kIsetThreads + threadIdx.x; j < words; j += stride)
    c += (unsigned long long)__popcll(src[w0 + j] & range_mask(w0 + j, lo, hi));
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) wtot[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int32_t k = 0; k < kIsetThreads / 64; ++k) s += wtot[k];
    if (s) atomicAdd(count, s);
  }
}

unsigned grid_for(int64_t n) {
  const int64_t b = (n + kIsetThreads - 1) / kIsetThreads;
  return (unsigned)(b < 1 ? 1 : b > kIsetMaxBlocks ? kIsetMaxBlocks : b);
}

}  // namespace

int launch_iset_scatter(const long long* list, int64_t n, int64_t n_inst, unsigned long long* bits, void* stream) {
  if (n < 1) return 0;
  if (!list || !bits || n_inst < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(cl_iset_scatter, dim3(grid_for(n)), dim3(kIsetThreads), 0, (hipStream_t)stream, list, n, n_inst,
                     bits);
  return (int)hipGetLastError();
}

int launch_iset_combine(unsigned long long* dst, const unsigned long long* a, const unsigned long long* b,
                        int32_t op, int64_t words, void* stream) {
  if (!dst || !a || !b || op < 0 || op >= ISET_NUM_OPS || words < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(cl_iset_combine, dim3(grid_for(words)), dim3(kIsetThreads), 0, (hipStream_t)stream, dst, a, b, op,
                     words);
  return (int)hipGetLastError();
}

int launch_iset_clip(unsigned long long* dst, const unsigned long long* src, int64_t lo, int64_t hi, void* stream) {
  if (!dst || !src || lo < 0 || hi <= lo) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(cl_iset_clip, dim3(grid_for(((hi + 63) >> 6) - (lo >> 6))), dim3(kIsetThreads), 0,
                     (hipStream_t)stream, dst, src, lo, hi);
  return (int)hipGetLastError();
}

int launch_iset_count(const unsigned long long* src, int64_t lo, int64_t hi, unsigned long long* count, void* stream) {
  if (!src || !count || lo < 0 || hi <= lo) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(cl_iset_count, dim3(grid_for(((hi + 63) >> 6) - (lo >> 6))), dim3(kIsetThreads), 0,
                     (hipStream_t)stream, src, lo, hi, count);
  return (int)hipGetLastError();
}

}  // namespace clsnap
