// cg_cut.hip -- the check of a host-supplied cut (cl_graph_restore_cut): before a seed that came
// from caller-held arrays may reach k_seed (cg_restore.hip), which stores to
// fifo[(channel << cap_log2) + q] and hq[channel] and trusts every entry, one pass over the
// uploaded arrays proves them well-formed:
//   rule 1  tokens[v] >= 0
//   rule 2  0 <= channel[i] < e, and channel[i - 1] < channel[i] for i > 0
//   rule 3  1 <= count[i] <= kCutMaxCount (the largest ring)
//   rule 4  msgs[j] >= 0: bit 31 of a queue word's payload marks a marker
// (rule 5, sum(count) == n_msgs, is the host's, from the offsets' total.)
//   k_cut_check   grid-stride over groups of four elements of each array: one aligned 16-byte load
//                 per group (the arrays are device allocations; a ragged last group is loaded
//                 element by element), and for a group of channels the one element in front of it.
//                 Every index is the thread's own position within the array's length; no value
//                 read from the arrays is ever used as one.  A defect is the word
//                 (rule << 56) | index; a thread keeps the least it met, the wave and the workgroup
//                 reduce to their least, and one atomicMin per workgroup that found any leaves the
//                 least of all in *verdict (kCutClean when none): the same word under any grid.
#include <hip/hip_runtime.h>

#include "cg_engine.h"

namespace clsnap {
namespace {

constexpr int32_t kCcThreads = 256;
constexpr int32_t kCcWaves = kCcThreads / 64;

__device__ __forceinline__ uint64_t cut_word(uint32_t rule, int64_t index) {
  return ((uint64_t)rule << 56) | (uint64_t)index;
}

// The four elements at i0 (a multiple of 4) of a[len]; past the end: `pad`.
__device__ __forceinline__ int4 cut_load4(const int32_t* __restrict__ a, int64_t i0, int64_t len, int32_t pad) {
  if (i0 + 4 <= len) return *reinterpret_cast<const int4*>(a + i0);
  int4 v;
  v.x = i0 < len ? a[i0] : pad;
  v.y = i0 + 1 < len ? a[i0 + 1] : pad;
  v.z = i0 + 2 < len ? a[i0 + 2] : pad;
  v.w = i0 + 3 < len ? a[i0 + 3] : pad;
  return v;
}

// The least defect word of a group whose element k is bad iff bad[k]: element order, so the first.
__device__ __forceinline__ uint64_t cut_first(uint64_t best, uint32_t rule, int64_t i0, bool b0, bool b1, bool b2,
                                              bool b3) {
  const int32_t k = b0 ? 0 : b1 ? 1 : b2 ? 2 : b3 ? 3 : -1;
  if (k < 0) return best;
  const uint64_t w = cut_word(rule, i0 + k);
  return w < best ? w : best;
}

__global__ void __launch_bounds__(kCcThreads) k_cut_check(const int32_t* __restrict__ tokens, int64_t n,
                                                          const int32_t* __restrict__ channel,
                                                          const int32_t* __restrict__ count, int64_t n_ent,
                                                          const int32_t* __restrict__ msgs, int64_t n_msgs, int32_t e,
                                                          unsigned long long* __restrict__ verdict) {
  __shared__ uint64_t lds[kCcWaves];
  uint64_t best = kCutClean;
  const int64_t first = ((int64_t)blockIdx.x * kCcThreads + threadIdx.x) * 4;
  const int64_t stride = (int64_t)gridDim.x * kCcThreads * 4;
  for (int64_t i0 = first; i0 < n; i0 += stride) {
    const int4 t = cut_load4(tokens, i0, n, 0);
    best = cut_first(best, kCutRuleTokens, i0, t.x < 0, t.y < 0, t.z < 0, t.w < 0);
  }
  for (int64_t i0 = first; i0 < n_ent; i0 += stride) {
    // past the end: a channel above every real one, never reported (its index is not below n_ent)
    const int4 c = cut_load4(channel, i0, n_ent, INT32_MAX);
    const int32_t before = i0 > 0 ? channel[i0 - 1] : -1;
    const int64_t left = n_ent - i0;
    best = cut_first(best, kCutRuleChannel, i0, (uint32_t)c.x >= (uint32_t)e || before >= c.x,
                     left > 1 && ((uint32_t)c.y >= (uint32_t)e || c.x >= c.y),
                     left > 2 && ((uint32_t)c.z >= (uint32_t)e || c.y >= c.z),
                     left > 3 && ((uint32_t)c.w >= (uint32_t)e || c.z >= c.w));
    const int4 k = cut_load4(count, i0, n_ent, 1);
    const uint32_t top = (uint32_t)kCutMaxCount;  // (1 <= k <= top as one unsigned compare of k - 1)
    best = cut_first(best, kCutRuleCount, i0, (uint32_t)k.x - 1u >= top, (uint32_t)k.y - 1u >= top,
                     (uint32_t)k.z - 1u >= top, (uint32_t)k.w - 1u >= top);
  }
  if (msgs)
    for (int64_t i0 = first; i0 < n_msgs; i0 += stride) {
      const int4 m = cut_load4(msgs, i0, n_msgs, 0);
      best = cut_first(best, kCutRulePayload, i0, m.x < 0, m.y < 0, m.z < 0, m.w < 0);
    }
#pragma unroll
  for (int32_t o = 32; o > 0; o >>= 1) {
    const uint64_t other = __shfl_down(best, o);
    best = other < best ? other : best;
  }
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int32_t w = 1; w < kCcWaves; ++w) best = lds[w] < best ? lds[w] : best;
    if (best != kCutClean) atomicMin(verdict, (unsigned long long)best);
  }
}

}  // namespace

int cg_launch_cut_check(const int32_t* tokens, int64_t n, const int32_t* channel, const int32_t* count, int64_t n_ent,
                        const int32_t* msgs, int64_t n_msgs, int32_t e, unsigned long long* verdict, int32_t n_cus,
                        void* stream) {
  int64_t most = n > n_ent ? n : n_ent;
  if (msgs && n_msgs > most) most = n_msgs;
  const int64_t per_block = (int64_t)kCcThreads * 4;
  int64_t grid = (most + per_block - 1) / per_block;
  const int64_t cap = (int64_t)(n_cus > 0 ? n_cus : 1) * 8;  // (two workgroups per SIMD: the loads of one hide the other's)
  grid = grid < 1 ? 1 : grid > cap ? cap : grid;
  hipLaunchKernelGGL(k_cut_check, dim3((unsigned)grid), dim3(kCcThreads), 0, (hipStream_t)stream, tokens, n, channel,
                     count, n_ent, msgs, n_msgs, e, verdict);
  return (int)hipGetLastError();
}

}  // namespace clsnap
