// cl_stats.hip -- per-snapshot batch statistics of the batch engine (cl_snapshot_stats).
//
// One pass over the result planes of a run: the status word of `regs`, the completion tick of
// snapshot `sid` in `snap_tick`, and snapshot sid's slice of the node records `snap_nod`.  For the
// sample (cl_sample.h: the instances of [lo, hi) with status OK in which the snapshot completed)
// the kernel reduces count / sum / sum of squares / min / max / histograms of the completion
// tick, of every node's tokenMap entry, of every channel's recorded messages and tokens, and of
// the per-instance totals, into one flat int64 array (StatsLayout).  All integer, so the result
// does not depend on the grid, the record layout or the exec kernel that wrote the records.
//
// Read pattern.  The sample walk of cl_sample.h: per tile of 64 record slots and chunk of record
// words (cl_analytics.h stats_chunk) the wave stages 64 x K words in LDS (stage_tile), rows at an odd
// pitch, so both views below read the tile without bank conflicts.
//
// Reduction.  Two views of the staged tile:
//   lane = slot      the instance's totals (recorded messages, recorded tokens) over the chunk's
//                    channel words; tick, msgs and inflight then accumulate in the lane's
//                    registers over all its tiles and are wave-reduced once at the end;
//   lane = word      each lane owns one record word of the chunk (a node's token word, or a
//                    channel's cursor word) and runs over the tile's sample instances (a scalar
//                    loop over the ballot mask): sum, sum of squares, min, max in registers, the
//                    message-count histogram in LDS; one LDS atomic per statistic and tile folds
//                    them into the workgroup's accumulators.
// A channel's recorded tokens are two loads of the host-built int64 prefix of its token history.
// At the end each workgroup issues one global integer atomic per accumulator that is not at its
// identity.  No per-lane global atomics, no floating point.
//
// LDS: kStatsLdsBytes per workgroup (cl_analytics.h).  When the N * rw record words of the topology
// need more accumulator rows than fit, the host runs several passes, each accumulating a range
// of chunks; the first also takes the per-instance totals (it reads every chunk).
#include <hip/hip_runtime.h>

#include "cl_sample.h"

namespace clsnap {
namespace {

struct Stat4 {
  unsigned long long sum, sq;
  long long mn, mx;
  __device__ __forceinline__ void init() { sum = 0, sq = 0, mn = kI64Max, mx = kI64Min; }
  __device__ __forceinline__ void add(long long v) {
    sum += (unsigned long long)v;
    sq += (unsigned long long)v * (unsigned long long)v;  // modulo 2^64
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
  }
  // values known to fit 32 bits: the square is one 32 x 32 -> 64 multiply-add
  __device__ __forceinline__ void add_i32(int32_t v) {
    sum += (unsigned long long)(long long)v;
    sq += (unsigned long long)((long long)v * (long long)v);
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
  }
  __device__ __forceinline__ void add_u32(uint32_t v) {
    sum += v;
    sq += (unsigned long long)v * (unsigned long long)v;
    mn = (long long)v < mn ? (long long)v : mn;
    mx = (long long)v > mx ? (long long)v : mx;
  }
  __device__ __forceinline__ void wave_reduce() {
    for (int o = 32; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o);
      sq += __shfl_xor(sq, o);
      const long long a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
      mn = a < mn ? a : mn;
      mx = b > mx ? b : mx;
    }
  }
};

// Accumulator rows in LDS: [8][acc_words] int64 -- sum, sumsq, min, max of the word's first
// statistic (tokenMap entry / recorded messages), then of its second (recorded tokens).
__device__ __forceinline__ void fold(long long* acc, int32_t aw, int32_t row, int32_t k, const Stat4& s) {
  long long* a = acc + (size_t)(4 * k) * aw + row;
  if (s.sum) atomicAdd((unsigned long long*)a, s.sum);
  if (s.sq) atomicAdd((unsigned long long*)(a + aw), s.sq);
  atomicMin(a + 2 * (size_t)aw, s.mn);
  atomicMax(a + 3 * (size_t)aw, s.mx);
}

__global__ __launch_bounds__(kStatsThreads) void cl_stats_kernel(StatsParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char stats_lds[];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t AW = p.acc_words, M = (int32_t)p.lay.msg_bins, T = (int32_t)p.lay.tick_bins;
  long long* acc = reinterpret_cast<long long*>(stats_lds);            // [8][AW]
  long long* scal = acc + 8 * (size_t)AW;                              // [kStatsScalars]
  uint32_t* mh = reinterpret_cast<uint32_t*>(scal + kStatsScalars);    // [AW][M]
  uint32_t* th = mh + (size_t)AW * M;                                  // [T]
  uint32_t* tile = th + T + (size_t)wave * kStatsStageWords;           // [64][K | 1]

  for (int32_t i = threadIdx.x; i < 8 * AW; i += kStatsThreads) {
    const int32_t k = (i / AW) & 3;
    acc[i] = k == 2 ? kI64Max : k == 3 ? kI64Min : 0;
  }
  for (int32_t i = threadIdx.x; i < kStatsScalars; i += kStatsThreads)
    scal[i] = (i == 5 || i == 9 || i == 13) ? kI64Max : (i == 6 || i == 10 || i == 14) ? kI64Min : 0;
  for (int32_t i = threadIdx.x; i < AW * M + T; i += kStatsThreads) mh[i] = 0;  // (mh and th are adjacent)
  __syncthreads();

  const int32_t N = p.s.n_nodes, rw = p.s.rw;
  const int32_t n_chunks = stats_chunks(N, rw);
  const int32_t word_lo = [&] {
    const StatsChunk c = stats_chunk(N, rw, p.chunk_lo);
    return c.v0 * rw + c.k0;
  }();

  SampleCounts counts;
  Stat4 s_tick, s_msgs, s_infl;
  s_tick.init(), s_msgs.init(), s_infl.init();

  for (int64_t t = sample_first_tile(p.s, wave); t < p.s.tile_hi; t += sample_tile_stride()) {
    const SampleLane l = sample_lane(p.s, t, lane);
    const bool sample = l.sample;
    const unsigned long long mask = __ballot(sample);
    if (p.totals) {
      counts.add(l);
      if (sample) {
        s_tick.add(l.tick);
        long long bin = (long long)l.tick - p.lay.tick_lo;
        bin = bin < 0 ? 0 : bin > T - 1 ? T - 1 : bin;
        atomicAdd(&th[bin], 1u);
      }
    }
    if (mask == 0) continue;  // (wave-uniform: no records of this tile are in the sample)

    unsigned long long tot_msgs = 0, tot_tok = 0;
    // a pass without the totals reads its own chunks only
    const int32_t c_begin = p.totals ? 0 : p.chunk_lo, c_end = p.totals ? n_chunks : p.chunk_hi;
    for (int32_t ci = c_begin; ci < c_end; ++ci) {
      const StatsChunk ch = stats_chunk(N, rw, ci);
      const int32_t K = ch.nv * ch.kw, pitch = K | 1, w0 = ch.v0 * rw + ch.k0;
      stage_tile(p.s, t, ch, tile, lane);  // 64 rows x K words, in memory order

      // ---- lane = slot: the instance's totals over this chunk's channel words
      if (p.totals && sample) {
        for (int32_t k = 0; k < K; ++k) {
          const int32_t c = p.word_ch[w0 + k];
          if (c < 0) continue;
          const uint32_t rec = tile[lane * pitch + k], cnt = rec_msgs(rec);
          tot_msgs += cnt;
          if (cnt) tot_tok += (unsigned long long)rec_tokens(rec, token_prefix(p.tab, c));
        }
      }

      // ---- lane = word: every word of the chunk over the tile's sample instances
      if (ci >= p.chunk_lo && ci < p.chunk_hi) {
        for (int32_t k0 = 0; k0 < K; k0 += 64) {
          const int32_t k = k0 + lane;
          const int32_t c = k < K ? p.word_ch[w0 + k] : -1;
          if (c == -1) continue;
          const int32_t row = w0 + k - word_lo;
          Stat4 a, b2;
          a.init(), b2.init();
          if (c == -2) {
            for (unsigned long long m = mask; m; m &= m - 1) {
              const int32_t i = __builtin_ctzll(m);
              a.add_i32((int32_t)tile[i * pitch + k]);
            }
            fold(acc, AW, row, 0, a);
          } else {
            const long long* pre = token_prefix(p.tab, c);
            uint32_t* h = mh + (size_t)row * M;
            for (unsigned long long m = mask; m; m &= m - 1) {
              const int32_t i = __builtin_ctzll(m);
              const uint32_t rec = tile[i * pitch + k], cnt = rec_msgs(rec);
              a.add_u32(cnt);
              // (the full 64 bits, as the lane = slot side keeps for the instance's total)
              b2.add(rec_tokens(rec, pre));
              atomicAdd(&h[cnt < (uint32_t)(M - 1) ? cnt : (uint32_t)(M - 1)], 1u);
            }
            fold(acc, AW, row, 0, a);
            fold(acc, AW, row, 1, b2);
          }
        }
      }
    }
    if (p.totals && sample) {
      s_msgs.add((long long)tot_msgs);
      s_infl.add((long long)tot_tok);
    }
  }

  if (p.totals) {
    unsigned long long* u = (unsigned long long*)scal;
    counts.fold_wave(u, lane);
    s_tick.wave_reduce(), s_msgs.wave_reduce(), s_infl.wave_reduce();
    if (lane == 0) {
      const Stat4* s3[3] = {&s_tick, &s_msgs, &s_infl};
      for (int q = 0; q < 3; ++q) {
        if (s3[q]->sum) atomicAdd(&u[3 + 4 * q], s3[q]->sum);
        if (s3[q]->sq) atomicAdd(&u[4 + 4 * q], s3[q]->sq);
        atomicMin(&scal[5 + 4 * q], s3[q]->mn);
        atomicMax(&scal[6 + 4 * q], s3[q]->mx);
      }
    }
  }
  __syncthreads();

  // ---- one global atomic per accumulator of the workgroup that left its identity
  const StatsLayout& L = p.lay;
  auto g_add = [&](int64_t at, unsigned long long v) {
    if (v) atomicAdd((unsigned long long*)(p.out + at), v);
  };
  auto g_min = [&](int64_t at, long long v) {
    if (v != kI64Max) atomicMin(p.out + at, v);
  };
  auto g_max = [&](int64_t at, long long v) {
    if (v != kI64Min) atomicMax(p.out + at, v);
  };
  if (p.totals) {
    unsigned long long* o = (unsigned long long*)p.out;
    sample_counts_to_global((const unsigned long long*)scal, o + L.instances, o + L.ok, o + L.sample);
    if (threadIdx.x == 0) {
      const int64_t sum_at[3] = {L.tick_sum, L.msgs_sum, L.inflight_sum};
      const int64_t sq_at[3] = {L.tick_sumsq, L.msgs_sumsq, L.inflight_sumsq};
      for (int q = 0; q < 3; ++q) {
        g_add(sum_at[q], (unsigned long long)scal[3 + 4 * q]);
        g_add(sq_at[q], (unsigned long long)scal[4 + 4 * q]);
        g_min(L.min_tick + q, scal[5 + 4 * q]);
        g_max(L.max_tick + q, scal[6 + 4 * q]);
      }
    }
    for (int32_t i = threadIdx.x; i < T; i += kStatsThreads) g_add(L.tick_hist + i, th[i]);
  }
  const int32_t n_words = [&] {
    if (p.chunk_hi <= p.chunk_lo) return 0;
    const StatsChunk c = stats_chunk(N, rw, p.chunk_hi - 1);
    return c.v0 * rw + c.k0 + c.nv * c.kw - word_lo;
  }();
  for (int32_t row = threadIdx.x; row < n_words; row += kStatsThreads) {
    const int32_t w = word_lo + row, c = p.word_ch[w];
    if (c == -1) continue;
    const long long* a = acc + row;
    if (c == -2) {
      const int32_t v = w / rw;
      g_add(L.node_sum + v, (unsigned long long)a[0]);
      g_add(L.node_sumsq + v, (unsigned long long)a[(size_t)AW]);
      g_min(L.min_node + v, a[2 * (size_t)AW]);
      g_max(L.max_node + v, a[3 * (size_t)AW]);
    } else {
      g_add(L.ch_msgs_sum + c, (unsigned long long)a[0]);
      g_add(L.ch_msgs_sumsq + c, (unsigned long long)a[(size_t)AW]);
      g_min(L.min_ch_msgs + c, a[2 * (size_t)AW]);
      g_max(L.max_ch_msgs + c, a[3 * (size_t)AW]);
      g_add(L.ch_tok_sum + c, (unsigned long long)a[4 * (size_t)AW]);
      g_add(L.ch_tok_sumsq + c, (unsigned long long)a[5 * (size_t)AW]);
      g_min(L.min_ch_tok + c, a[6 * (size_t)AW]);
      g_max(L.max_ch_tok + c, a[7 * (size_t)AW]);
    }
  }
  // the message-count histograms: rows of channel words only
  for (int32_t i = threadIdx.x; i < n_words * M; i += kStatsThreads) {
    const uint32_t v = mh[i];
    if (!v) continue;
    const int32_t row = i / M, c = p.word_ch[word_lo + row];
    if (c >= 0) g_add(L.ch_msg_hist + (int64_t)c * M + (i - row * M), v);
  }
}

}  // namespace

int launch_stats(const StatsParams& p, int32_t blocks, void* stream) {
  const size_t lds = (size_t)stats_lds_bytes(p.acc_words, (int32_t)p.lay.tick_bins, (int32_t)p.lay.msg_bins);
  if (lds > (size_t)kStatsLdsBytes || blocks < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(cl_stats_kernel, dim3((unsigned)blocks), dim3(kStatsThreads), lds, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

}  // namespace clsnap
