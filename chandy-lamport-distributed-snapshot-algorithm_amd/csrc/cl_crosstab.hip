// cl_crosstab.hip -- joint distribution of two snapshot quantities of the batch engine
// (cl_snapshot_crosstab).
//
// A two-axis contingency table with the five joint moments.  An axis names a quantity of a snapshot
// (cl_quantity.h; any field but the key, which is not binnable); the two axes may belong to
// different snapshot ids.  The sample is the instances of [lo, hi) with status OK in which the
// snapshots of both axes completed -- of the members of an instance set when one is given.  All
// integer, so the result does not depend on the grid, the record layout or the exec kernel.
//
// One walk (cl_sample.h), lane = slot.  The two axes see the same walk through two views of it
// (cl_quantity.h sample_view): sample_lane() classifies the slot for axis a's snapshot, the lane
// then reads the completion tick of axis b's (view_tick).
//
// One staging tile per wave.  An axis that reads records gets its plane's tile staged in LDS when
// the records have at most kCensusStageWords words (stage_tile), else its lane reads word by word
// (RecordRow): plane a is staged, the lane computes its value into a register, then plane b is
// staged into the same tile -- not again when both axes read the same snapshot, and never for a
// completion-tick axis.  A lane computes only what its axis names.
//
// Reduction.  The cell of a sample lane is one 32-bit LDS atomic on the workgroup's table (at most
// kXtMaxCells counters, 16 KB); the moments, minima and maxima accumulate in the lane's registers
// over all its tiles, are wave-reduced once, and fold into LDS scalars.  At the end the workgroup
// issues one global 64-bit atomic per cell that is not zero and per scalar that left its identity.
// A 32-bit LDS counter cannot wrap: a workgroup counts an instance at most once and the launcher
// refuses walks of 2^32 slots or more, so no counter is flushed before the end.
#include <hip/hip_runtime.h>

#include "cl_quantity.h"

namespace clsnap {
namespace {

__device__ __forceinline__ bool axis_reads_records(const CrosstabAxis& z) { return z.field != SEL_TICK; }

// bin(v) = v < lo ? 0 : min((uint64)(v - lo) / width, bins - 1); the subtraction only when v >= lo,
// so it is exact for every int64 lo.  (width is uniform over the grid: width 1 skips the 64-bit divide)
__device__ __forceinline__ uint32_t axis_bin(const CrosstabAxis& z, long long v) {
  if (v < z.lo) return 0;
  unsigned long long d = (unsigned long long)v - (unsigned long long)z.lo;
  if (z.width != 1) d /= (unsigned long long)z.width;
  const unsigned long long last = (unsigned long long)(z.bins - 1);
  return (uint32_t)(d < last ? d : last);
}

__global__ __launch_bounds__(kXtThreads) void cl_crosstab_kernel(CrosstabParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char crosstab_lds[];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t n_cells = p.a.bins * p.b.bins;
  // scal: [0 .. 3) the counters, [3 .. 8) the sums, [8 .. 10) minima, [10 .. 12) maxima -- the
  // words of the result before the cells
  long long* scal = reinterpret_cast<long long*>(crosstab_lds);  // [16] (12 used)
  uint32_t* cells = reinterpret_cast<uint32_t*>(scal + 16);      // [n_cells]
  uint32_t* tile = cells + n_cells + (size_t)wave * kStatsStageWords;  // [64][N * rw | 1], when staged
  for (int32_t i = threadIdx.x; i < 16; i += kXtThreads)
    scal[i] = (i == XT_MIN_A || i == XT_MIN_B) ? kI64Max : (i == XT_MAX_A || i == XT_MAX_B) ? kI64Min : 0;
  for (int32_t i = threadIdx.x; i < n_cells; i += kXtThreads) cells[i] = 0;
  __syncthreads();

  const SampleParams sb = sample_view(p.s, p.b.sid);  // axis b's snapshot: the same walk, another plane
  const bool same_sid = p.a.sid == p.b.sid;
  const bool rec_a = axis_reads_records(p.a), rec_b = axis_reads_records(p.b);

  SampleCounts counts;
  unsigned long long sum_a = 0, sum_b = 0, sum_aa = 0, sum_ab = 0, sum_bb = 0;
  long long mn_a = kI64Max, mn_b = kI64Max, mx_a = kI64Min, mx_b = kI64Min;

  for (int64_t t = sample_first_tile(p.s, wave); t < p.s.tile_hi; t += sample_tile_stride()) {
    SampleLane l = sample_lane(p.s, t, lane);
    int32_t tick_b = -1;
    if (l.sample) tick_b = view_tick(p.s, l, p.b.sid);
    l.sample = l.sample && tick_b >= 0;  // both snapshots completed
    counts.add(l);
    if (__ballot(l.sample) == 0) continue;  // (wave-uniform)

    long long va = l.tick, vb = tick_b;
    if (rec_a) {
      if (p.staged) stage_tile(p.s, t, whole_record_chunk(p.s), tile, lane);
      if (l.sample)
        va = quantity_value<SEL_CH_TOK>(p.s, p.tab, p.a.sid, p.a.field, p.a.index,
                                        RecordRow(p.s, t, lane, tile, p.staged), l.tick);
    }
    if (rec_b) {
      // (the tile still holds this plane when axis a staged the same snapshot)
      if (p.staged && !(rec_a && same_sid)) stage_tile(sb, t, whole_record_chunk(sb), tile, lane);
      if (l.sample)
        vb = quantity_value<SEL_CH_TOK>(sb, p.tab, p.b.sid, p.b.field, p.b.index,
                                        RecordRow(sb, t, lane, tile, p.staged), tick_b);
    }

    if (l.sample) {
      sum_a += (unsigned long long)va, sum_b += (unsigned long long)vb;
      sum_aa += (unsigned long long)va * (unsigned long long)va;  // modulo 2^64
      sum_ab += (unsigned long long)va * (unsigned long long)vb;
      sum_bb += (unsigned long long)vb * (unsigned long long)vb;
      mn_a = va < mn_a ? va : mn_a, mx_a = va > mx_a ? va : mx_a;
      mn_b = vb < mn_b ? vb : mn_b, mx_b = vb > mx_b ? vb : mx_b;
      // (plain LDS atomics: counting the equal cells of a wave first measured slower)
      atomicAdd(&cells[axis_bin(p.a, va) * (uint32_t)p.b.bins + axis_bin(p.b, vb)], 1u);
    }
  }

  unsigned long long* u = reinterpret_cast<unsigned long long*>(scal);
  counts.fold_wave(u, lane);
  for (int o = 32; o > 0; o >>= 1) {
    sum_a += __shfl_xor(sum_a, o), sum_b += __shfl_xor(sum_b, o);
    sum_aa += __shfl_xor(sum_aa, o), sum_ab += __shfl_xor(sum_ab, o), sum_bb += __shfl_xor(sum_bb, o);
    const long long a0 = __shfl_xor(mn_a, o), a1 = __shfl_xor(mx_a, o);
    const long long b0 = __shfl_xor(mn_b, o), b1 = __shfl_xor(mx_b, o);
    mn_a = a0 < mn_a ? a0 : mn_a, mx_a = a1 > mx_a ? a1 : mx_a;
    mn_b = b0 < mn_b ? b0 : mn_b, mx_b = b1 > mx_b ? b1 : mx_b;
  }
  if (lane == 0) {
    if (sum_a) atomicAdd(&u[XT_SUM_A], sum_a);
    if (sum_b) atomicAdd(&u[XT_SUM_B], sum_b);
    if (sum_aa) atomicAdd(&u[XT_SUM_AA], sum_aa);
    if (sum_ab) atomicAdd(&u[XT_SUM_AB], sum_ab);
    if (sum_bb) atomicAdd(&u[XT_SUM_BB], sum_bb);
    atomicMin(&scal[XT_MIN_A], mn_a), atomicMin(&scal[XT_MIN_B], mn_b);
    atomicMax(&scal[XT_MAX_A], mx_a), atomicMax(&scal[XT_MAX_B], mx_b);
  }
  __syncthreads();

  // ---- one global atomic per scalar that left its identity and per cell that is not zero
  unsigned long long* o = reinterpret_cast<unsigned long long*>(p.out);
  sample_counts_to_global(u, o + XT_INSTANCES, o + XT_OK, o + XT_SAMPLE);
  if (threadIdx.x >= XT_SUM_A && threadIdx.x < XT_MIN_A) {
    if (u[threadIdx.x]) atomicAdd(o + threadIdx.x, u[threadIdx.x]);
  } else if (threadIdx.x >= XT_MIN_A && threadIdx.x < XT_MAX_A) {
    if (scal[threadIdx.x] != kI64Max) atomicMin(p.out + threadIdx.x, scal[threadIdx.x]);
  } else if (threadIdx.x >= XT_MAX_A && threadIdx.x < XT_CELLS) {
    if (scal[threadIdx.x] != kI64Min) atomicMax(p.out + threadIdx.x, scal[threadIdx.x]);
  }
  for (int32_t i = threadIdx.x; i < n_cells; i += kXtThreads) {
    const uint32_t v = cells[i];
    if (v) atomicAdd(o + XT_CELLS + i, (unsigned long long)v);
  }
}

}  // namespace

int launch_crosstab(const CrosstabParams& p, int32_t blocks, void* stream) {
  const int64_t cells = (int64_t)p.a.bins * (int64_t)p.b.bins;
  if (blocks < 1 || p.a.bins < 1 || p.b.bins < 1 || p.a.bins > kXtMaxBins || p.b.bins > kXtMaxBins ||
      cells > kXtMaxCells || p.a.width < 1 || p.b.width < 1 || p.s.sid != p.a.sid)
    return (int)hipErrorInvalidValue;
  const auto axis_ok = [&p](const CrosstabAxis& z) {  // (a key is not binnable: the fields end at SEL_CH_TOK)
    return quantity_ok(z.field, z.index, SEL_CH_TOK, p.s.n_nodes, p.s.n_ch) && z.sid >= 0 && z.sid < p.s.s_cap;
  };
  if (!axis_ok(p.a) || !axis_ok(p.b) || !staged_ok(p.s, p.staged)) return (int)hipErrorInvalidValue;
  const bool staged = p.staged != 0 && (p.a.field != SEL_TICK || p.b.field != SEL_TICK);
  // the bound that keeps a workgroup's 32-bit cell counters from wrapping
  if (p.s.tile_hi - p.s.tile_lo >= ((int64_t)1 << 32) / 64) return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)crosstab_lds_bytes((int32_t)cells, staged);
  hipLaunchKernelGGL(cl_crosstab_kernel, dim3((unsigned)blocks), dim3(kXtThreads), lds, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

}  // namespace clsnap
