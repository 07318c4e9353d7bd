// cl_census.hip -- snapshot outcome census of the batch engine (cl_snapshot_census).
//
// Which distinct global snapshots did a batch produce, how often, and which instance is an example
// of each: a group-by of the 64-bit snapshot content hash (cl_checksum_kernel's per-snapshot term,
// orc_snapshot_hash) over the sample (cl_sample.h) -- the instances of [lo, hi) with status
// OK in which snapshot `sid` completed.  Per class: count, smallest instance, min and max
// completion tick.  All integer; sums, minima and maxima commute, so the table's contents do not
// depend on the grid, the workgroup tables, the record layout or the exec kernel, and the host's
// sort (count descending, key ascending) fixes the order.
//
// Key pass (cl_census_keys).  The sample walk of cl_sample.h, lane = slot.  Records of at most
// kCensusStageWords words per instance are staged in LDS as one chunk (stage_tile) and each sample
// lane hashes its row; longer records are read word by word by their lane (RecordRow).  The hash
// consumes the N token words, then the channels in channel order, so it cannot be split over
// staging chunks the way the statistics are.
//
// Aggregation.  One class usually holds most of the sample, so one global atomic per instance
// would put the whole grid on one cache line.  Each workgroup first aggregates in an
// open-addressing LDS table (64-bit CAS on the key, then LDS add / min / max); a lane whose probe
// sequence finds no room inserts into the global table directly.  At the end every occupied LDS
// entry issues one global insert.  The global table has >= 2 * (hi - lo) slots and cannot fill;
// the thread that claims a slot appends it to the class list.  The key value kCensusEmptyKey marks
// an empty slot; a snapshot with that very key goes to the extra entry behind the hashed slots.
//
// class_of (on request).  The key pass keeps each sample instance's key; after the host's sort the
// ranks are written into the table entries and a lookup kernel maps key -> rank per instance.
#include <hip/hip_runtime.h>

#include "cl_engine.h"
#include "cl_sample.h"

namespace clsnap {
namespace {

__global__ __launch_bounds__(kCensusThreads) void cl_census_init(CensusEntry* table, int64_t entries,
                                                                 unsigned long long empty_key) {
  // one entry = two 16-byte stores
  uint4 a, b;
  a.x = (uint32_t)empty_key, a.y = (uint32_t)(empty_key >> 32), a.z = 0, a.w = 0;
  b.x = 0xffffffffu, b.y = 0x7fffffffu, b.z = (uint32_t)kI32Max, b.w = (uint32_t)kI32Min;
  uint4* t = reinterpret_cast<uint4*>(table);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < entries; i += stride) {
    t[2 * i] = a;
    t[2 * i + 1] = b;
  }
}

// The table slot of `key`: its entry, claimed if new (then appended to the class list).
__device__ __forceinline__ int64_t census_slot(const CensusParams& p, unsigned long long key, bool claim) {
  if (key == p.empty_key) return p.slots;
  const unsigned long long mask = (unsigned long long)p.slots - 1;
  unsigned long long s = (key >> 16) & mask;
  for (int64_t probe = 0; probe < p.slots; ++probe, s = (s + 1) & mask) {
    if (claim) {
      const unsigned long long old = atomicCAS(&p.table[s].key, p.empty_key, key);
      if (old == p.empty_key) p.list[atomicAdd(&p.info[3], 1ULL)] = (uint32_t)s;
      if (old == p.empty_key || old == key) return (int64_t)s;
    } else {
      const unsigned long long k = p.table[s].key;
      if (k == key) return (int64_t)s;
      if (k == p.empty_key) return -1;
    }
  }
  return -1;  // (unreachable: the table has twice as many slots as the range has instances)
}

__device__ __forceinline__ void census_global_insert(const CensusParams& p, unsigned long long key,
                                                     unsigned long long count, long long first, int32_t mn,
                                                     int32_t mx) {
  const int64_t s = census_slot(p, key, true);
  if (s < 0) return;
  CensusEntry* e = p.table + s;
  const unsigned long long before = atomicAdd(&e->count, count);
  // the extra entry has no key to claim: its first adder lists it
  if (s == p.slots && before == 0) p.list[atomicAdd(&p.info[3], 1ULL)] = (uint32_t)s;
  atomicMin(&e->first, first);
  atomicMin(&e->min_tick, mn);
  atomicMax(&e->max_tick, mx);
}

__global__ __launch_bounds__(kCensusThreads) void cl_census_keys(CensusParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char census_lds[];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t S = p.lds_slots;
  unsigned long long* lkey = reinterpret_cast<unsigned long long*>(census_lds);  // [S]
  long long* lfirst = reinterpret_cast<long long*>(lkey + S);                    // [S]
  unsigned long long* scal = reinterpret_cast<unsigned long long*>(lfirst + S);  // [4] (3 used)
  uint32_t* lcnt = reinterpret_cast<uint32_t*>(scal + 4);                        // [S]
  int32_t* lmn = reinterpret_cast<int32_t*>(lcnt + S);                           // [S]
  int32_t* lmx = lmn + S;                                                        // [S]
  uint32_t* tile = reinterpret_cast<uint32_t*>(lmx + S) + (size_t)wave * kStatsStageWords;  // [64][N * rw | 1]

  for (int32_t i = threadIdx.x; i < S; i += kCensusThreads) {
    lkey[i] = p.empty_key;
    lfirst[i] = kI64Max;
    lcnt[i] = 0;
    lmn[i] = kI32Max;
    lmx[i] = kI32Min;
  }
  if (threadIdx.x < 4) scal[threadIdx.x] = 0;
  __syncthreads();

  SampleCounts counts;
  for (int64_t t = sample_first_tile(p.s, wave); t < p.s.tile_hi; t += sample_tile_stride()) {
    const SampleLane l = sample_lane(p.s, t, lane);
    const int64_t inst = l.inst;
    const int32_t tick = l.tick;
    counts.add(l);
    if (l.in && p.keys && !l.sample) p.class_of[inst - p.s.lo] = -1;
    if (__ballot(l.sample) == 0) continue;  // (wave-uniform)
    if (p.staged) stage_tile(p.s, t, whole_record_chunk(p.s), tile, lane);
    if (!l.sample) continue;

    // ---- the key: cl_checksum_kernel's arithmetic for one snapshot id
    const unsigned long long key = snapshot_key(p.s.sid, p.s.n_nodes, p.s.rw, p.s.n_ch, p.ch_slot, p.hist_off,
                                                p.hist_val, RecordRow(p.s, t, lane, tile, p.staged));
    if (p.keys) {
      p.keys[inst - p.s.lo] = key;
      p.class_of[inst - p.s.lo] = 0;
    }

    // ---- the workgroup's table, else the global one
    bool placed = false;
    if (S > 0 && key != p.empty_key) {
      uint32_t s = (uint32_t)key & (uint32_t)(S - 1);
      const int32_t probes = S < kCensusLdsProbes ? S : kCensusLdsProbes;
      for (int32_t probe = 0; probe < probes && !placed; ++probe, s = (s + 1) & (uint32_t)(S - 1)) {
        const unsigned long long old = atomicCAS(&lkey[s], p.empty_key, key);
        if (old == p.empty_key || old == key) {
          atomicAdd(&lcnt[s], 1u);
          atomicMin(&lfirst[s], (long long)inst);
          atomicMin(&lmn[s], tick);
          atomicMax(&lmx[s], tick);
          placed = true;
        }
      }
    }
    if (!placed) census_global_insert(p, key, 1, inst, tick, tick);
  }

  counts.fold_wave(scal, lane);
  __syncthreads();
  sample_counts_to_global(scal, &p.info[0], &p.info[1], &p.info[2]);
  // ---- one global insert per occupied entry of the workgroup's table
  for (int32_t i = threadIdx.x; i < S; i += kCensusThreads)
    if (lcnt[i]) census_global_insert(p, lkey[i], lcnt[i], lfirst[i], lmn[i], lmx[i]);
}

__global__ __launch_bounds__(kCensusThreads) void cl_census_gather(CensusParams p, int64_t n, CensusEntry* out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint4* e = reinterpret_cast<const uint4*>(p.table + p.list[j]);
  uint4* o = reinterpret_cast<uint4*>(out + j);
  o[0] = e[0];
  o[1] = e[1];
}

__global__ __launch_bounds__(kCensusThreads) void cl_census_rank(CensusParams p, int64_t n, const int32_t* rank) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) p.table[p.list[j]].count = (unsigned long long)(uint32_t)rank[j];
}

__global__ __launch_bounds__(kCensusThreads) void cl_census_lookup(CensusParams p) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.s.hi - p.s.lo || p.class_of[i] < 0) return;
  const int64_t s = census_slot(p, p.keys[i], false);
  p.class_of[i] = s < 0 ? -1 : (int32_t)p.table[s].count;
}

unsigned grid_for(int64_t n) { return (unsigned)((n + kCensusThreads - 1) / kCensusThreads); }

}  // namespace

int launch_census_init(const CensusParams& p, void* stream) {
  const int64_t entries = p.slots + 1;
  const unsigned blocks = (unsigned)(entries / kCensusThreads < 4096 ? grid_for(entries) : 4096);
  hipLaunchKernelGGL(cl_census_init, dim3(blocks), dim3(kCensusThreads), 0, (hipStream_t)stream, p.table, entries,
                     p.empty_key);
  return (int)hipGetLastError();
}

int launch_census_keys(const CensusParams& p, int32_t blocks, void* stream) {
  const size_t lds = (size_t)census_lds_bytes(p.lds_slots, p.staged != 0);
  if (lds > (size_t)kMaxLdsBytes || blocks < 1) return (int)hipErrorInvalidValue;
  if (p.staged && p.s.n_nodes * p.s.rw > kCensusStageWords) return (int)hipErrorInvalidValue;
  if (lds > 64 * 1024) {
    const hipError_t e =
        hipFuncSetAttribute((const void*)cl_census_keys, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(cl_census_keys, dim3((unsigned)blocks), dim3(kCensusThreads), lds, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

int launch_census_gather(const CensusParams& p, int64_t n, CensusEntry* out, void* stream) {
  if (n < 1) return 0;
  hipLaunchKernelGGL(cl_census_gather, dim3(grid_for(n)), dim3(kCensusThreads), 0, (hipStream_t)stream, p, n, out);
  return (int)hipGetLastError();
}

int launch_census_class_of(const CensusParams& p, int64_t n, const int32_t* rank, void* stream) {
  if (n > 0)
    hipLaunchKernelGGL(cl_census_rank, dim3(grid_for(n)), dim3(kCensusThreads), 0, (hipStream_t)stream, p, n, rank);
  if (p.s.hi > p.s.lo)
    hipLaunchKernelGGL(cl_census_lookup, dim3(grid_for(p.s.hi - p.s.lo)), dim3(kCensusThreads), 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

}  // namespace clsnap
