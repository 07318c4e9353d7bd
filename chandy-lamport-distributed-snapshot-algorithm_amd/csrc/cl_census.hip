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
// Aggregation (cl_census_table.h, shared with the key pass of cl_groups.hip).  Each workgroup first
// aggregates in an open-addressing LDS table; a lane whose probe sequence finds no room inserts
// into the global table directly, and at the end every occupied LDS entry issues one global
// insert.  The key value kCensusEmptyKey marks an empty slot; a snapshot with that very key goes to
// the extra entry behind the hashed slots.
//
// class_of (on request).  The key pass keeps each sample instance's key; after the host's sort the
// ranks are written into the table entries and a lookup kernel maps key -> rank per instance.
#include <hip/hip_runtime.h>

#include "cl_census_table.h"
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

__global__ __launch_bounds__(kCensusThreads) void cl_census_keys(CensusParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char census_lds_mem[];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const CensusLds L = census_lds(census_lds_mem, p.lds_slots, wave);
  census_lds_init(L, p.lds_slots, p.empty_key);

  SampleCounts counts;
  for (int64_t t = sample_first_tile(p.s, wave); t < p.s.tile_hi; t += sample_tile_stride()) {
    const SampleLane l = sample_lane(p.s, t, lane);
    const int64_t inst = l.inst;
    counts.add(l);
    if (l.in && p.keys && !l.sample) p.class_of[inst - p.s.lo] = -1;
    if (__ballot(l.sample) == 0) continue;  // (wave-uniform)
    if (p.staged) stage_tile(p.s, t, whole_record_chunk(p.s), L.tile, lane);
    if (!l.sample) continue;

    // ---- the key: cl_checksum_kernel's arithmetic for one snapshot id
    const unsigned long long key = record_key(p.s, p.tab, p.s.sid, RecordRow(p.s, t, lane, L.tile, p.staged));
    if (p.keys) {
      p.keys[inst - p.s.lo] = key;
      p.class_of[inst - p.s.lo] = 0;
    }
    // ---- the workgroup's table, else the global one
    census_insert(p, L, key, inst, l.tick);
  }
  // ---- the counters, then one global insert per occupied entry of the workgroup's table
  census_lds_flush(p, L, counts, lane);
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
  if (lds > (size_t)kMaxLdsBytes || blocks < 1 || !staged_ok(p.s, p.staged)) return (int)hipErrorInvalidValue;
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
