// cl_census_table.h -- the group-by table shared by the key passes of the census (cl_census.hip)
// and of the tuple group-by (cl_groups.hip).  Device code, like cl_sample.h.
//
// Aggregation.  One group usually holds most of the sample, so one global atomic per instance
// would put the whole grid on one cache line.  Each workgroup first aggregates in an
// open-addressing LDS table (64-bit CAS on the key, then LDS add / min / max); a lane whose probe
// sequence finds no room inserts into the global table directly.  At the end every occupied LDS
// entry issues one global insert.  The global table has >= 2 * (hi - lo) slots and cannot fill;
// the thread that claims a slot appends it to the class list.  The key value
// CensusParams::empty_key marks an empty slot; a group with that very key goes to the extra entry
// behind the hashed slots.
#pragma once
#include <hip/hip_runtime.h>

#include "cl_sample.h"

namespace clsnap {

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

// A key pass's dynamic LDS (census_lds_bytes): the workgroup's table of S = p.lds_slots entries,
// the scalars of the call's counters, and one staging tile per wave when the records are staged.
struct CensusLds {
  unsigned long long* key;   // [S]
  long long* first;          // [S]
  unsigned long long* scal;  // [4] (3 used)
  uint32_t* cnt;             // [S]
  int32_t *mn, *mx;          // [S]
  uint32_t* tile;            // this wave's [64][N * rw | 1]
};
__device__ __forceinline__ CensusLds census_lds(unsigned char* lds, int32_t S, int32_t wave) {
  CensusLds L;
  L.key = reinterpret_cast<unsigned long long*>(lds);
  L.first = reinterpret_cast<long long*>(L.key + S);
  L.scal = reinterpret_cast<unsigned long long*>(L.first + S);
  L.cnt = reinterpret_cast<uint32_t*>(L.scal + 4);
  L.mn = reinterpret_cast<int32_t*>(L.cnt + S);
  L.mx = L.mn + S;
  L.tile = reinterpret_cast<uint32_t*>(L.mx + S) + (size_t)wave * kStatsStageWords;
  return L;
}

// Empties the workgroup's table and zeroes the scalars (a barrier closes it).
__device__ __forceinline__ void census_lds_init(const CensusLds& L, int32_t S, unsigned long long empty_key) {
  for (int32_t i = threadIdx.x; i < S; i += kCensusThreads) {
    L.key[i] = empty_key;
    L.first[i] = kI64Max;
    L.cnt[i] = 0;
    L.mn[i] = kI32Max;
    L.mx[i] = kI32Min;
  }
  if (threadIdx.x < 4) L.scal[threadIdx.x] = 0;
  __syncthreads();
}

// One sample instance into the workgroup's table, else the global one.
__device__ __forceinline__ void census_insert(const CensusParams& p, const CensusLds& L, unsigned long long key,
                                              int64_t inst, int32_t tick) {
  const int32_t S = p.lds_slots;
  bool placed = false;
  if (S > 0 && key != p.empty_key) {
    uint32_t s = (uint32_t)key & (uint32_t)(S - 1);
    const int32_t probes = S < kCensusLdsProbes ? S : kCensusLdsProbes;
    for (int32_t probe = 0; probe < probes && !placed; ++probe, s = (s + 1) & (uint32_t)(S - 1)) {
      const unsigned long long old = atomicCAS(&L.key[s], p.empty_key, key);
      if (old == p.empty_key || old == key) {
        atomicAdd(&L.cnt[s], 1u);
        atomicMin(&L.first[s], (long long)inst);
        atomicMin(&L.mn[s], tick);
        atomicMax(&L.mx[s], tick);
        placed = true;
      }
    }
  }
  if (!placed) census_global_insert(p, key, 1, inst, tick, tick);
}

// The close of a key pass: the wave's counters into the call's info, then one global insert per
// occupied entry of the workgroup's table.
__device__ __forceinline__ void census_lds_flush(const CensusParams& p, const CensusLds& L, SampleCounts& counts,
                                                 int32_t lane) {
  counts.fold_wave(L.scal, lane);
  __syncthreads();
  sample_counts_to_global(L.scal, &p.info[0], &p.info[1], &p.info[2]);
  for (int32_t i = threadIdx.x; i < p.lds_slots; i += kCensusThreads)
    if (L.cnt[i]) census_global_insert(p, L.key[i], L.cnt[i], L.first[i], L.mn[i], L.mx[i]);
}

}  // namespace clsnap
