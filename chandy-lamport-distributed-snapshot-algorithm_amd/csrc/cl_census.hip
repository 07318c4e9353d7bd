// cl_census.hip -- snapshot outcome census of the batch engine (cl_snapshot_census).
//
// Which distinct global snapshots did a batch produce, how often, and which instance is an example
// of each: a group-by of the 64-bit snapshot content hash (cl_checksum_kernel's per-snapshot term,
// orc_snapshot_hash) over the sample of cl_snapshot_stats -- the instances of [lo, hi) with status
// OK in which snapshot `sid` completed.  Per class: count, smallest instance, min and max
// completion tick.  All integer; sums, minima and maxima commute, so the table's contents do not
// depend on the grid, the workgroup tables, the record layout or the exec kernel, and the host's
// sort (count descending, key ascending) fixes the order.
//
// Key pass (cl_census_keys).  A wave walks tiles of 64 record slots, grid-stride, like the
// statistics kernel; lane = slot.  Records of at most kCensusStageWords words per instance are
// staged in LDS with address-ordered loads (in both layouts the tile's 64 * N * rw words are
// contiguous), rows at an odd pitch, and each sample lane hashes its row; longer records are read
// word by word by their lane.  The hash consumes the N token words, then the channels in channel
// order, so it cannot be split over staging chunks the way the statistics are.
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

namespace clsnap {
namespace {

constexpr long long kI64Max = 0x7fffffffffffffffLL;
constexpr int32_t kI32Max = 0x7fffffff, kI32Min = -kI32Max - 1;

__device__ __forceinline__ void census_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

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
  uint32_t* tile = reinterpret_cast<uint32_t*>(lmx + S) + (size_t)wave * kStatsStageWords;  // [64][NW | 1]

  for (int32_t i = threadIdx.x; i < S; i += kCensusThreads) {
    lkey[i] = p.empty_key;
    lfirst[i] = kI64Max;
    lcnt[i] = 0;
    lmn[i] = kI32Max;
    lmx[i] = kI32Min;
  }
  if (threadIdx.x < 4) scal[threadIdx.x] = 0;
  __syncthreads();

  const int32_t N = p.n_nodes, rw = p.rw, NW = N * rw, pitch = NW | 1;
  const size_t plane = (size_t)p.sid * (size_t)p.stride * (size_t)NW;
  const bool vec = (rw & 3) == 0;
  unsigned long long n_all = 0, n_ok = 0, n_sample = 0;

  const int64_t wave_stride = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t t = p.tile_lo + (int64_t)blockIdx.x * kWavesPerBlock + wave; t < p.tile_hi; t += wave_stride) {
    const int64_t slot = t * 64 + lane;
    int64_t inst = -1;
    if (slot < p.n_inst) inst = p.blocked && p.inst_map ? (int64_t)p.inst_map[slot] : slot;
    const bool in = inst >= p.lo && inst < p.hi;
    bool ok = false, sample = false;
    int32_t tick = -1;
    if (in) {
      ok = p.regs[inst * R_NUM + R_STATUS] == ST_OK;
      tick = p.snap_tick[inst * p.s_cap + p.sid];
      sample = ok && tick >= 0;
    }
    n_all += in, n_ok += ok, n_sample += sample;
    if (in && p.keys && !sample) p.class_of[inst - p.lo] = -1;
    if (__ballot(sample) == 0) continue;  // (wave-uniform)

    // the tile's 64 * NW record words, contiguous in both layouts
    const uint32_t* src = p.snap_nod + plane + (size_t)t * 64 * (size_t)NW;
    if (p.staged) {
      census_wave_sync();  // (the previous tile's readers are done)
      if (vec) {
        const int32_t rq = rw >> 2;
        for (int32_t f = lane; f < 16 * NW; f += 64) {
          const uint4 x = reinterpret_cast<const uint4*>(src)[f];
          // instance-major: word 4 f of row r = 4 f / NW; block-major [N][64][rw]: record
          // g = f / rq of node v = g / 64, row r = g % 64
          int32_t r, k;
          if (p.blocked) {
            const int32_t g = f / rq, q = f - g * rq, v = g >> 6;
            r = g & 63, k = v * rw + 4 * q;
          } else {
            r = (4 * f) / NW, k = 4 * f - r * NW;
          }
          uint32_t* d = tile + r * pitch + k;
          d[0] = x.x, d[1] = x.y, d[2] = x.z, d[3] = x.w;
        }
      } else {
        for (int32_t f = lane; f < 64 * NW; f += 64) {
          int32_t r, k;
          if (p.blocked) {
            const int32_t g = f / rw, w = f - g * rw, v = g >> 6;
            r = g & 63, k = v * rw + w;
          } else {
            r = f / NW, k = f - r * NW;
          }
          tile[r * pitch + k] = src[f];
        }
      }
      census_wave_sync();
    }
    if (!sample) continue;

    // ---- the key: cl_checksum_kernel's arithmetic for one snapshot id
    auto rb = [&](int32_t idx) -> uint32_t {
      if (p.staged) return tile[lane * pitch + idx];
      if (!p.blocked) return src[(size_t)lane * NW + idx];
      const int32_t v = idx / rw;
      return src[((size_t)v * 64 + lane) * rw + (idx - v * rw)];
    };
    const unsigned long long key = snapshot_key(p.sid, N, rw, p.n_ch, p.ch_slot, p.hist_off, p.hist_val, rb);
    if (p.keys) {
      p.keys[inst - p.lo] = key;
      p.class_of[inst - p.lo] = 0;
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

  for (int o = 32; o > 0; o >>= 1) {
    n_all += __shfl_xor(n_all, o);
    n_ok += __shfl_xor(n_ok, o);
    n_sample += __shfl_xor(n_sample, o);
  }
  if (lane == 0) {
    if (n_all) atomicAdd(&scal[0], n_all);
    if (n_ok) atomicAdd(&scal[1], n_ok);
    if (n_sample) atomicAdd(&scal[2], n_sample);
  }
  __syncthreads();
  if (threadIdx.x < 3 && scal[threadIdx.x]) atomicAdd(&p.info[threadIdx.x], scal[threadIdx.x]);
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
  if (i >= p.hi - p.lo || p.class_of[i] < 0) return;
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
  if (p.staged && p.n_nodes * p.rw > kCensusStageWords) return (int)hipErrorInvalidValue;
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
  if (p.hi > p.lo)
    hipLaunchKernelGGL(cl_census_lookup, dim3(grid_for(p.hi - p.lo)), dim3(kCensusThreads), 0, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

}  // namespace clsnap
