// cl_sample.h -- the sample walk shared by the analytics kernels of the batch engine
// (cl_stats.hip, cl_census.hip, cl_select.hip, cl_crosstab.hip, cl_groups.hip).  Device code; the
// declarations it works on are cl_analytics.h's.
//
// The sample (SampleParams).  Every instance of [lo, hi) with status OK in which snapshot `sid`
// completed (completion tick >= 0) -- of the members of an instance set when one is given
// (SampleParams::where, the cl_*_in calls).
//
// The walk.  A wave walks tiles of 64 record slots, grid-stride (sample_first_tile,
// sample_tile_stride), the grid sized to the chip; lane = slot.  sample_lane() classifies the
// lane's slot: with block-major records the slot's instance comes from the replay's slot ->
// instance map and a sub-range filters on it; instance-major, slot = instance.  SampleCounts keeps
// the instances / OK / sample counters of the call's info.
//
// Staging (stage_tile).  A tile of records is staged in LDS chunk by chunk (cl_analytics.h
// stats_chunk; records of at most kCensusStageWords words are one chunk, whole_record_chunk):
//   block-major records [S][I/64][N][64][rw]: the tile is one 64-slot block, a chunk of whole
//     nodes is nv * 64 * rw contiguous words;
//   instance-major records [S][I][N][rw]: the tile's 64 instances are 64 * N * rw contiguous
//     words; a chunk takes K contiguous words of each (all of them when N * rw <= 32, e.g. the
//     8-node degree-3 topology's 128 B).
// Both are read lane-linear in address order, dwordx4 when rw % 4 == 0 (every chunk then starts
// and ends on 16 bytes).  Rows are padded to an odd pitch K | 1, so a lane reading its own row and
// a lane reading one word of every row both go without bank conflicts.  RecordRow reads a word of
// the lane's record from the staged tile, or from the plane when the records are not staged;
// PlaneRow reads a word of any instance's record from the plane.
#pragma once
#include <hip/hip_runtime.h>

#include "cl_analytics.h"

namespace clsnap {

constexpr long long kI64Max = 0x7fffffffffffffffLL, kI64Min = -kI64Max - 1;
constexpr int32_t kI32Max = 0x7fffffff, kI32Min = -kI32Max - 1;

// Orders the wave's LDS writes before its later LDS reads (and the reverse): the tile is private
// to the wave, so no workgroup barrier is needed.
__device__ __forceinline__ void sample_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int64_t sample_first_tile(const SampleParams& s, int32_t wave) {
  return s.tile_lo + (int64_t)blockIdx.x * kWavesPerBlock + wave;
}
__device__ __forceinline__ int64_t sample_tile_stride() { return (int64_t)gridDim.x * kWavesPerBlock; }

// What slot `lane` of tile `t` holds: its instance (-1 past the batch), whether that is in
// [lo, hi), has status OK, is in the sample, and the snapshot's completion tick (-1 outside the range).
struct SampleLane {
  int64_t inst;
  bool in, ok, sample;
  int32_t tick;
};
//
// With an instance set (s.where) only its members are in the sample; `in` and `ok` still describe
// the range.  Where slot = instance the tile's 64 instances are bitmap word t: one wave-uniform
// load per tile, each lane tests its own bit, and a tile whose word is 0 reads the status words
// only.  Through a slot -> instance map every lane gathers the word of its instance.  A lane that is
// no member does not read its tick (it stays -1).
__device__ __forceinline__ SampleLane sample_lane(const SampleParams& s, int64_t t, int32_t lane) {
  const int64_t slot = t * 64 + lane;
  SampleLane l{-1, false, false, false, -1};
  const bool mapped = s.blocked && s.inst_map;
  if (slot < s.n_inst) l.inst = mapped ? (int64_t)s.inst_map[slot] : slot;
  l.in = l.inst >= s.lo && l.inst < s.hi;
  bool member = true;
  if (s.where) {  // (uniform over the grid)
    if (mapped) {
      if (l.in) member = (s.where[l.inst >> 6] >> (l.inst & 63)) & 1ULL;
    } else {
      // t is the same in every lane of the wave: a scalar load
      const uint32_t t_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)t);
      const uint32_t t_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)((uint64_t)t >> 32));
      member = (s.where[((uint64_t)t_hi << 32) | t_lo] >> lane) & 1ULL;
    }
  }
  if (l.in) {
    l.ok = s.regs[l.inst * R_NUM + R_STATUS] == ST_OK;
    if (member) {
      l.tick = s.snap_tick[l.inst * s.s_cap + s.sid];
      l.sample = l.ok && l.tick >= 0;
    }
  }
  return l;
}

// The counters of a call's info: instances of the range, those with status OK, those in the sample.
struct SampleCounts {
  unsigned long long n_all = 0, n_ok = 0, n_sample = 0;
  __device__ __forceinline__ void add(const SampleLane& l) { n_all += l.in, n_ok += l.ok, n_sample += l.sample; }
  // the wave's totals into the workgroup's LDS scalars scal[0 .. 2] (zeroed; a barrier follows)
  __device__ __forceinline__ void fold_wave(unsigned long long* scal, int32_t lane) {
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
  }
};
// After the barrier: the workgroup's scalars into the call's three global counters, one thread each.
__device__ __forceinline__ void sample_counts_to_global(const unsigned long long* scal, unsigned long long* n_all,
                                                        unsigned long long* n_ok, unsigned long long* n_sample) {
  if (threadIdx.x < 3 && scal[threadIdx.x])
    atomicAdd(threadIdx.x == 0 ? n_all : threadIdx.x == 1 ? n_ok : n_sample, scal[threadIdx.x]);
}

// The chunk that is the whole record (N * rw <= kStatsChunkWords: stats_chunk(N, rw, 0)).
__device__ __forceinline__ StatsChunk whole_record_chunk(const SampleParams& s) {
  return StatsChunk{0, s.n_nodes, 0, s.rw};
}

// The record words of tile t of snapshot sid's plane: 64 * N * rw words, contiguous in both layouts.
__device__ __forceinline__ const uint32_t* sample_tile_records(const SampleParams& s, int64_t t) {
  const size_t NW = (size_t)s.n_nodes * (size_t)s.rw;
  return s.snap_nod + ((size_t)s.sid * (size_t)s.stride + (size_t)t * 64) * NW;
}

// One load of E words (4: dwordx4) per step, in memory order.  A chunk's words of one record are a
// piece of kw words; a load is piece g = f / kq, q-th load of it.
template <bool kBlocked, int E>
__device__ __forceinline__ void stage_rows(const uint32_t* src, int32_t rw, int32_t row, const StatsChunk& ch,
                                           uint32_t* tile, int32_t lane) {
  const int32_t K = ch.nv * ch.kw, pitch = K | 1;
  // block-major: pieces of one record each -- rows of node v are 64 records at pitch rw, nodes at
  // pitch 64 * rw, so piece g of the chunk is record v0 * 64 + g of the tile; instance-major: one
  // piece of K words per row, starting at word w0 of its N * rw.  (Offsets within a tile are
  // 32-bit: with N <= kMaxNodes its 64 * N * rw words are far fewer than 2^31.)
  const int32_t kq = (kBlocked ? ch.kw : K) / E, pieces = kBlocked ? ch.nv * 64 : 64;
  // (not unrolled: with the whole-record chunk's constants the compiler would unroll the loop, which
  // takes cl_select_eval from 59 to 92 VGPRs and from 7 to 5 waves per SIMD)
#pragma unroll 1
  for (int32_t f = lane; f < pieces * kq; f += 64) {
    const int32_t g = f / kq, k = E * (f - g * kq);
    const uint32_t* from;
    uint32_t* d;
    if (kBlocked) {
      from = src + (uint32_t)((ch.v0 * 64 + g) * rw + ch.k0 + k);
      d = tile + (g & 63) * pitch + (g >> 6) * ch.kw + k;
    } else {
      from = src + (uint32_t)(g * row + (ch.v0 * rw + ch.k0) + k);
      d = tile + g * pitch + k;
    }
    if (E == 4) {
      const uint4 x = *reinterpret_cast<const uint4*>(from);
      d[0] = x.x, d[1] = x.y, d[2] = x.z, d[3] = x.w;
    } else {
      d[0] = from[0];
    }
  }
}

// Stages 64 rows x the K = nv * kw words of chunk `ch` of tile t into the wave's LDS tile
// [64][K | 1]: row r is slot 64 t + r, word k of it is word (v0 + k / kw) * rw + k0 + k % kw of
// the slot's record.  Wave-uniform; fenced on both sides (the previous readers are done with the
// tile; the rows are visible to every lane after it).
__device__ __forceinline__ void stage_tile(const SampleParams& s, int64_t t, const StatsChunk& ch, uint32_t* tile,
                                           int32_t lane) {
  const uint32_t* src = sample_tile_records(s, t);
  const int32_t row = s.n_nodes * s.rw;
  const bool vec = (s.rw & 3) == 0;
  sample_wave_sync();
  if (s.blocked) {
    if (vec) stage_rows<true, 4>(src, s.rw, row, ch, tile, lane);
    else stage_rows<true, 1>(src, s.rw, row, ch, tile, lane);
  } else {
    if (vec) stage_rows<false, 4>(src, s.rw, row, ch, tile, lane);
    else stage_rows<false, 1>(src, s.rw, row, ch, tile, lane);
  }
  sample_wave_sync();
}

// Reads word idx of the N * rw record words of the lane's slot in tile t: when `staged`, from the
// tile staged with whole_record_chunk, else from the plane (instance-major: the slot's words are
// contiguous; block-major: word idx % rw of node idx / rw's record).  snapshot_key takes it as
// its `word`.
struct RecordRow {
  const uint32_t* tile;  // the wave's LDS tile
  const uint32_t* src;   // sample_tile_records
  int32_t lane, rw, nw, blocked, staged;
  __device__ __forceinline__ RecordRow(const SampleParams& s, int64_t t, int32_t lane_, const uint32_t* tile_,
                                       int32_t staged_)
      : tile(tile_), src(sample_tile_records(s, t)), lane(lane_), rw(s.rw), nw(s.n_nodes * s.rw), blocked(s.blocked),
        staged(staged_) {}
  __device__ __forceinline__ uint32_t operator()(int32_t idx) const {
    if (staged) return tile[lane * (nw | 1) + idx];
    if (!blocked) return src[(size_t)lane * nw + idx];
    const int32_t v = idx / rw;
    return src[((size_t)v * 64 + lane) * rw + (idx - v * rw)];
  }
};
// Word idx of the N * rw record words of (snapshot sid, instance inst), read from the plane in
// either layout (rec_word; rec_slot: instance -> record slot of block-major records, else nullptr).
struct PlaneRow {
  const uint32_t* nod;
  const int32_t* rec_slot;
  int64_t stride, inst;
  int32_t n_nodes, rw, sid;
  __device__ __forceinline__ uint32_t operator()(int32_t idx) const {
    return nod[rec_word(stride, n_nodes, rw, sid, inst, rec_slot, idx)];
  }
};

// A channel's cursor word: begin and end index into its token history, 16 bits each.
__device__ __forceinline__ uint32_t rec_msgs(uint32_t rec) { return (rec >> 16) - (rec & 0xffffu); }
// The int64 prefix sums of channel c's token history (the host stores channel c at hist_off[c] + c:
// one more entry per channel than the history has).
__device__ __forceinline__ const long long* token_prefix(const RecordTables& tab, int32_t c) {
  return tab.hist_pre + tab.hist_off[c] + c;
}
// The recorded tokens of the cursor word: two loads of the channel's prefix (none for no messages).
__device__ __forceinline__ long long rec_tokens(uint32_t rec, const long long* pre) {
  const uint32_t b = rec & 0xffffu, e = rec >> 16;
  return e != b ? pre[e] - pre[b] : 0;
}
// The content hash of the record `word` reads, as snapshot sid's: the census key (snapshot_key).
template <class Word>
__device__ __forceinline__ unsigned long long record_key(const SampleParams& s, const RecordTables& tab, int32_t sid,
                                                         const Word& word) {
  return snapshot_key(sid, s.n_nodes, s.rw, s.n_ch, tab.ch_slot, tab.hist_off, tab.hist_val, word);
}

}  // namespace clsnap
