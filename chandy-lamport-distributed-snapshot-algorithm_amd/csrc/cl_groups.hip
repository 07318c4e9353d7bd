// cl_groups.hip -- group-by over a tuple of snapshot quantities of the batch engine
// (cl_snapshot_groups).
//
// GROUP BY (q1, ..., qk), k <= kGroupsMaxTerms, over quantities of snapshots (cl_quantity.h), possibly
// of different snapshot ids: exact, without bin edges, one row per tuple that occurs.  The sample is
// the instances of [lo, hi) with status OK in which the snapshot of every term completed -- of the
// members of an instance set when one is given.  Groups are keyed by the 64-bit group_key() of the
// tuple (cl_analytics.h); per group the census's row: count, smallest instance, min and max completion
// tick of terms[0]'s snapshot.  All integer and commutative, so the result does not depend on the
// grid, the workgroup tables, the record layout or the exec kernel.
//
// Key pass (cl_groups_keys).  The sample walk of cl_sample.h, lane = slot.  sample_lane() classifies
// the slot for terms[0]'s snapshot; a sample lane then reads the completion tick of every other
// distinct snapshot id (view_tick) and leaves the sample if one is negative (the crosstab's scheme,
// for up to 8 ids); every term is read through the view of its snapshot (sample_view).  The key is
// folded as a running hash in term order: no lane keeps an array of values.  A term that reads
// records needs its snapshot's plane: records of at most kCensusStageWords words are staged in the
// wave's LDS tile (stage_tile, whole-record chunk)
// unless the tile already holds that snapshot -- adjacent terms of one snapshot id stage once,
// alternating ids restage -- and longer records are read word by word (RecordRow).  A term list of
// completion ticks reads no records.  Aggregation is the census's (cl_census_table.h).
//
// Values (cl_groups_values).  After the host's sort, one lane per returned group evaluates the terms
// for the group's smallest instance with the same quantity_value(): the records are addressed directly
// (PlaneRow; block-major through the instance -> slot map of the replay).
//
// group_of reuses cl_census_rank / cl_census_lookup (launch_census_class_of).
#include <hip/hip_runtime.h>

#include "cl_census_table.h"
#include "cl_quantity.h"

namespace clsnap {
namespace {

__global__ __launch_bounds__(kCensusThreads) void cl_groups_keys(GroupsParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char groups_lds[];
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const CensusLds L = census_lds(groups_lds, p.c.lds_slots, wave);
  census_lds_init(L, p.c.lds_slots, p.c.empty_key);
  const int32_t staged = p.c.staged && p.reads_records;

  SampleCounts counts;
  for (int64_t t = sample_first_tile(p.c.s, wave); t < p.c.s.tile_hi; t += sample_tile_stride()) {
    SampleLane l = sample_lane(p.c.s, t, lane);
    const int64_t inst = l.inst;
    // ---- the sample: every other snapshot id completed, too
    if (l.sample)
      for (int32_t q = 0; q < p.n_other; ++q)
        if (view_tick(p.c.s, l, p.other_sid[q]) < 0) l.sample = false;
    counts.add(l);
    if (l.in && p.c.keys && !l.sample) p.c.class_of[inst - p.c.s.lo] = -1;
    if (__ballot(l.sample) == 0) continue;  // (wave-uniform)

    // ---- the key: a running hash over the terms, the tile restaged when the snapshot id changes
    unsigned long long key = group_key_seed(p.n_terms);
    int32_t staged_sid = -1;  // (wave-uniform) the snapshot whose records the tile holds
#pragma unroll 1
    for (int32_t k = 0; k < p.n_terms; ++k) {
      const GroupTerm z = p.term[k];
      const SampleParams sv = sample_view(p.c.s, z.sid);  // term k's snapshot: the same walk, another plane
      if (staged && z.field != SEL_TICK && staged_sid != z.sid) {
        stage_tile(sv, t, whole_record_chunk(sv), L.tile, lane);
        staged_sid = z.sid;
      }
      if (l.sample)
        key = group_key_fold(key, quantity_value<SEL_KEY>(sv, p.c.tab, z.sid, z.field, z.index,
                                                          RecordRow(sv, t, lane, L.tile, staged),
                                                          view_tick(p.c.s, l, z.sid)));
    }
    if (!l.sample) continue;
    if (p.c.keys) {
      p.c.keys[inst - p.c.s.lo] = key;
      p.c.class_of[inst - p.c.s.lo] = 0;
    }
    census_insert(p.c, L, key, inst, l.tick);
  }
  census_lds_flush(p.c, L, counts, lane);
}

__global__ __launch_bounds__(kCensusThreads) void cl_groups_values(GroupsParams p, const int32_t* rec_slot,
                                                                   const long long* first, int64_t n,
                                                                   long long* values) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const SampleParams& s = p.c.s;
  const int64_t inst = first[g];
  const bool known = inst >= 0 && inst < s.n_inst;  // (a group's smallest instance always is)
#pragma unroll 1
  for (int32_t k = 0; k < p.n_terms; ++k) {
    const GroupTerm z = p.term[k];
    long long v = 0;
    if (known) {
      const PlaneRow row{s.snap_nod, rec_slot, s.stride, inst, s.n_nodes, s.rw, z.sid};
      v = quantity_value<SEL_KEY>(s, p.c.tab, z.sid, z.field, z.index, row, s.snap_tick[inst * s.s_cap + z.sid]);
    }
    values[g * p.n_terms + k] = v;
  }
}

bool terms_ok(const GroupsParams& p) {
  const SampleParams& s = p.c.s;
  if (p.n_terms < 1 || p.n_terms > kGroupsMaxTerms || p.n_other < 0 || p.n_other >= kGroupsMaxTerms) return false;
  if (s.sid != p.term[0].sid) return false;
  for (int32_t k = 0; k < p.n_terms; ++k) {
    const GroupTerm& z = p.term[k];
    if (!quantity_ok(z.field, z.index, SEL_KEY, s.n_nodes, s.n_ch) || z.sid < 0 || z.sid >= s.s_cap) return false;
  }
  for (int32_t q = 0; q < p.n_other; ++q)
    if (p.other_sid[q] < 0 || p.other_sid[q] >= s.s_cap) return false;
  return true;
}

}  // namespace

int launch_groups_keys(const GroupsParams& p, int32_t blocks, void* stream) {
  const bool staged = p.c.staged != 0 && p.reads_records != 0;
  const size_t lds = (size_t)census_lds_bytes(p.c.lds_slots, staged);
  if (lds > (size_t)kMaxLdsBytes || blocks < 1 || !terms_ok(p) || !staged_ok(p.c.s, p.c.staged))
    return (int)hipErrorInvalidValue;
  if (lds > 64 * 1024) {
    const hipError_t e =
        hipFuncSetAttribute((const void*)cl_groups_keys, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(cl_groups_keys, dim3((unsigned)blocks), dim3(kCensusThreads), lds, (hipStream_t)stream, p);
  return (int)hipGetLastError();
}

int launch_groups_values(const GroupsParams& p, const int32_t* rec_slot, const long long* first, int64_t n,
                         long long* values, void* stream) {
  if (n < 1) return 0;
  if (!terms_ok(p) || (p.c.s.blocked != 0) != (rec_slot != nullptr)) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((n + kCensusThreads - 1) / kCensusThreads);
  hipLaunchKernelGGL(cl_groups_values, dim3(blocks), dim3(kCensusThreads), 0, (hipStream_t)stream, p, rec_slot, first,
                     n, values);
  return (int)hipGetLastError();
}

}  // namespace clsnap
