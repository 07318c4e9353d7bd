// cl_groups.h -- group-by over a tuple of snapshot quantities (cl_groups.hip; include/clsnap.h
// cl_snapshot_groups).  Declarations shared by the kernels and the analytics host layer; kept out
// of cl_engine.h, which is also compiled into the run-time lanes kernel.
//
// A term names one of the quantities a select clause names (SEL_TICK .. SEL_KEY) of one snapshot
// id.  The sample is the instances of [lo, hi) with status OK in which the snapshot of every term
// completed; a group is the set of sample instances with the same tuple of term values, keyed by
// group_key().  Equality of groups MEANS equality of that 64-bit key: tuples are not compared.
#pragma once
#include "cl_engine.h"

namespace clsnap {

constexpr int32_t kGroupsMaxTerms = 8;
struct GroupTerm {  // the layout of cl_group_term
  int32_t sid, field, index, reserved;
};

// group_key(v[0 .. n)): h = 0x9E3779B97F4A7C15 ^ n, then h = mix64(h ^ v[k]) in term order.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint64_t group_key_seed(int32_t n) { return 0x9E3779B97F4A7C15ULL ^ (uint64_t)n; }
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint64_t group_key_fold(uint64_t h, int64_t v) { return mix64(h ^ (uint64_t)v); }

struct GroupsParams {
  // The walk, the planes of terms[0]'s snapshot (c.s.sid == term[0].sid) and the census's table:
  // the init / gather / rank / lookup kernels of cl_census.hip run on `c` as they are.
  CensusParams c;
  const long long* hist_pre;  // as StatsParams::hist_pre
  int32_t n_terms;
  GroupTerm term[kGroupsMaxTerms];
  // the distinct snapshot ids of term[1 ..] other than term[0].sid: a sample lane leaves the sample
  // when one of them did not complete
  int32_t n_other;
  int32_t other_sid[kGroupsMaxTerms];
  int32_t reads_records;  // a term reads the records (any field but SEL_TICK)
};
// The key pass: c.table / c.list / c.info filled as launch_census_keys fills them.
int launch_groups_keys(const GroupsParams& p, int32_t blocks, void* stream);
// values[g * n_terms + k] = term k of instance first[g], g < n.  rec_slot: instance -> record slot
// of block-major records (SimTables::rec_slot), nullptr when they are instance-major.
int launch_groups_values(const GroupsParams& p, const int32_t* rec_slot, const long long* first, int64_t n,
                         long long* values, void* stream);

}  // namespace clsnap
