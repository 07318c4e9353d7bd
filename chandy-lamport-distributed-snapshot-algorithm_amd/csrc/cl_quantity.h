// cl_quantity.h -- a quantity of a snapshot, the one definition behind the select clause
// (cl_select.hip), the crosstab axis (cl_crosstab.hip) and the group term (cl_groups.hip).
// Device code, like cl_sample.h; the fields and their validity check are cl_analytics.h's.
//
// A quantity (sid, field, index) has one int64 value per instance in which snapshot `sid`
// completed, whichever call reads it: quantity_value() computes it from the snapshot's completion
// tick and a reader of the instance's record of that snapshot (RecordRow in a sample walk, PlaneRow
// for a single instance).  A walk is that of one snapshot id; a quantity of another one is read
// through a view of the same walk (sample_view, view_tick): the slot -> instance map of block-major
// records is shared by all snapshot planes, so tile t names the same 64 instances in every view.
#pragma once
#include <hip/hip_runtime.h>

#include "cl_sample.h"

namespace clsnap {

// The view of snapshot `sid` of the walk `s`: the same walk, another plane.
__device__ __forceinline__ SampleParams sample_view(const SampleParams& s, int32_t sid) {
  SampleParams v = s;
  v.sid = sid;
  return v;
}
// The completion tick of snapshot `sid` of the lane's instance (l.in): the lane's own for the
// walk's snapshot, else read from the instance's snap_tick row.
__device__ __forceinline__ int32_t view_tick(const SampleParams& s, const SampleLane& l, int32_t sid) {
  return sid == s.sid ? l.tick : s.snap_tick[l.inst * s.s_cap + sid];
}

// The instance's totals of recorded messages and tokens: one pass over the C cursor words.
struct ChannelTotals {
  long long msgs, inflight;
};
template <class Word>
__device__ __forceinline__ ChannelTotals channel_totals(const SampleParams& s, const RecordTables& tab,
                                                        const Word& word) {
  ChannelTotals t{0, 0};
  for (int32_t c = 0; c < s.n_ch; ++c) {
    const uint32_t rec = word(tab.ch_slot[c]);
    t.msgs += (long long)rec_msgs(rec);
    t.inflight += rec_tokens(rec, token_prefix(tab, c));
  }
  return t;
}

// What a caller that evaluates several quantities of one record computes once and hands to
// quantity_value (the select clauses): the totals, when a quantity names one, and the key likewise.
struct QuantityOnce {
  ChannelTotals totals;
  unsigned long long key;
};

// The value of quantity (sid, field, index), field <= kMaxField, for one instance: its completion
// tick `tick` of snapshot sid, or what the field names of the record `word` reads (the instance's
// record of snapshot sid); the key as its bit pattern.
template <int32_t kMaxField, class Word>
__device__ __forceinline__ long long quantity_value(const SampleParams& s, const RecordTables& tab, int32_t sid,
                                                    int32_t field, int32_t index, const Word& word, int32_t tick,
                                                    const QuantityOnce* once = nullptr) {
  switch (field) {
    case SEL_MSGS: return once ? once->totals.msgs : channel_totals(s, tab, word).msgs;
    case SEL_INFLIGHT: return once ? once->totals.inflight : channel_totals(s, tab, word).inflight;
    case SEL_NODE: return (int32_t)word(index * s.rw);
    case SEL_CH_MSGS: return (long long)rec_msgs(word(tab.ch_slot[index]));
    case SEL_CH_TOK: return rec_tokens(word(tab.ch_slot[index]), token_prefix(tab, index));
    case SEL_KEY:
      if constexpr (kMaxField >= SEL_KEY) return (long long)(once ? once->key : record_key(s, tab, sid, word));
      else return tick;
    default: return tick;
  }
}

}  // namespace clsnap
