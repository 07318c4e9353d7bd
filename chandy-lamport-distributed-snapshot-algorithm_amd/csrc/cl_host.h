// cl_host.h -- what the analytics host layer (cl_analytics.cpp) knows of a cl_sim: cl_host.cpp
// defines the sim and the functions of the first part, cl_analytics.cpp the second.  The analytics
// read a sim through these only; they see no field of it.
#pragma once
#include "cl_analytics.h"
#include "cl_dev.h"

struct cl_sim;

namespace clsnap {

// ---- of cl_host.cpp ---------------------------------------------------------------------------
// The opening of an ABI call on a sim: a null handle is refused, the sim's (recursive) lock is
// held while the guard lives, and a pipelined replay's stream2 half is joined first (`join`: every
// call but cl_rerun and the host-only cl_stats_layout_of).  A constructor cannot return from its
// caller, so SIM_CALL(sim[, join]) opens a call: the guard, and the return of its failure.
class SimCall {
 public:
  explicit SimCall(const cl_sim* sim, bool join = true);
  ~SimCall();
  SimCall(const SimCall&) = delete;
  SimCall& operator=(const SimCall&) = delete;
  int rc;

 private:
  const cl_sim* locked_ = nullptr;
};
#define SIM_CALL(...)                 \
  clsnap::SimCall call_(__VA_ARGS__); \
  if (call_.rc) return call_.rc

// What the argument checks need; no device work behind it (every argument is checked before any).
struct SimFacts {
  int64_t n_inst, stride;
  int64_t n_nodes, n_ch;  // nodes and channels added so far
  int32_t n_sids;
  bool dev_ready;         // the sim has its device and stream
  bool ran;               // an event was issued, or dev_ready
};
SimFacts sim_facts(const cl_sim* sim);

// The sim's device, chosen and made current (also before anything has run), its stream, and the
// CU count the grids are sized by (one cached value, the delay generator's too).
struct SimDevice {
  int device;
  hipStream_t stream;
  int32_t n_cus;
};
int sim_device(cl_sim* sim, SimDevice* out);

// The tables next to the records, resident after sim_records.
struct SimTables : RecordTables {
  const int32_t* word_ch;  // [N * rw] record word -> channel, -2 token word, -1 padding
  // instance -> record slot of block-major records (rec_word; the map the packed collect over a
  // list uses), nullptr when the records are instance-major
  const int32_t* rec_slot;
};
// Executes what is pending, makes the device current (*dev as from sim_device) and the token
// histories resident, and fills the plane fields of *s (n_nodes .. snap_nod, blocked, inst_map);
// the sample's own fields are the caller's.
int sim_records(cl_sim* sim, SimDevice* dev, SampleParams* s, SimTables* t);

// ---- of cl_analytics.cpp ------------------------------------------------------------------------
// A sim's analytics scratch, timers and instance sets.  The sim makes it with itself and deletes
// it once its streams are idle (a kernel may still read a set's bitmap before that).
struct Analytics;
Analytics* analytics_new(cl_sim* sim);
void analytics_delete(Analytics* a);
Analytics* sim_analytics(const cl_sim* sim);  // (defined in cl_host.cpp)
int64_t analytics_device_bytes(const Analytics* a);

// The arguments every call over a sample shares (after the call's own): the instance range, a sim
// that has run something, the snapshot id.
int sample_args_ok(const cl_sim* sim, int32_t sid, int64_t inst_lo, int64_t inst_hi);

}  // namespace clsnap
