// cl_plan.h -- the batch engine's replay plan: what the first fresh full run of a program (the
// probe) teaches the host about its replays, and the one owner of what is derived from it on the
// device.  cl_plan.cpp defines it and the cl_replay_plan_of ABI function; a cl_sim holds one
// ReplayPlan by value and sees no field of it.
//
// The probe runs ops [0, n_ops) on the spill-capable kernel with per-instance spill flags.  Its
// replays (cl_rerun: the same program and delays, hence the same queues and final ticks) launch
// through a slot map: instances grouped by their final tick so the 64 / N instances sharing a wave
// end their drains together, and the instances that spilled last; slots [0, split_slot) then run
// the spill-free kernel (6 waves per SIMD at degree bounds 3-4) and the rest the spill-capable
// one, concurrently on a second stream.  Results are per instance and identical on either kernel.
//
// The rules:
//   * A plan ends in drop() and nowhere else: whoever changes the delays, the layout, the exec
//     engine or the rows on the device calls it.  drop() also forgets a probe that was launched
//     but not yet evaluated (a plan evaluated after a drop would describe what was dropped), so
//     between a drop and the next launch there is no plan, and that launch is a probe again.
//   * drop() leaves the buffers and the record order alone: the records on the device are still
//     those of the latest launch, and their readers need the order they were written in.
//   * The slot map on the device is overwritten only at a probe's end.  The probe itself is a
//     launch from the initial state that is not a replay of a plan, so it left the records
//     instance-major (wrote_records(false)) and no reader needs the old map any more.
//   * The packed delay rows are read by both halves of a split replay, and the second stream's
//     half of the next replay does not wait for `stream`.  So the caller of pack_rows first joins
//     the second stream and drains `stream` (an earlier replay may still read the plane), and
//     drains `stream` again after it, before anything is launched.
#pragma once
#include <cstdint>
#include <vector>

#include "cl_delays.h"
#include "cl_dev.h"

namespace clsnap {

// Batches of at least this many instances replay through a length-ordered slot map (a few
// thousand waves: the grouping pays for its one host sort and 4 B per instance of HBM).
constexpr int64_t kMapMinInstances = 4096;

// A length-ordered slot map is used when it keeps at most this % of the wave-ticks of the
// unordered launch (C3 90 %: kept; C2 95 %: measured slower mapped, §9)
constexpr int64_t kMapPct = 92;

// The slot order of a program's replays.
struct PlanOrder {
  std::vector<int32_t> order;  // slot -> instance: the clean instances, then the spilled ones ascending
  bool mapped = false;         // replays launch through `order` (else it is clean-then-spilled, unused)
  bool nospill = false;        // no instance spilled: replays run wholly on the spill-free kernel
  int64_t split_slot = 0;      // slots before it run spill-free, the rest spill-capable (0: no split)
  int64_t n_spilled = 0;
};
// The planning policy, on the host alone: from every instance's final tick and spill flag
// (spilled may be null: none), the instances per wave of the layout and whether the launcher's
// kernels can split a replay (cl_sim::specialized).
PlanOrder plan_order(const int32_t* final_tick, const uint8_t* spilled, int64_t n_inst, int32_t insts_per_wave,
                     bool can_split);

// The order the records on the device were written in: instance-major, or block-major by the slot
// of the replay that wrote them (cl_engine.h rec_word) with that replay's two maps.
struct RecordOrder {
  bool blocked;
  const int32_t* rec_slot;    // device, instance -> slot; nullptr when instance-major
  const int32_t* inst_map;    // device, slot -> instance; nullptr when instance-major
  const int32_t* h_rec_slot;  // rec_slot's host mirror (a one-instance collect)
};

class ReplayPlan {
 public:
  void drop() {
    ops_ = tried_ = -1;
    probe_ = false;
  }
  // A plan exists for a program of n_ops ops; the four below describe it (and mean nothing without).
  bool holds(int64_t n_ops) const { return ops_ == n_ops; }
  bool mapped() const { return mapped_; }
  bool nospill() const { return nospill_; }
  int64_t split_slot() const { return split_; }
  int64_t spilled() const { return spilled_; }
  const int32_t* inst_map() const { return mapped_ ? d_map_.p : nullptr; }

  // Every launch says whether it is a fresh full run of a program no plan holds for.  The first
  // such run of a program is the probe: with spill rings in the layout its per-instance spill
  // flags are cleared on `stream` (once per program, not per replay) and returned for
  // ExecParams::spill_flag; nullptr otherwise.
  int begin_launch(bool unplanned_full_run, int64_t n_ops, bool spill_rings, int64_t n_inst, hipStream_t stream,
                   uint8_t** spill_flag);
  bool probe_pending() const { return probe_; }
  // The probe's end, once its streams are idle: reads the R_TIME column of `regs` and the flags,
  // runs plan_order, and where replays are mapped uploads the map and builds its inverse.
  int end_probe(const int32_t* regs, int64_t n_inst, int32_t insts_per_wave, bool can_split);

  // The instance -> slot table of a block-major replay, resident for this plan: one upload per
  // plan on `stream`, synchronised before it returns.
  int slot_table(hipStream_t stream);
  // The plan's delay rows packed for the instance-per-lane kernel (ExecParams::sched_pk,
  // cl_rowpack.hip), valid for this plan and the rows.gen they were packed from.  A replay that
  // finds rows_packed false calls pack_rows, under the caller's rule at the top.
  bool rows_packed(const DelayRows& rows) const { return pk_for_plan_ == gen_ && pk_rows_gen_ == rows.gen; }
  int pack_rows(const DelayRows& rows, int64_t n_inst, hipStream_t stream);
  const uint32_t* packed_rows() const { return d_sched_pk_.p; }

  // Set by every launch from the initial state (a replay through the map with no state image
  // writes block-major, after slot_table; every other launch instance-major), read by every
  // reader of the records.
  void wrote_records(bool blocked) { rec_blocked_ = blocked; }
  RecordOrder record_order() const {
    return rec_blocked_ ? RecordOrder{true, d_rec_slot_.p, d_map_.p, h_rec_slot_.data()}
                        : RecordOrder{false, nullptr, nullptr, nullptr};
  }

  int64_t device_bytes() const { return (int64_t)d_sched_pk_.bytes(); }  // the packed rows

 private:
  int64_t ops_ = -1;    // program length the plan holds for (-1: none)
  int64_t tried_ = -1;  // program length a probe last ran for
  bool probe_ = false;  // the latest launch was a probe (evaluated at the next sync)
  int64_t probe_ops_ = 0;
  bool probe_flags_ = false;  // the probe recorded spill flags
  bool mapped_ = false, nospill_ = false;
  int64_t split_ = 0, spilled_ = 0;
  DevBuf<uint8_t> d_spill_inst_;  // [n_inst] probe: 1 where a push spilled to HBM
  DevBuf<int32_t> d_map_;         // PlanOrder::order
  std::vector<int32_t> inv_;      // its inverse
  int64_t gen_ = 0;               // maps made so far: what is derived from a map holds for one
  std::vector<int32_t> h_rec_slot_;
  DevBuf<int32_t> d_rec_slot_;
  int64_t rec_slot_for_ = -1;  // gen_ of the map the slot table is the inverse of
  bool rec_blocked_ = false;
  DevBuf<uint32_t> d_sched_pk_;
  int64_t pk_for_plan_ = -1, pk_rows_gen_ = -1;
};

}  // namespace clsnap
