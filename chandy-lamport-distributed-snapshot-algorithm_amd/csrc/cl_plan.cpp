// cl_plan.cpp -- the replay plan (cl_plan.h): the planning policy on the host, the probe that
// feeds it, and what a plan keeps on the device.
#include "cl_plan.h"

#include <algorithm>

#include "cl_engine.h"

namespace clsnap {

namespace {
// Sum over waves of the longest instance (wave-ticks) of a slot order.
int64_t wave_ticks(const int32_t* t, const std::vector<int32_t>& order, int64_t ipw) {
  const int64_t n = (int64_t)order.size();
  int64_t sum = 0;
  for (int64_t w = 0; w < n; w += ipw) {
    int32_t m = 0;
    for (int64_t k = w; k < std::min(w + ipw, n); ++k) m = std::max(m, t[order[(size_t)k]]);
    sum += m;
  }
  return sum;
}
}  // namespace

PlanOrder plan_order(const int32_t* t, const uint8_t* sp, int64_t n_inst, int32_t insts_per_wave, bool can_split) {
  PlanOrder po;
  // the length of an instance's replay: its final tick (one tick-loop iteration per tick)
  std::vector<int32_t> clean, spilled;
  for (int64_t i = 0; i < n_inst; ++i) (sp && sp[i] ? spilled : clean).push_back((int32_t)i);
  po.n_spilled = (int64_t)spilled.size();
  po.nospill = spilled.empty();
  // length order of the clean instances: one global counting sort by final tick (sorting
  // within windows of 64 waves instead, to keep each window's scattered per-instance stores
  // close in time, measured C3 2.71 -> 2.96 ms: the global order is kept)
  int32_t mx = 0;
  for (int32_t i : clean) mx = std::max(mx, t[i]);
  std::vector<int64_t> start((size_t)mx + 2, 0);
  for (int32_t i : clean) start[(size_t)std::max(t[i], 0) + 1]++;
  for (size_t k = 1; k < start.size(); ++k) start[k] += start[k - 1];
  std::vector<int32_t> by_len(clean.size());
  for (int32_t i : clean) by_len[(size_t)start[(size_t)std::max(t[i], 0)]++] = i;
  // longest waves first (LPT): the dispatcher starts workgroups in slot order as resident
  // ones retire, so the last to start are the shortest and the grid drains evenly
  std::reverse(by_len.begin(), by_len.end());
  const int64_t nc = (int64_t)clean.size(), ipw = insts_per_wave;
  // split replays: the clean instances' whole waves on the spill-free kernel (a wave that
  // holds a spilling instance runs spill-capable), when the launcher's kernels can split
  const bool split = !spilled.empty() && can_split;
  // The length order is worth it only when it removes enough wave-ticks to pay for the scattered
  // stores (C3: 43.9 -> 39.5 ticks per wave, kept; C2: 55.8 -> 52.8, measured slower mapped).  A
  // split launches through the map anyway (its scattered result stores are paid), so the clean
  // instances then go in length order too (C2: 0.1829 -> 0.1807 ms per step)
  const bool sort = n_inst >= kMapMinInstances &&
                    (split || wave_ticks(t, by_len, ipw) * 100 <= wave_ticks(t, clean, ipw) * kMapPct);
  po.order = sort ? by_len : clean;
  po.order.insert(po.order.end(), spilled.begin(), spilled.end());
  if (split) po.split_slot = nc / ipw * ipw;
  po.mapped = sort || po.split_slot > 0;
  return po;
}

int ReplayPlan::begin_launch(bool unplanned_full_run, int64_t n_ops, bool spill_rings, int64_t n_inst,
                             hipStream_t stream, uint8_t** spill_flag) {
  probe_ = unplanned_full_run && tried_ != n_ops;
  probe_ops_ = n_ops;
  probe_flags_ = probe_ && spill_rings;
  *spill_flag = nullptr;
  if (!probe_flags_) return CL_OK;
  if (int rc = d_spill_inst_.ensure((size_t)n_inst)) return rc;
  HIP_TRY(hipMemsetAsync(d_spill_inst_.p, 0, (size_t)n_inst, stream));
  *spill_flag = d_spill_inst_.p;
  return CL_OK;
}

int ReplayPlan::end_probe(const int32_t* regs, int64_t n_inst, int32_t insts_per_wave, bool can_split) {
  probe_ = false;
  tried_ = probe_ops_;
  mapped_ = nospill_ = false;
  split_ = spilled_ = 0;
  std::vector<int32_t> t((size_t)n_inst);
  HIP_TRY(hipMemcpy2D(t.data(), sizeof(int32_t), regs + R_TIME, R_NUM * sizeof(int32_t), sizeof(int32_t), t.size(),
                      hipMemcpyDeviceToHost));
  std::vector<uint8_t> sp;
  if (probe_flags_) {
    sp.resize((size_t)n_inst);
    HIP_TRY(hipMemcpy(sp.data(), d_spill_inst_.p, sp.size(), hipMemcpyDeviceToHost));
  }
  const PlanOrder po = plan_order(t.data(), probe_flags_ ? sp.data() : nullptr, n_inst, insts_per_wave, can_split);
  if (po.mapped) {
    if (int rc = d_map_.upload(po.order)) return rc;
    // the inverse (instance -> slot): where a block-major replay puts each instance's records
    inv_.assign(po.order.size(), 0);
    for (size_t i = 0; i < po.order.size(); ++i) inv_[(size_t)po.order[i]] = (int32_t)i;
    gen_ += 1;
  }
  mapped_ = po.mapped;
  nospill_ = po.nospill;
  split_ = po.split_slot;
  spilled_ = po.n_spilled;
  ops_ = probe_ops_;
  return CL_OK;
}

int ReplayPlan::slot_table(hipStream_t stream) {
  if (rec_slot_for_ == gen_) return CL_OK;
  if (int rc = d_rec_slot_.ensure(inv_.size())) return rc;
  HIP_TRY(hipMemcpyAsync(d_rec_slot_.p, inv_.data(), inv_.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  h_rec_slot_ = inv_;
  rec_slot_for_ = gen_;
  return CL_OK;
}

int ReplayPlan::pack_rows(const DelayRows& rows, int64_t n_inst, hipStream_t stream) {
  if (int rc = d_sched_pk_.ensure(row_pack_words(n_inst, rows.row))) return rc;
  const int pe = launch_row_pack(rows.d, rows.row, d_map_.p, n_inst, d_sched_pk_.p, stream);
  if (pe != 0) return set_err(CL_E_DEVICE, "row pack launch failed: %s", hipGetErrorString((hipError_t)pe));
  pk_for_plan_ = gen_;
  pk_rows_gen_ = rows.gen;
  return CL_OK;
}

}  // namespace clsnap

extern "C" int cl_replay_plan_of(const int32_t* final_ticks, const uint8_t* spilled, int64_t n, int32_t insts_per_wave,
                                 int32_t can_split, int32_t* order, int32_t* mapped, int64_t* split_slot,
                                 int64_t* n_spilled) {
  using namespace clsnap;
  if (!final_ticks || n <= 0 || insts_per_wave <= 0)
    return set_err(CL_E_INVALID, "cl_replay_plan_of needs final ticks, n > 0 and insts_per_wave > 0");
  const PlanOrder po = plan_order(final_ticks, spilled, n, insts_per_wave, can_split != 0);
  if (order) std::copy(po.order.begin(), po.order.end(), order);
  if (mapped) *mapped = po.mapped ? 1 : 0;
  if (split_slot) *split_slot = po.split_slot;
  if (n_spilled) *n_spilled = po.n_spilled;
  return CL_OK;
}
