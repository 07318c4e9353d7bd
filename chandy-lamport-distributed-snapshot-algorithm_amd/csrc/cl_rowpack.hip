// cl_rowpack.hip -- the delay rows of a replay plan, packed for the instance-per-lane kernel.
//
// A replay through the slot map runs the same schedule again: lane l of a wave runs the instance
// inst_map[slot], and its prologue (cl_lanes.h program()) needs that instance's delay row as
// nibbles in its LDS column.  From the byte rows that is 64 scattered rows per wave, fetched after
// the slot map's own load, and the same byte-to-nibble repacking on every replay.  This kernel
// does it once per plan and schedule: out word w of slot r, at ((r / 64) * nd + w) * 64 + r % 64
// (nd = sched_row / 8 words per row, ExecParams::sched_pk), holds delays 8 w .. 8 w + 7 of
// instance inst_map[r], delay k in bits 4 k .. 4 k + 3 -- the column word as the prologue builds it.
// One thread per (slot, word): 8 bytes read, one word stored, consecutive threads on consecutive
// slots so the stores of a wave are contiguous.  Slots at and above n_inst get no word (a
// launch's lanes past the batch load none).
#include <hip/hip_runtime.h>

#include "cl_engine.h"

namespace clsnap {
namespace {

constexpr int kPackThreads = 256;

__global__ __launch_bounds__(kPackThreads) void cl_row_pack(const uint8_t* __restrict__ sched, int64_t sched_row,
                                                            const int32_t* __restrict__ inst_map, int64_t n_inst,
                                                            uint32_t* __restrict__ out) {
  const int64_t nd = sched_row / 8;
  const int64_t blocks = (n_inst + 63) / 64;
  // thread t: slot lane t % 64 of (block, word) pair t / 64
  const int64_t t = (int64_t)blockIdx.x * kPackThreads + threadIdx.x;
  const int64_t pair = t >> 6, lane = t & 63;
  if (pair >= blocks * nd) return;
  const int64_t blk = pair / nd, w = pair - blk * nd;
  const int64_t slot = blk * 64 + lane;
  if (slot >= n_inst) return;
  const int64_t inst = inst_map[slot];
  const uint2 b = *reinterpret_cast<const uint2*>(sched + inst * sched_row + w * 8);  // (rows are multiples of 16 bytes)
  auto nib = [](uint32_t x) { return (x & 0xfu) | ((x >> 4) & 0xf0u) | ((x >> 8) & 0xf00u) | ((x >> 12) & 0xf000u); };
  out[pair * 64 + lane] = nib(b.x) | (nib(b.y) << 16);
}

}  // namespace

int launch_row_pack(const uint8_t* sched, int64_t sched_row, const int32_t* inst_map, int64_t n_inst, uint32_t* out,
                    void* stream) {
  const int64_t threads = (n_inst + 63) / 64 * (sched_row / 8) * 64;
  if (threads <= 0) return 0;
  const int64_t grid = (threads + kPackThreads - 1) / kPackThreads;
  if (grid > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(cl_row_pack, dim3((uint32_t)grid), dim3(kPackThreads), 0, (hipStream_t)stream, sched, sched_row,
                     inst_map, n_inst, out);
  return (int)hipGetLastError();
}

}  // namespace clsnap
