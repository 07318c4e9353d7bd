// cl_delays.h -- the batch engine's delay source: which delays the instances draw (Go math/rand
// streams by seed, from either generator, or a caller's schedule) and the one owner of their rows
// on the device.  cl_delays.cpp defines it, the generators behind it and the cl_go_* ABI
// functions; a cl_sim holds one DelaySource by value and sees the rows through rows() only.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "cl_dev.h"

namespace clsnap {

struct SimDevice;  // cl_host.h

// Go's rand.Intn(5) streams as a [n][draws] plane: row i from seeds[i], or from seed_base + i
// (wrapping) without a list.  The sequential generator, on up to 16 host threads.
void go_schedule(int64_t seed_base, const int64_t* seeds, int64_t n, int64_t draws, uint8_t* out);

// The rows resident on the device: [n_inst][row] bytes at d, of which the first `draws` of every
// row are valid (draws < 0: none resident).  gen advances with every rewrite of the plane: what
// was derived from the rows (the packed rows of a lanes replay) holds for one gen.
struct DelayRows {
  const uint8_t* d;
  int64_t draws, row, gen;
};

// One run of the device generator, or (device_ms and patched 0) of the host generator.
struct DeviceGen {
  double device_ms = 0, host_ms = 0;
  int64_t patched = 0;
  bool overflow = false;  // more flagged rows than the list holds: nothing was patched
};

class DelaySource {
 public:
  // Each setter drops the resident rows (rows().draws == -1 until the next ensure).
  void set_go_seeds(int64_t seed_base);  // drops a seed list
  void set_seed_list(const int64_t* seeds, int64_t n);
  void set_schedule(const uint8_t* delays, int64_t draws, int64_t n_inst);  // drops a seed list
  bool set_generator(int32_t mode) {     // false: already that mode, nothing dropped
    if (mode == delaygen_) return false;
    delaygen_ = mode;
    draws_ = -1;  // the next launch generates the rows again, with this generator
    return true;
  }

  // Row length of rows for a program that draws `draws_needed` delays: whole 16-byte groups, at
  // least one (a schedule has its own length, of at least one draw).
  int64_t row_for(int64_t draws_needed) const {
    const int64_t d = go_seeds_ ? draws_needed : user_draws_;
    return std::max<int64_t>(16, (d + 15) / 16 * 16);
  }
  // ... and the valid draws of those rows, as rows().draws has them after ensure(need).
  int64_t draws_for(int64_t draws_needed) const { return go_seeds_ ? row_for(draws_needed) : user_draws_; }
  // Makes rows for `need` draws resident, on dev.stream.  *rewritten: the plane was (or was about
  // to be) written, so what the caller derived from the old rows is void.
  int ensure(const SimDevice& dev, int64_t n_inst, int64_t need, bool* rewritten);
  DelayRows rows() const { return DelayRows{plane_.p, draws_, row_, gen_}; }

  // CL_DELAYGEN_* of the resident Go rows, -1 without any
  int32_t generator_used() const { return go_seeds_ && draws_ >= 0 ? dev_gen_ : -1; }
  // The latest generation of Go rows; CL_E_STATE before any.  Any output may be null.
  int gen_time(double* device_ms, double* host_ms, int64_t* patched) const {
    if (!timed_) return set_err(CL_E_STATE, "no delay generation has run");
    if (device_ms) *device_ms = last_.device_ms;
    if (host_ms) *host_ms = last_.host_ms;
    if (patched) *patched = last_.patched;
    return CL_OK;
  }
  // the rows, the seed list and the generator's flagged-row list
  int64_t device_bytes() const { return (int64_t)(plane_.n + d_seeds_.n * 8 + d_flag_.n * 8); }

 private:
  // The only code that changes the plane's contents or address (cl_delays.cpp).
  int rewrite(const SimDevice& dev, int64_t n_inst, int64_t row, int64_t draws, const uint8_t* host, bool* done);
  int device_fill(const SimDevice& dev, int64_t n_inst, int64_t D, bool* done);
  void drop_seed_list();

  bool go_seeds_ = true;
  int64_t seed_base_ = 8053172852482175524LL;  // snapshot_test.go:9,20 (seed + 1)
  std::vector<uint8_t> user_sched_;
  int64_t user_draws_ = 0;
  // Go streams: which generator makes the rows (cl_set_delay_generator) and which made the rows
  // now on the device; per-instance seeds (cl_set_delay_go_seed_list) replace seed_base + i.  The
  // list lives on the host until the device generator first needs it, then in d_seeds_ only (the
  // host generator fetches it back).
  int32_t delaygen_ = CL_DELAYGEN_HOST;
  int32_t dev_gen_ = -1;
  bool seed_list_ = false, seeds_on_dev_ = false;
  std::vector<int64_t> h_seeds_;
  bool timed_ = false;  // a generation has run: last_ holds the three figures of gen_time
  DeviceGen last_;

  int device_ = 0;        // the device of the latest ensure: where d_seeds_ lives
  DevBuf<uint8_t> plane_;
  int64_t draws_ = -1;    // valid draws per instance of the rows in plane_
  int64_t row_ = 0;       // their row stride
  int64_t gen_ = 0;
  DevBuf<long long> d_seeds_;            // [n_inst] the seed list, once the device generator ran with it
  DevBuf<unsigned long long> d_flag_;    // device generator: count, then the rows that met a rejection
  DevTimer<2> tm_;
};

}  // namespace clsnap
