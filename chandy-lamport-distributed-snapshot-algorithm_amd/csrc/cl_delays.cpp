// cl_delays.cpp -- the delay source of a batch (cl_delays.h): the reference's rand.Intn(5)
// (sim.go:101) replayed from a per-instance schedule, by default Go's own math/rand stream for
// seed_base + i, restated here; the device generator's host half (cl_gorand.hip); the owner of the
// rows on the device; and the cl_go_* ABI functions, which take no sim.
#include "cl_delays.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>

#include "cl_gorand.h"
#include "cl_host.h"

namespace clsnap {
namespace {

// ---------------------------------------------------------------------------
// Go math/rand (Go 1.22, go.mod:3): rngSource seeded as in rng.go, Intn -> Int31n.
// rngCooked (cl_gorand.h) is regenerated offline by oracle/gen_go_rng_cooked.py (KAT-pinned).
// ---------------------------------------------------------------------------
using gorand::kRngCooked;

struct GoRand {
  int tap = 0, feed = 334;
  uint64_t vec[607];

  static int32_t seedrand(int32_t x) {
    const int32_t hi = x / 44488, lo = x % 44488;
    x = 48271 * lo - 3399 * hi;
    if (x < 0) x += 2147483647;
    return x;
  }
  explicit GoRand(int64_t seed) {
    seed %= 2147483647LL;
    if (seed < 0) seed += 2147483647LL;
    if (seed == 0) seed = 89482311;
    int32_t x = (int32_t)seed;
    for (int i = -20; i < 607; ++i) {
      x = seedrand(x);
      if (i >= 0) {
        uint64_t u = (uint64_t)(int64_t)x << 40;
        x = seedrand(x);
        u ^= (uint64_t)(int64_t)x << 20;
        x = seedrand(x);
        u ^= (uint64_t)(int64_t)x;
        vec[i] = u ^ (uint64_t)kRngCooked[i];
      }
    }
  }
  uint64_t uint64() {
    if (--tap < 0) tap += 607;
    if (--feed < 0) feed += 607;
    vec[feed] += vec[tap];
    return vec[feed];
  }
  int64_t int63() { return (int64_t)(uint64() & 0x7fffffffffffffffULL); }
  int32_t int31() { return (int32_t)(int63() >> 32); }
  int32_t int31n(int32_t n) {
    if ((n & (n - 1)) == 0) return int31() & (n - 1);
    const int32_t max = (int32_t)((1LL << 31) - 1 - (int64_t)((1ULL << 31) % (uint32_t)n));
    int32_t v = int31();
    while (v > max) v = int31();
    return v % n;
  }
};

int host_threads() {
  unsigned n = std::thread::hardware_concurrency();
  if (n == 0) n = 1;
  return (int)std::min(n, 16u);  // the GPU box grants 16 host cores per GPU
}

// seed of instance i: seeds[i], or seed_base + i (wrapping) without a list
inline int64_t seed_of(int64_t seed_base, const int64_t* seeds, int64_t i) {
  return seeds ? seeds[i] : (int64_t)((uint64_t)seed_base + (uint64_t)i);
}

void go_row(int64_t seed, int64_t draws, uint8_t* o) {
  GoRand r(seed);
  for (int64_t k = 0; k < draws; ++k) o[k] = (uint8_t)r.int31n(5);  // rand.Intn(maxDelay)
}

// The same plane from the closed form of cl_gorand.h, row by row as the device generator computes
// it; a row that met a rejection is regenerated sequentially.  Returns the number of such rows.
int64_t go_schedule_jump(int64_t seed_base, const int64_t* seeds, int64_t n, int64_t draws, uint8_t* out) {
  static const std::vector<uint32_t> pw = [] {
    std::vector<uint32_t> t(gorand::kPowN);
    gorand::build_pow_table(t.data());
    return t;
  }();
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), (n + 255) / 256));
  std::atomic<int64_t> rejected{0};
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) {
    th.emplace_back([=, &rejected] {
      std::vector<uint64_t> o((size_t)draws + 1);
      for (int64_t i = n * t / T; i < n * (t + 1) / T; ++i) {
        const int64_t seed = seed_of(seed_base, seeds, i);
        const uint32_t x0 = gorand::norm_seed(seed);
        uint8_t* row = out + i * draws;
        bool rej = false;
        for (int64_t k = 1; k <= draws; ++k) {
          o[(size_t)k] = gorand::output(x0, (int32_t)k, pw.data(), kRngCooked, o.data());
          row[k - 1] = (uint8_t)gorand::intn5(o[(size_t)k], &rej);
        }
        if (rej) {
          go_row(seed, draws, row);
          ++rejected;
        }
      }
    });
  }
  for (auto& x : th) x.join();
  return rejected.load();
}

// ---- the device generator (cl_gorand.hip) and its host-side patching ---------------------------
// Shapes it takes: rows up to the documented cap, a plane of fewer than 2^31 dwords.
bool delaygen_fits(int64_t n, int64_t row) {
  return n >= 1 && row >= 4 && row <= CL_DELAYGEN_MAX_DRAWS && n * (row / 4) < (1ll << 31);
}

// Generate the [n][row] plane at d_plane on `stream` (seeds: d_seeds, a device array, or
// seed_base + i), wait, and regenerate the rows that met a rejection among their first `draws`
// outputs with the sequential generator.  d_flag has 1 + kDelayGenFlagCap words; `tm` times the kernel.
int device_generate(int device, hipStream_t stream, int32_t n_cus, int64_t seed_base, const long long* d_seeds,
                    int64_t n, int64_t row, int64_t draws, uint8_t* d_plane, unsigned long long* d_flag,
                    DevTimer<2>* tm, DeviceGen* g) {
  const void* tables = nullptr;
  int e = gorand::delaygen_tables(device, &tables);
  if (e) return set_err(CL_E_DEVICE, "delay generator tables: %s", hipGetErrorString((hipError_t)e));
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(unsigned long long), stream));
  gorand::DelayGenParams p{};
  p.plane = d_plane;
  p.seeds = d_seeds;
  p.seed_base = seed_base;
  p.n_inst = n;
  p.row = (int32_t)row;
  p.draws = (int32_t)draws;
  p.flagged = d_flag;
  p.flag_cap = gorand::kDelayGenFlagCap;
  p.tables = tables;
  if (int rc = tm->mark(0, stream)) return rc;
  e = gorand::launch_delaygen(p, n_cus, stream);
  if (e) return set_err(CL_E_DEVICE, "delay generator launch failed: %s", hipGetErrorString((hipError_t)e));
  if (int rc = tm->mark(1, stream)) return rc;
  unsigned long long cnt = 0;
  HIP_TRY(hipMemcpyAsync(&cnt, d_flag, sizeof cnt, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  const auto t0 = std::chrono::steady_clock::now();
  *g = DeviceGen{};
  if (cnt > (unsigned long long)gorand::kDelayGenFlagCap) {
    g->overflow = true;
  } else if (cnt) {
    std::vector<unsigned long long> rows((size_t)cnt);
    HIP_TRY(hipMemcpy(rows.data(), d_flag + 1, (size_t)cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    std::vector<uint8_t> buf((size_t)row);
    for (unsigned long long i : rows) {
      if (i >= (unsigned long long)n) return set_err(CL_E_DEVICE, "delay generator flagged row %llu of %lld", i, (long long)n);
      long long seed = (long long)((uint64_t)seed_base + (uint64_t)i);
      if (d_seeds) HIP_TRY(hipMemcpy(&seed, d_seeds + i, sizeof seed, hipMemcpyDeviceToHost));
      go_row((int64_t)seed, row, buf.data());
      HIP_TRY(hipMemcpy(d_plane + (size_t)i * (size_t)row, buf.data(), (size_t)row, hipMemcpyHostToDevice));
    }
    g->patched = (int64_t)rows.size();
  }
  g->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return tm->ms(0, 1, &g->device_ms);
}

}  // namespace

void go_schedule(int64_t seed_base, const int64_t* seeds, int64_t n, int64_t draws, uint8_t* out) {
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), (n + 255) / 256));
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) {
    th.emplace_back([=] {
      for (int64_t i = n * t / T; i < n * (t + 1) / T; ++i) go_row(seed_of(seed_base, seeds, i), draws, out + i * draws);
    });
  }
  for (auto& x : th) x.join();
}

// ---- DelaySource -------------------------------------------------------------------------------
// (the generator's kernel has finished whenever an ABI call returns: nothing reads d_seeds_ then)
void DelaySource::drop_seed_list() {
  seed_list_ = seeds_on_dev_ = false;
  std::vector<int64_t>().swap(h_seeds_);
  if (d_seeds_.p) {
    (void)hipSetDevice(device_);
    d_seeds_.release();
  }
}

void DelaySource::set_go_seeds(int64_t seed_base) {
  go_seeds_ = true;
  seed_base_ = seed_base;
  drop_seed_list();
  draws_ = -1;
}

void DelaySource::set_seed_list(const int64_t* seeds, int64_t n) {
  drop_seed_list();
  h_seeds_.assign(seeds, seeds + n);
  seed_list_ = go_seeds_ = true;
  draws_ = -1;
}

void DelaySource::set_schedule(const uint8_t* delays, int64_t draws, int64_t n_inst) {
  user_sched_.assign(delays, delays + (size_t)(draws * n_inst));
  user_draws_ = draws;
  go_seeds_ = false;
  drop_seed_list();
  draws_ = -1;
}

// The only code that changes the plane's contents or address: [n_inst] rows of `row` bytes, `draws`
// of them valid, copied from `host` or (host null; *done as from device_fill) made by the device
// generator.  No rows are valid from before the first byte changes until the new rows are complete.
int DelaySource::rewrite(const SimDevice& dev, int64_t n_inst, int64_t row, int64_t draws, const uint8_t* host,
                         bool* done) {
  HIP_TRY(hipStreamSynchronize(dev.stream));  // (an async launch may read the plane)
  draws_ = -1;
  gen_ += 1;
  const size_t bytes = (size_t)(row * n_inst);
  int rc = plane_.ensure(bytes);
  if (rc) return rc;
  if (host) {
    HIP_TRY(hipMemcpy(plane_.p, host, bytes, hipMemcpyHostToDevice));
  } else if ((rc = device_fill(dev, n_inst, row, done)) || !*done) {
    return rc;
  }
  draws_ = draws;
  row_ = row;
  return CL_OK;
}

// Rows of D draws from the device generator, on the sim's stream, straight into the plane.  *done =
// false when more rows met a rejection than its list holds (ensure then takes the host generator).
int DelaySource::device_fill(const SimDevice& dev, int64_t n_inst, int64_t D, bool* done) {
  int rc;
  if ((rc = d_flag_.ensure(1 + (size_t)gorand::kDelayGenFlagCap))) return rc;
  if (seed_list_ && !seeds_on_dev_) {
    if ((rc = d_seeds_.ensure((size_t)n_inst))) return rc;
    HIP_TRY(hipMemcpy(d_seeds_.p, h_seeds_.data(), (size_t)n_inst * sizeof(int64_t), hipMemcpyHostToDevice));
    std::vector<int64_t>().swap(h_seeds_);
    seeds_on_dev_ = true;
  }
  DeviceGen g;
  if ((rc = device_generate(dev.device, dev.stream, dev.n_cus, seed_base_, seed_list_ ? d_seeds_.p : nullptr, n_inst, D,
                            D, plane_.p, d_flag_.p, &tm_, &g)))
    return rc;
  *done = !g.overflow;
  if (g.overflow) return CL_OK;
  last_ = g;
  timed_ = true;
  dev_gen_ = CL_DELAYGEN_DEVICE;
  return CL_OK;
}

int DelaySource::ensure(const SimDevice& dev, int64_t n_inst, int64_t need, bool* rewritten) {
  *rewritten = false;
  device_ = dev.device;
  const int64_t row = row_for(need);
  // (Go rows: longer rows of the same streams serve too, saved draw cursors stay valid)
  if (go_seeds_ ? draws_ >= row : draws_ == user_draws_) return CL_OK;
  *rewritten = true;
  if (!go_seeds_) {
    std::vector<uint8_t> padded((size_t)(row * n_inst), 0);
    for (int64_t i = 0; i < n_inst; ++i)
      std::memcpy(&padded[(size_t)(i * row)], &user_sched_[(size_t)(i * user_draws_)], (size_t)user_draws_);
    return rewrite(dev, n_inst, row, user_draws_, padded.data(), nullptr);
  }
  bool on_device = delaygen_ == CL_DELAYGEN_DEVICE && delaygen_fits(n_inst, row);
  if (on_device)
    if (int rc = rewrite(dev, n_inst, row, row, nullptr, &on_device)) return rc;
  if (on_device) return CL_OK;
  const auto t0 = std::chrono::steady_clock::now();
  if (seed_list_ && seeds_on_dev_) {  // (the list goes back to the host generator's side)
    h_seeds_.resize((size_t)n_inst);
    HIP_TRY(hipMemcpy(h_seeds_.data(), d_seeds_.p, (size_t)n_inst * sizeof(int64_t), hipMemcpyDeviceToHost));
    d_seeds_.release();
    seeds_on_dev_ = false;
  }
  std::vector<uint8_t> sched((size_t)(row * n_inst));
  go_schedule(seed_base_, seed_list_ ? h_seeds_.data() : nullptr, n_inst, row, sched.data());
  if (int rc = rewrite(dev, n_inst, row, row, sched.data(), nullptr)) return rc;
  last_ = DeviceGen{0, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), 0, false};
  timed_ = true;
  dev_gen_ = CL_DELAYGEN_HOST;
  return CL_OK;
}

}  // namespace clsnap

// ---- C ABI: the generators on their own ----------------------------------------------------------
using namespace clsnap;

extern "C" {

int cl_go_delay_schedule(int64_t seed_base, int64_t n, int64_t draws, uint8_t* out) {
  if (!out || n < 0 || draws < 0) return set_err(CL_E_INVALID, "bad arguments");
  go_schedule(seed_base, nullptr, n, draws, out);
  return CL_OK;
}

int cl_go_delay_schedule_jump(int64_t seed_base, const int64_t* seeds, int64_t n, int64_t draws, uint8_t* out,
                              int64_t* rejected_rows) {
  if (!out || n < 0 || draws < 0 || draws > (1 << 30)) return set_err(CL_E_INVALID, "bad arguments");
  const int64_t r = go_schedule_jump(seed_base, seeds, n, draws, out);
  if (rejected_rows) *rejected_rows = r;
  return CL_OK;
}

int cl_go_delay_schedule_device(int32_t device, int64_t seed_base, const int64_t* seeds, int64_t n, int64_t draws,
                                uint8_t* out, int64_t* patched_rows, double* device_ms) {
  if (!out || n < 0 || draws < 0) return set_err(CL_E_INVALID, "bad arguments");
  hipDeviceProp_t prop;
  if (int rc = open_gfx950(device, &prop)) return rc;
  if (patched_rows) *patched_rows = 0;
  if (device_ms) *device_ms = 0;
  if (n == 0 || draws == 0) return CL_OK;
  const int64_t row = DelaySource().row_for(draws);  // the engine's row padding (a fresh source is on Go seeds)
  if (!delaygen_fits(n, row)) {  // above the cap: the host generator, as in the engine
    go_schedule(seed_base, seeds, n, draws, out);
    return CL_OK;
  }
  struct Scratch {  // (the buffers and the timer free themselves on every return path)
    DevBuf<uint8_t> plane;
    DevBuf<long long> seeds;
    DevBuf<unsigned long long> flag;
    DevTimer<2> tm;
    hipStream_t stream = nullptr;
    ~Scratch() {
      if (stream) (void)hipStreamDestroy(stream);
    }
  } s;
  int rc;
  if ((rc = s.plane.ensure((size_t)(n * row))) || (rc = s.flag.ensure(1 + (size_t)gorand::kDelayGenFlagCap))) return rc;
  if (seeds) {
    if ((rc = s.seeds.ensure((size_t)n))) return rc;
    HIP_TRY(hipMemcpy(s.seeds.p, seeds, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  DeviceGen g;
  if ((rc = device_generate(device, s.stream, prop.multiProcessorCount, seed_base, seeds ? s.seeds.p : nullptr, n, row,
                            draws, s.plane.p, s.flag.p, &s.tm, &g)))
    return rc;
  if (g.overflow) {  // more flagged rows than the list holds: the host generator, as in the engine
    go_schedule(seed_base, seeds, n, draws, out);
    return CL_OK;
  }
  HIP_TRY(hipMemcpy2D(out, (size_t)draws, s.plane.p, (size_t)row, (size_t)draws, (size_t)n, hipMemcpyDeviceToHost));
  if (patched_rows) *patched_rows = g.patched;
  if (device_ms) *device_ms = g.device_ms;
  return CL_OK;
}

int cl_go_int63(int64_t seed, int64_t n, int64_t* out) {
  if (!out || n < 0) return set_err(CL_E_INVALID, "bad arguments");
  GoRand r(seed);
  for (int64_t i = 0; i < n; ++i) out[i] = r.int63();
  return CL_OK;
}

int cl_go_intn(int64_t seed, int32_t bound, int64_t n, int32_t* out) {
  if (!out || n < 0 || bound <= 0) return set_err(CL_E_INVALID, "bad arguments");
  GoRand r(seed);
  for (int64_t i = 0; i < n; ++i) out[i] = r.int31n(bound);
  return CL_OK;
}

}  // extern "C"

