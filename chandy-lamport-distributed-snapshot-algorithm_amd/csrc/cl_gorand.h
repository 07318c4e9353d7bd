// cl_gorand.h -- Go math/rand (Go 1.22 rngSource, rng.go) in closed form, for host and device.
//
// The engine replays rand.Intn(5) of rand.Seed(seed) per instance.  The sequential generator
// (cl_delays.cpp GoRand) seeds a 607-word state with 1,841 Lehmer steps and then runs an additive
// lagged Fibonacci recurrence over it.  Both parts have a form that needs no sequential state:
//
//   seeding  seedrand is Schrage's form of x <- 48271 x mod M, M = 2^31 - 1, so the n-th x after the
//            normalised seed x0 is 48271^n x0 mod M: one modular multiplication by a constant of
//            the power table.  State word i is
//              vec0[i] = (x_{21+3i} << 40) ^ (x_{22+3i} << 20) ^ x_{23+3i} ^ rngCooked[i]
//   outputs  the k-th Uint64(), k >= 1, is o_k = a(k) + b(k) (mod 2^64) with
//              a(k) = vec0[(334 - k) mod 607]  for k <= 607, else o_{k-607}
//              b(k) = vec0[607 - k]            for k <= 273, else o_{k-273}
//            (feed starts at 334 and tap at 0, both step down by one per call; the word at feed was
//            last written 607 calls ago, the word at tap 273 calls ago).  The first 273 outputs of
//            a stream depend on the seed alone; later ones on outputs 273 and 607 places earlier.
//   Intn(5)  v = (o_k & 2^63-1) >> 32; Go rejects v > 2^31 - 1 - (2^31 mod 5) = 2147483644 and draws
//            again, which shifts every later draw of the stream by one output.  intn5() reports
//            the rejection; the callers regenerate such a row with the sequential generator.
//
// The kernel (cl_gorand.hip) and the host evaluation (cl_go_delay_schedule_jump) are both written
// over the functions below.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CLGR_HD __host__ __device__
#else
#define CLGR_HD
#endif

namespace clsnap {
namespace gorand {

constexpr int32_t kLen = 607;        // rngLen
constexpr int32_t kTap = 273;        // rngTap
constexpr int32_t kFeed0 = kLen - kTap;  // 334: feed before the first call
constexpr uint32_t kM = 2147483647u; // 2^31 - 1
constexpr uint32_t kA = 48271u;
constexpr int32_t kPowFirst = 21;    // x_21 is the first Lehmer value that enters the state
constexpr int32_t kPowN = 3 * kLen;  // 1,821 powers: 48271^21 .. 48271^1841
constexpr uint32_t kIntn5Max = 2147483644u;  // Int31n(5): largest accepted v

// rngCooked (rng.go), regenerated offline by oracle/gen_go_rng_cooked.py (KAT-pinned)
static const int64_t kRngCooked[kLen] = {
#include "go_rng_cooked.inc"
};

// seed -> x0 as rngSource.Seed does: seed mod M, made positive, 0 replaced
CLGR_HD inline uint32_t norm_seed(int64_t seed) {
  seed %= (int64_t)kM;
  if (seed < 0) seed += (int64_t)kM;
  if (seed == 0) seed = 89482311;
  return (uint32_t)seed;
}

// a * b mod M for a, b < 2^31: the product is < 2^62, reduced by the Mersenne fold (2^31 = 1 mod M)
CLGR_HD inline uint32_t mulmod(uint32_t a, uint32_t b) {
  const uint64_t p = (uint64_t)a * (uint64_t)b;
  uint64_t r = (p & kM) + (p >> 31);  // < 2^32
  r = (r & kM) + (r >> 31);           // <= 2^31
  return (uint32_t)(r >= kM ? r - kM : r);
}

// pw[j] = 48271^(kPowFirst + j) mod M, j < kPowN.  Host: built once, then staged where it is used.
inline void build_pow_table(uint32_t* pw) {
  uint32_t x = 1;
  for (int32_t n = 0; n < kPowFirst; ++n) x = mulmod(x, kA);
  for (int32_t j = 0; j < kPowN; ++j) {
    pw[j] = x;
    x = mulmod(x, kA);
  }
}

// state word i of the freshly seeded generator
template <class Pow, class Cooked>
CLGR_HD inline uint64_t vec0(uint32_t x0, int32_t i, Pow pw, Cooked cooked) {
  const uint64_t x1 = mulmod(x0, pw[3 * i]), x2 = mulmod(x0, pw[3 * i + 1]), x3 = mulmod(x0, pw[3 * i + 2]);
  return ((x1 << 40) ^ (x2 << 20) ^ x3) ^ (uint64_t)cooked[i];
}

// the k-th Uint64() of the stream, k >= 1; prev[j] = o_j must hold for j = k - 273 and k - 607
// where those are >= 1 (never read for k <= 273)
template <class Pow, class Cooked, class Prev>
CLGR_HD inline uint64_t output(uint32_t x0, int32_t k, Pow pw, Cooked cooked, Prev prev) {
  const uint64_t a = k <= kLen ? vec0(x0, k <= kFeed0 ? kFeed0 - k : kFeed0 + kLen - k, pw, cooked) : prev[k - kLen];
  const uint64_t b = k <= kTap ? vec0(x0, kLen - k, pw, cooked) : prev[k - kTap];
  return a + b;
}

// `prev` of a caller that stays within the first 273 outputs
struct NoPrev {
  CLGR_HD uint64_t operator[](int32_t) const { return 0; }
};

// rand.Intn(5) of one output where Go accepts it; *reject |= Go would draw again
CLGR_HD inline uint32_t intn5(uint64_t o, bool* reject) {
  const uint32_t v = (uint32_t)(o >> 32) & 0x7fffffffu;
  if (v > kIntn5Max) *reject = true;
  return v % 5u;
}

// ---- the device generator (cl_gorand.hip) ----------------------------------------------------
// plane[i * row + d], d < draws: the d-th delay of instance i, drawn from seeds[i] (seeds a device
// array) or from seed_base + i (seeds == nullptr).  row is a multiple of 4, draws <= row; bytes
// [draws, row) of a row are written too (further outputs of the stream).  An instance that met a
// rejection among its first `draws` outputs is appended to flagged[1 ..] (flagged[0] counts them,
// duplicates included, also beyond flag_cap entries; zeroed by the caller).
constexpr int32_t kDelayGenThreads = 256;
constexpr int32_t kDelayGenFlagCap = 4096;
struct DelayGenParams {
  uint8_t* plane;
  const long long* seeds;
  long long seed_base;
  long long n_inst;
  int32_t row, draws;
  unsigned long long* flagged;  // [1 + flag_cap]
  int32_t flag_cap;
  const void* tables;           // delaygen_tables
};
constexpr int32_t kDelayGenTableBytes = kLen * 8 + kPowN * 4;  // rngCooked, then the powers
// The device copy of rngCooked and the power table on `device` (built and uploaded once per
// process and device, never freed).  Returns a hipError_t.
int delaygen_tables(int device, const void** tables);
// LDS bytes of a workgroup for rows of `row` bytes; rows above the no-communication range keep
// one instance's outputs per wave.
inline int32_t delaygen_lds_bytes(int32_t row) {
  const int32_t tab = (kDelayGenTableBytes + 15) / 16 * 16;
  return row <= kTap ? tab : tab + (kDelayGenThreads / 64) * (row + 1) * 8;
}
// Returns a hipError_t; hipErrorInvalidValue for a shape outside the kernel's range.
int launch_delaygen(const DelayGenParams& p, int32_t n_cus, void* stream);

}  // namespace gorand
}  // namespace clsnap
