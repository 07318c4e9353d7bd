// cl_gorand.hip -- the Go delay streams of a batch, generated in device memory.
//
// Writes the uint8 [n_inst][row] schedule plane the exec kernels read (cl_host.cpp ensure_delays):
// byte d of row i is the d-th rand.Intn(5) of rand.Seed(seed of instance i), from the closed form of
// cl_gorand.h.  No lane holds generator state: an output is six modular multiplications by
// table constants (two state words) or the sum of two earlier outputs.
//
// Tables.  rngCooked (607 x 8 B) and the 1,821 powers of 48271 (4 B each) are staged in LDS once per
// workgroup; the grid is a few workgroups per CU that stride over the plane.
//
// Rows of at most 273 bytes (cl_delaygen_flat): every output depends on the seed alone.  The plane
// is one flat array of dwords (rows are contiguous, row % 4 == 0); thread t of the grid computes
// dword g = t, t + threads, ...: instance g / (row / 4), outputs 4 (g % (row / 4)) + 1 .. + 4, and
// stores the four delays packed, so a wave's stores are 256 contiguous bytes.
//
// Longer rows (cl_delaygen_rows): one wave per instance, the instance's outputs o_1 .. o_row in
// LDS.  Outputs are computed in blocks of 273 (each reads the block before it and the state words or
// the block 607 places back), the waves of a workgroup in step, a barrier between blocks; then
// every lane packs four consecutive outputs into one dword, again contiguous over the wave.
//
// Rejections (cl_gorand.h intn5): a lane that meets one among the row's first `draws` outputs
// appends the instance to the flagged list (the long-row kernel once per row; the flat kernel once
// per dword that met one, the host removes the duplicates); the host regenerates those rows
// sequentially.
#include <hip/hip_runtime.h>

#include <mutex>

#include "cl_gorand.h"

namespace clsnap {
namespace gorand {
namespace {

struct Tables {
  const unsigned long long* cooked;  // [kLen]
  const uint32_t* pw;                // [kPowN]
};

// (the dynamic LDS region starts with the tables: 8-byte words first)
__device__ __forceinline__ Tables stage_tables(unsigned char* lds, const void* src) {
  uint32_t* d = reinterpret_cast<uint32_t*>(lds);
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  for (int32_t i = threadIdx.x; i < kDelayGenTableBytes / 4; i += kDelayGenThreads) d[i] = s[i];
  __syncthreads();
  Tables t;
  t.cooked = reinterpret_cast<const unsigned long long*>(lds);
  t.pw = reinterpret_cast<const uint32_t*>(lds + kLen * 8);
  return t;
}

__device__ __forceinline__ uint32_t seed_x0(const DelayGenParams& p, long long inst) {
  const long long seed = p.seeds ? p.seeds[inst] : (long long)((unsigned long long)p.seed_base + (unsigned long long)inst);
  return norm_seed(seed);
}

__device__ __forceinline__ void flag_instance(const DelayGenParams& p, long long inst) {
  const unsigned long long at = atomicAdd(p.flagged, 1ull);
  if (at < (unsigned long long)p.flag_cap) p.flagged[1 + at] = (unsigned long long)inst;
}

__global__ __launch_bounds__(kDelayGenThreads) void cl_delaygen_flat(DelayGenParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dg_lds[];
  const Tables t = stage_tables(dg_lds, p.tables);
  const uint32_t dpr = (uint32_t)p.row >> 2;                   // dwords per row
  const uint32_t total = (uint32_t)p.n_inst * dpr;              // (< 2^31: launch_delaygen)
  uint32_t* plane = reinterpret_cast<uint32_t*>(p.plane);
  for (uint32_t g = blockIdx.x * kDelayGenThreads + threadIdx.x; g < total; g += gridDim.x * kDelayGenThreads) {
    const uint32_t inst = g / dpr, k0 = (g - inst * dpr) * 4u;
    const uint32_t x0 = seed_x0(p, inst);
    uint32_t w = 0;
    bool rej = false;
#pragma unroll
    for (int32_t j = 0; j < 4; ++j) {
      const int32_t k = (int32_t)k0 + j + 1;  // <= row <= 273
      bool r = false;
      const uint32_t d = intn5(output(x0, k, t.pw, t.cooked, NoPrev{}), &r);
      w |= d << (8 * j);
      rej |= r && k <= p.draws;
    }
    plane[g] = w;
    if (rej) flag_instance(p, inst);
  }
}

__global__ __launch_bounds__(kDelayGenThreads) void cl_delaygen_rows(DelayGenParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dg_lds[];
  const Tables t = stage_tables(dg_lds, p.tables);
  constexpr int32_t kWaves = kDelayGenThreads / 64;
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t row = p.row, dpr = row >> 2;
  // o[k] = k-th output of this wave's instance, k in [1, row]
  unsigned long long* o =
      reinterpret_cast<unsigned long long*>(dg_lds + (kDelayGenTableBytes + 15) / 16 * 16) + (size_t)wave * (row + 1);
  const long long tiles = (p.n_inst + kWaves - 1) / kWaves;
  // (every loop bound below is uniform over the workgroup: the barriers are reached by all waves)
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long inst = tile * kWaves + wave;
    const bool live = inst < p.n_inst;
    const uint32_t x0 = seed_x0(p, live ? inst : p.n_inst - 1);
    for (int32_t b0 = 0; b0 < row; b0 += kTap) {
      const int32_t hi = b0 + kTap < row ? b0 + kTap : row;
      for (int32_t k = b0 + 1 + lane; k <= hi; k += 64) o[k] = output(x0, k, t.pw, t.cooked, o);
      __syncthreads();
    }
    if (live) {
      uint32_t* out = reinterpret_cast<uint32_t*>(p.plane + (size_t)inst * (size_t)row);
      bool rej = false;
      for (int32_t dw = lane; dw < dpr; dw += 64) {
        uint32_t w = 0;
#pragma unroll
        for (int32_t j = 0; j < 4; ++j) {
          const int32_t k = 4 * dw + j + 1;
          bool r = false;
          w |= intn5(o[k], &r) << (8 * j);
          rej |= r && k <= p.draws;
        }
        out[dw] = w;
      }
      // (`live` is uniform over the wave: one entry per row, whichever lanes met the rejection)
      if (__ballot(rej) != 0ull && lane == 0) flag_instance(p, inst);
    }
    __syncthreads();  // (the next tile overwrites o)
  }
}

constexpr int kMaxDevices = 64;
std::mutex g_tab_mu;
void* g_tab[kMaxDevices] = {};

}  // namespace

int delaygen_tables(int device, const void** tables) {
  if (device < 0 || device >= kMaxDevices) return (int)hipErrorInvalidDevice;
  std::lock_guard<std::mutex> lk(g_tab_mu);
  if (!g_tab[device]) {
    static unsigned char host[kDelayGenTableBytes];
    static bool built = false;
    if (!built) {
      for (int32_t i = 0; i < kLen; ++i) reinterpret_cast<int64_t*>(host)[i] = kRngCooked[i];
      build_pow_table(reinterpret_cast<uint32_t*>(host + kLen * 8));
      built = true;
    }
    hipError_t e = hipSetDevice(device);
    void* d = nullptr;
    if (e == hipSuccess) e = hipMalloc(&d, kDelayGenTableBytes);
    if (e == hipSuccess) e = hipMemcpy(d, host, kDelayGenTableBytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      if (d) (void)hipFree(d);
      return (int)e;
    }
    g_tab[device] = d;
  }
  *tables = g_tab[device];
  return (int)hipSuccess;
}

int launch_delaygen(const DelayGenParams& p, int32_t n_cus, void* stream) {
  if (p.n_inst < 1 || p.row < 4 || (p.row & 3) || p.draws < 0 || p.draws > p.row || !p.plane || !p.flagged || !p.tables ||
      p.flag_cap < 0 || p.n_inst * (long long)(p.row >> 2) >= (1ll << 31))
    return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)delaygen_lds_bytes(p.row);
  if (lds > 160u * 1024u) return (int)hipErrorInvalidValue;
  if (n_cus < 1) n_cus = 256;
  if (p.row <= kTap) {
    const long long need = (p.n_inst * (p.row >> 2) + kDelayGenThreads - 1) / kDelayGenThreads;
    const unsigned blocks = (unsigned)(need < (long long)n_cus * 8 ? need : (long long)n_cus * 8);
    hipLaunchKernelGGL(cl_delaygen_flat, dim3(blocks), dim3(kDelayGenThreads), lds, (hipStream_t)stream, p);
  } else {
    if (lds > 64u * 1024u) {
      hipError_t e = hipFuncSetAttribute((const void*)cl_delaygen_rows, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         160 * 1024);
      if (e != hipSuccess) return (int)e;
    }
    const long long need = (p.n_inst + kDelayGenThreads / 64 - 1) / (kDelayGenThreads / 64);
    const long long per_cu = (long long)(160u * 1024u / lds) < 8 ? (long long)(160u * 1024u / lds) : 8;
    const long long cap = (long long)n_cus * (per_cu < 1 ? 1 : per_cu);
    const unsigned blocks = (unsigned)(need < cap ? need : cap);
    hipLaunchKernelGGL(cl_delaygen_rows, dim3(blocks), dim3(kDelayGenThreads), lds, (hipStream_t)stream, p);
  }
  return (int)hipGetLastError();
}

}  // namespace gorand
}  // namespace clsnap
