// cl_dev.h -- what every host unit (cl_host.cpp, cl_delays.cpp, cl_analytics.cpp, cg_host.cpp,
// cg_readout.cpp) owns on the device: the error return of a failed HIP call, the one way a device
// is opened, a buffer that frees itself, and a set of timing events that destroy themselves.
// Nothing here orders the frees against work in flight: an owner synchronises its streams in its
// destructor's body, and its members go after that.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <vector>

#include "../../include/clsnap.h"

namespace clsnap {

// Sets the calling thread's cl_last_error() text and returns `code` (defined in cl_host.cpp).
int set_err(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                               \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return clsnap::set_err(CL_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// Makes `device` current and reads its properties; CL_E_DEVICE where there is no device, the
// ordinal is out of range, or the device is not a gfx950 (defined in cl_host.cpp).
int open_gfx950(int device, hipDeviceProp_t* prop);

// n elements of T on the device, grown on demand (the contents do not survive a growth).
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  int ensure(size_t count) {
    if (count <= n && p) return CL_OK;
    release();
    if (count == 0) count = 1;
    HIP_TRY(hipMalloc((void**)&p, count * sizeof(T)));
    n = count;
    return CL_OK;
  }
  int upload(const std::vector<T>& v) {
    int rc = ensure(v.size());
    if (rc) return rc;
    if (!v.empty()) HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return CL_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  size_t bytes() const { return n * sizeof(T); }
};
static_assert(!std::is_copy_constructible<DevBuf<int>>::value, "a DevBuf is never copied: it frees what it holds");

// N timing events of one call, created at the first mark.  `done` is the owner's: how many of the
// marks (or pairs of them) of the latest call completed, 0 while nothing has been timed.
template <int N, unsigned Flags = hipEventDefault>
struct DevTimer {
  hipEvent_t ev[N] = {};
  int done = 0;
  DevTimer() = default;
  DevTimer(const DevTimer&) = delete;
  DevTimer& operator=(const DevTimer&) = delete;
  ~DevTimer() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int mark(int i, hipStream_t stream) {
    for (hipEvent_t& e : ev)
      if (!e) HIP_TRY(hipEventCreateWithFlags(&e, Flags));
    HIP_TRY(hipEventRecord(ev[i], stream));
    return CL_OK;
  }
  // milliseconds from mark i to mark j (both complete: the caller has synchronised the stream)
  int ms(int i, int j, double* out) const {
    float f = 0.f;
    HIP_TRY(hipEventElapsedTime(&f, ev[i], ev[j]));
    *out = f;
    return CL_OK;
  }
};

}  // namespace clsnap
