// cloud_src.h — a cloud as one stage hands it to the next (processor -> scan-to-scan odometry -> scan-to-map -> estimator push): n points
// x y z i, and whether they lie in host or in device memory.  The place travels with the pointer: a copy takes its kind from to_device(),
// a kernel record takes p only from a device source, which is complete and left alone until the call it is given to returns.  Host code only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <stdexcept>

namespace lio {

struct CloudSrc {
  const float4 *p = nullptr; size_t n = 0; bool on_device = false;
  // the one place a host float * (four floats per point) becomes a float4 *; (nullptr, 0) is the empty cloud
  static CloudSrc host(const float *xyzi, size_t n) { return CloudSrc{reinterpret_cast<const float4 *>(xyzi), n, false}; }
  static CloudSrc device(const float4 *p, size_t n) { return CloudSrc{p, n, true}; }
  static CloudSrc at(const float *xyzi, size_t n, bool on_device) { return CloudSrc{host(xyzi, n).p, n, on_device}; }   // the C-ABI's float *, either place
  hipMemcpyKind to_device() const { return on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice; }   // of a copy into device memory
};

// Whether the clouds get(0) .. get(n - 1) of a call are all the device's (true) or all the host's (false; also for no cloud at all).  A launch
// chain takes its clouds one way per call — one take launch that reads them where they lie, or an upload per cloud; a mix is the caller's
// mistake (no entry point of the C-ABI can build one) and throws.
template <class Get> inline bool clouds_on_device(size_t n, Get get) {
  const bool dev = n != 0 && get(size_t(0)).on_device;
  for (size_t i = 1; i < n; ++i)
    if (get(i).on_device != dev) throw std::logic_error("CloudSrc: a call's clouds lie partly in host and partly in device memory");
  return dev;
}
inline bool clouds_on_device(const CloudSrc *c, size_t n) { return clouds_on_device(n, [c](size_t i) { return c[i]; }); }

}  // namespace lio
