// h2s_testhooks.hip — private test entries (not in include/h2s.h): host arrays
// in and out, synchronous, on the current device; 0 or a negative HIP error.
// They reach the library through h2s_launch.h and the libm forms alone (libm_powf /
// libm_expf over h2s_libm.h's tables live in h2s_chain.h; no contraction inside)
#include <vector>

#include "h2s_chain.h"
#include "h2s_launch.h"

namespace h2s {

// device libm_powf / libm_expf over n inputs (fn 0: powf(x, y), 1: expf(x)),
// for tests/test_libm_tables.py's bit-equality check against the libm the
// oracle links
__global__ void k_test_libm(int fn, const float* x, const float* y, float* out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = fn == 0 ? libm_powf(x[i], y[i]) : libm_expf(x[i]);
}

}  // namespace h2s

extern "C" __attribute__((visibility("default"))) int h2stest_libm(int fn, const float* x, const float* y, float* out,
                                                                    int n) {
  if (n <= 0) return 0;
  float* d = nullptr;
  const size_t b = (size_t)n * sizeof(float);
  if (hipMalloc(&d, 3 * b) != hipSuccess) return -1;
  hipError_t e = hipMemcpy(d, x, b, hipMemcpyHostToDevice);
  if (e == hipSuccess && y) e = hipMemcpy(d + n, y, b, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(h2s::k_test_libm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, d, d + n, d + 2 * n, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d + 2 * n, b, hipMemcpyDeviceToHost);
  hipFree(d);
  return e == hipSuccess ? 0 : -(int)e;
}

// the libplacebo branch's lut3d 8-bit table (k_build_lut8x) for a host lattice of n^3 R'G'B'
// records (3 floats each, r fastest), copied back in the kernel's bit-interleaved order
// (2^24 u32), for tests/test_gpu_parity.py's whole-table comparison with the oracle's
extern "C" __attribute__((visibility("default"))) int h2stest_lut8x(const float* lut_rgb, int n, unsigned* out) {
  if (n < 2 || n > 256) return -1;
  const size_t nn = (size_t)n * n * n;
  std::vector<float4> l4(nn + 1, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  for (size_t i = 0; i < nn; i++) l4[i] = make_float4(lut_rgb[3 * i], lut_rgb[3 * i + 1], lut_rgb[3 * i + 2], 0.0f);
  float4* dl = nullptr;
  unsigned* dt = nullptr;
  if (hipMalloc(&dl, l4.size() * sizeof(float4)) != hipSuccess) return -1;
  if (hipMalloc(&dt, sizeof(unsigned) << 24) != hipSuccess) {
    hipFree(dl);
    return -1;
  }
  hipError_t e = hipMemcpy(dl, l4.data(), l4.size() * sizeof(float4), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = h2s::build_lut8x(dl, n, dt, 0);
  if (e == hipSuccess) e = hipMemcpy(out, dt, sizeof(unsigned) << 24, hipMemcpyDeviceToHost);
  hipFree(dl);
  hipFree(dt);
  return e == hipSuccess ? 0 : -(int)e;
}
