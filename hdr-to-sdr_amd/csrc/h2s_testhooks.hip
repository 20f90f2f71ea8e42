// h2s_testhooks.hip — private test entries (not in include/h2s.h): host arrays
// in and out, synchronous, on the current device; 0 or a negative HIP error.
// They reach the library through h2s_launch.h and the libm forms (libm_powf /
// libm_expf over h2s_libm.h's tables live in h2s_chain.h; no contraction inside);
// h2stest_decimate alone takes a context, through h2s_host.h's front-end steps
#include <vector>

#include "h2s_chain.h"
#include "h2s_host.h"
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

// the 4:2:0 front-end alone (h2s_set_input_decimation's k_decimate420, whatever the setting) on up
// to 16 device frames of the context's 4:2:2 / 4:4:4 input form, for tests/test_gpu_decimate.py: the
// decimated chroma comes back tight in `out` (host), frame by frame: the planar set's Cb plane then
// its Cr plane, or the semi-planar set's one plane of pairs.  run > 0 forces the kernel's run length.
// Synchronous on the null stream; an H2S_E_* code (h2s_last_error says why)
extern "C" __attribute__((visibility("default"))) int h2stest_decimate(h2s_ctx* c, const h2s_frames* in, int nframes,
                                                                        void* out, int64_t out_bytes, int run) {
  using namespace h2s::host;
  if (!c) return fail(nullptr, H2S_E_INVALID_ARG, "ctx is NULL");
  const Format f = c->in_fmt;
  if (f.sub == H2S_SUB_420 || nframes < 1 || nframes > 16 || !out || !in || in->location != H2S_LOC_DEVICE)
    return fail(c, H2S_E_INVALID_ARG, "h2stest_decimate: 1..16 device frames of a 4:2:2 / 4:4:4 set");
  Decimated d;
  h2s_frames v;
  int rc;
  if ((rc = decimate_begin(c, in, nframes, nullptr, f, &d))) return rc;
  const size_t row = (size_t)(in->width / 2) * 2 * (f.semi() ? 2 : 1), rows = (size_t)in->height / 2;
  const int np = f.semi() ? 1 : 2;
  if ((int64_t)(row * rows * np * nframes) != out_bytes) return fail(c, H2S_E_INVALID_ARG, "h2stest_decimate: out_bytes");
  DeviceGuard g(c->device);
  if ((rc = decimate_chunk(c, d, in, nframes, nullptr, &v, run))) return rc;
  hipError_t e = hipSuccess;
  uint8_t* o = (uint8_t*)out;
  for (int fr = 0; fr < nframes && e == hipSuccess; fr++)
    for (int p = 1; p <= np && e == hipSuccess; p++, o += row * rows)
      e = hipMemcpy2DAsync(o, row, (const uint8_t*)v.data[p] + fr * v.frame_pitch[p], v.linesize[p], row, rows,
                           hipMemcpyDeviceToHost, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  return e == hipSuccess ? 0 : hip_fail(c, e, "h2stest_decimate");
}
