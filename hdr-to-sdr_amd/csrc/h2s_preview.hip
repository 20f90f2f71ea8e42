// h2s_preview.hip — the preview tail of the chain (src/utils.py:46-49,
// :719-765; src/preview.py:108-117): aspect-fit resize of the 8-bit yuv420p
// the chain produced, Y'CbCr -> RGB24 and the GUI's display gamma.
//
// The preview is latency-bound (a 4K frame is ~25 MB of RGB out), so these
// kernels are plain one-thread-per-output-sample gathers; blockIdx.z is the
// frame of a batch (extract_frames_with_conversion_batch, src/utils.py:668-716:
// N frames, one call); the tone-map work before them runs through k_tile.
//
// k_source_rgb24 is the other pane (extract_frame / extract_frames_batch,
// src/utils.py:827-859, :629-665): the source as decoded, with no tone mapping,
// read in place from the 10/12-bit surfaces and written as RGB24 in one launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "h2s_launch.h"
#include "h2s_srcprev.h"

namespace h2s {

// separable resize of one u8 plane, taps/weights precomputed on the host per
// output column (wx: ow x Tx, start sx) and row (wy: oh x Ty, start sy); source
// indices clamp at the edges (swscale's edge handling)
__global__ void k_resize_u8(const uint8_t* __restrict__ src, int sw, int sh, long long sls, long long sfp,
                            uint8_t* __restrict__ dst, int ow, int oh, long long dls, long long dfp,
                            const float* __restrict__ wx, const int* __restrict__ sx, int Tx,
                            const float* __restrict__ wy, const int* __restrict__ sy, int Ty) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= ow || y >= oh) return;
  src += blockIdx.z * sfp;
  dst += blockIdx.z * dfp;
  float acc = 0.0f;
  for (int j = 0; j < Ty; j++) {
    int r = sy[y] + j;
    r = r < 0 ? 0 : (r > sh - 1 ? sh - 1 : r);
    const uint8_t* row = src + r * sls;
    float h = 0.0f;
    for (int i = 0; i < Tx; i++) {
      int c = sx[x] + i;
      c = c < 0 ? 0 : (c > sw - 1 ? sw - 1 : c);
      h = fmaf(wx[x * Tx + i], (float)row[c], h);
    }
    acc = fmaf(wy[y * Ty + j], h, acc);
  }
  const float v = floorf(acc + 0.5f);
  dst[y * dls + x] = (uint8_t)(v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v));
}

// yuv420p (BT.709, limited) -> RGB24 full range, chroma of pixel (x, y) from
// sample (x/2, y/2); then the display-gamma LUT
__global__ void k_yuv8_rgb24(const uint8_t* __restrict__ yp, long long yls, const uint8_t* __restrict__ up,
                             const uint8_t* __restrict__ vp, long long cls, long long yuv_fp, int w, int h,
                             uint8_t* __restrict__ rgb, long long rls, long long rgb_fp,
                             const uint8_t* __restrict__ glut) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= w || y >= h) return;
  yp += blockIdx.z * yuv_fp, up += blockIdx.z * yuv_fp, vp += blockIdx.z * yuv_fp;
  rgb += blockIdx.z * rgb_fp;
  const float Y = 1.16438356f * ((float)yp[y * yls + x] - 16.0f);
  const float U = (float)up[(y >> 1) * cls + (x >> 1)] - 128.0f;
  const float V = (float)vp[(y >> 1) * cls + (x >> 1)] - 128.0f;
  const float c[3] = {fmaf(1.79274107f, V, Y), fmaf(-0.53290933f, V, fmaf(-0.21324861f, U, Y)), fmaf(2.11240179f, U, Y)};
  uint8_t* o = rgb + y * rls + 3 * x;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float v = floorf(c[k] + 0.5f);
    o[k] = glut[(int)(v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v))];
  }
}

hipError_t launch_resize_u8(const uint8_t* src, int sw, int sh, long long sls, long long sfp, uint8_t* dst, int ow,
                            int oh, long long dls, long long dfp, const float* wx, const int* sx, int Tx,
                            const float* wy, const int* sy, int Ty, int nframes, hipStream_t s) {
  hipLaunchKernelGGL(k_resize_u8, dim3((ow + 255) / 256, oh, nframes), dim3(256), 0, s, src, sw, sh, sls, sfp, dst, ow,
                     oh, dls, dfp, wx, sx, Tx, wy, sy, Ty);
  return hipGetLastError();
}

hipError_t launch_yuv8_rgb24(const uint8_t* yp, long long yls, const uint8_t* up, const uint8_t* vp, long long cls,
                             long long yuv_fp, int w, int h, uint8_t* rgb, long long rls, long long rgb_fp,
                             const uint8_t* glut, int nframes, hipStream_t s) {
  hipLaunchKernelGGL(k_yuv8_rgb24, dim3((w + 255) / 256, h, nframes), dim3(256), 0, s, yp, yls, up, vp, cls, yuv_fp, w,
                     h, rgb, rls, rgb_fp, glut);
  return hipGetLastError();
}

// ---- the source pane ---------------------------------------------------------
// One swscale context from the source format to packed RGB: nothing is rounded
// between the resize and the matrix, and packed RGB output is horizontally 2:1
// chroma (pixel (x, y) takes the resized chroma sample (x >> 1, y)).

// separable bicubic gather of one 16-bit plane (pw x ph, samples `step` words
// apart) at one output sample: sum of w * (code - bias), source indices clamped
// at the edges; wx / wy point at the output sample's own Tx / Ty weights
__device__ __forceinline__ float src_taps(const SrcPreviewParams& P, const uint8_t* __restrict__ plane, long long ls,
                                          int step, int pw, int ph, const float* __restrict__ wx, int x0, int Tx,
                                          const float* __restrict__ wy, int y0, int Ty, int bias) {
  float acc = 0.0f;
  for (int j = 0; j < Ty; j++) {
    int r = y0 + j;
    r = r < 0 ? 0 : (r > ph - 1 ? ph - 1 : r);
    const uint16_t* row = (const uint16_t*)(plane + r * ls);
    float h = 0.0f;
    for (int i = 0; i < Tx; i++) {
      int c = x0 + i;
      c = c < 0 ? 0 : (c > pw - 1 ? pw - 1 : c);
      h = fmaf(wx[i], (float)((int)((row[(long long)c * step] >> P.sh) & P.mask) - bias), h);
    }
    acc = fmaf(wy[j], h, acc);
  }
  return acc;
}

// a thread owns the horizontal pixel pair (2p, 2p + 1) of row y, which shares
// chroma sample p; blockIdx.z is the frame.  At odd ow the last pair is half
__global__ void __launch_bounds__(256) k_source_rgb24(const SrcPreviewParams P) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (p >= P.ow2 || y >= P.oh) return;
  const long long f = blockIdx.z;
  const uint8_t* yp = P.in[0] + f * P.fp[0];
  const uint8_t* up = P.in[1] + f * P.fp[1];
  const uint8_t* vp = P.in[2] + f * P.fp[2];
  const int x0 = 2 * p, npx = x0 + 1 < P.ow ? 2 : 1;
  float Y[2] = {0.0f, 0.0f};
  if (P.identity) {
    const uint16_t* row = (const uint16_t*)(yp + y * P.ls[0]);
    for (int k = 0; k < npx; k++) Y[k] = (float)((int)((row[x0 + k] >> P.sh) & P.mask) - P.y_off);
  } else {
    for (int k = 0; k < npx; k++)
      Y[k] = src_taps(P, yp, P.ls[0], 1, P.W, P.H, P.wx + (long long)(x0 + k) * P.Tx, P.sx[x0 + k], P.Tx,
                      P.wy + (long long)y * P.Ty, P.sy[y], P.Ty, P.y_off);
  }
  const float* wcx = P.wcx + (long long)p * P.Tcx;
  const float* wcy = P.wcy + (long long)y * P.Tcy;
  const float Cb = P.c_inv * src_taps(P, up, P.ls[1], P.cstep, P.cw, P.ch, wcx, P.scx[p], P.Tcx, wcy, P.scy[y], P.Tcy, P.mid);
  const float Cr = P.c_inv * src_taps(P, vp, P.ls[2], P.cstep, P.cw, P.ch, wcx, P.scx[p], P.Tcx, wcy, P.scy[y], P.Tcy, P.mid);
  const float dr = P.m_rcr * Cr, dg = fmaf(P.m_gcr, Cr, P.m_gcb * Cb), db = P.m_bcb * Cb;
  uint8_t o[6];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const float Yn = P.y_inv * Y[k];
    const float c[3] = {Yn + dr, Yn + dg, Yn + db};
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const float v = c[q] < 0.0f ? 0.0f : (c[q] > 1.0f ? 1.0f : c[q]);
      o[3 * k + q] = P.round8 ? (uint8_t)(int)floorf(fmaf(255.0f, v, 0.5f))
                              : (uint8_t)((int)floorf(fmaf(65535.0f, v, 0.5f)) >> 8);
    }
  }
  // the pair's 6 bytes lie 6 p into a row of any byte alignment: stored as a
  // unit (unaligned vector stores), a half pair as its 3 bytes
  uint8_t* dst = P.rgb + f * P.rfp + y * P.rls + 6LL * p;
  if (npx == 2) memcpy(dst, o, 6);
  else memcpy(dst, o, 3);
}

hipError_t launch_source_rgb24(const SrcPreviewParams& P, int nframes, hipStream_t s) {
  const dim3 block(64, 4);
  hipLaunchKernelGGL(k_source_rgb24, dim3((P.ow2 + block.x - 1) / block.x, (P.oh + block.y - 1) / block.y, nframes),
                     block, 0, s, P);
  return hipGetLastError();
}

}  // namespace h2s
